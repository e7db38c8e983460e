"""DPM-Solver++(2M) and Karras sigmas, the host side (no GPU): the scheduler tables, the C entry point's argument checks
and DenoiseLoop's solver buffers."""
import numpy as np
import pytest
import torch

from stabletriton_amd import _C
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import (DPMSolverTables, EulerTables, dpmpp_2m_tables, euler_discrete_tables, sigma_to_t,
                                        training_sigmas)

SIGMA_MAX, SIGMA_MIN = 14.6146, 0.029167


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("n", [1, 2, 10, 25, 50])
@pytest.mark.parametrize("karras", [False, True])
def test_dpmpp_tables_are_the_euler_tables(n, karras):
    d, e = dpmpp_2m_tables(n, karras=karras), euler_discrete_tables(n, karras=karras)
    assert isinstance(d, DPMSolverTables) and not isinstance(d, EulerTables)
    assert d.timesteps.dtype == d.sigmas.dtype == np.float32
    assert d.timesteps.tobytes() == e.timesteps.tobytes() and d.sigmas.tobytes() == e.sigmas.tobytes()
    assert d.init_noise_sigma == e.init_noise_sigma and d.n_steps == e.n_steps == n
    assert d.in_scale().tobytes() == e.in_scale().tobytes()


def test_euler_default_tables_unchanged():
    """Values of the default (leading-spacing) tables as they were before Karras sigmas existed."""
    e = euler_discrete_tables(50)
    assert e.timesteps[:4].tolist() == [981.0, 961.0, 941.0, 921.0] and e.timesteps[-1] == 1.0
    np.testing.assert_array_equal(e.sigmas[:3], np.array([13.120411, 11.676046, 10.425041], dtype=np.float32))
    assert e.sigmas[-1] == 0.0 and len(e.sigmas) == 51
    assert e.sigmas[-2] == np.float32(0.041314412)
    assert e.init_noise_sigma == float.fromhex("0x1.a5122359c41c5p+3")
    assert e.dsigma()[0] == np.float32(-1.4443645) and e.in_scale()[0] == np.float32(0.07599671)
    e10 = euler_discrete_tables(10)
    assert e10.timesteps.tolist() == [901.0, 801.0, 701.0, 601.0, 501.0, 401.0, 301.0, 201.0, 101.0, 1.0]
    k = euler_discrete_tables(10, karras=False)
    assert e10.timesteps.tobytes() == k.timesteps.tobytes() and e10.sigmas.tobytes() == k.sigmas.tobytes()


@pytest.mark.parametrize("n", [2, 10, 25, 30])
def test_karras_sigmas(n):
    t = euler_discrete_tables(n, karras=True)
    s = t.sigmas
    assert len(s) == n + 1 and s[-1] == 0.0 and s.dtype == np.float32
    assert s[0] == pytest.approx(SIGMA_MAX, abs=1e-4) and s[n - 1] == pytest.approx(SIGMA_MIN, abs=1e-6)
    allsig = training_sigmas()
    assert s[0] == np.float32(allsig.max()) and s[n - 1] == np.float32(allsig.min())
    assert np.all(np.diff(s.astype(np.float64)) < 0)
    # the rho = 7 formula, in float64
    rho, lo, hi = 7.0, allsig.min() ** (1 / 7.0), allsig.max() ** (1 / 7.0)
    want = np.array([(hi + i / (n - 1) * (lo - hi)) ** rho for i in range(n)])
    np.testing.assert_array_equal(s[:-1], want.astype(np.float32))
    assert t.init_noise_sigma == pytest.approx(float(np.sqrt(want[0] ** 2 + 1.0)), rel=1e-15)
    # timesteps: fractional, decreasing, in [0, 999], log-sigma linear between integer t
    ts = t.timesteps.astype(np.float64)
    assert ts[0] == 999.0 and 0.0 <= ts[-1] < 1e-6 and np.all(np.diff(ts) < 0)
    assert n == 2 or any(x != np.floor(x) for x in ts[1:-1])              # not rounded
    for sig, tv in zip(want, ts):
        lo_t = int(np.floor(tv))
        if lo_t >= 999:
            continue
        w = tv - lo_t
        logs = (1 - w) * np.log(allsig[lo_t]) + w * np.log(allsig[lo_t + 1])
        assert logs == pytest.approx(np.log(sig), abs=1e-4)


def test_sigma_to_t_maps_training_sigmas_to_integers():
    allsig = training_sigmas()
    for k in (0, 1, 17, 500, 998, 999):
        assert sigma_to_t(np.array([allsig[k]]), allsig)[0] == float(k)
    mid = np.exp(0.5 * (np.log(allsig[300]) + np.log(allsig[301])))
    assert sigma_to_t(np.array([mid]), allsig)[0] == pytest.approx(300.5, abs=1e-9)


def _restated_coefficients(sigmas):
    s = [float(v) for v in sigmas]
    n = len(s) - 1
    rows = []
    for i in range(n):
        if s[i + 1] == 0.0:
            rows.append([s[i], 0.0, 1.0, 0.0])
            continue
        lam, lam_next = -np.log(s[i]), -np.log(s[i + 1])
        h = lam_next - lam
        a, b = s[i + 1] / s[i], -np.expm1(-h)
        k = 0.0
        if 0 < i < n - 1:
            r = (lam - (-np.log(s[i - 1]))) / h
            k = 1.0 / (2.0 * r)
        rows.append([s[i], a, b, k])
    return np.array(rows, dtype=np.float64)


@pytest.mark.parametrize("n", [2, 10, 25, 50])
@pytest.mark.parametrize("karras", [False, True])
def test_coefficients(n, karras):
    t = dpmpp_2m_tables(n, karras=karras)
    c = t.coefficients()
    assert c.shape == (n, 4) and c.dtype == np.float32
    assert c[0, 3] == 0.0 and c[-1, 3] == 0.0                       # first-order: the first and the last step
    assert c[-1, 1] == 0.0 and c[-1, 2] == 1.0                      # last step: x = d
    np.testing.assert_array_equal(c[:, 0], t.sigmas[:-1])
    want = _restated_coefficients(t.sigmas)
    np.testing.assert_allclose(c.astype(np.float64), want, rtol=2 ** -23, atol=0)
    if n > 2:
        assert np.all(c[1:-1, 3] > 0.0)
    # a + b relation: a = exp(-h), b = 1 - exp(-h) (k-diffusion's sigma form)
    np.testing.assert_allclose(c[:-1, 1].astype(np.float64) + c[:-1, 2], 1.0, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ the C entry point
P = 1 << 20            # fake, aligned, never dereferenced device addresses: validation happens before any launch


def _dpm(lib, **kw):
    a = dict(latent=P, eps=P, next_in=P, history=P, coef=P, in_scale=P, guidance=None, rescale=None, step=P, start=P, batch=1,
             per_sample=1024, n_steps=25, dtype=_C.ST_BF16, workspace=None, workspace_bytes=0)
    a.update(kw)
    return lib.st_dpmpp2m_step(a["latent"], a["eps"], a["next_in"], a["history"], a["coef"], a["in_scale"], a["guidance"],
                               a["rescale"], a["step"], a["start"], a["batch"], a["per_sample"], a["n_steps"], a["dtype"],
                               a["workspace"], a["workspace_bytes"], None)


def test_dpmpp_step_entry_point_validates_on_host(lib):
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    assert "st_dpmpp2m_step" in _C.SIGNATURES
    for name in ("latent", "eps", "next_in", "history", "coef", "in_scale", "step", "start"):
        assert _dpm(lib, **{name: None}) != 0 and b"null" in lib.st_last_error(), name
    assert _dpm(lib, rescale=P) != 0 and b"guidance" in lib.st_last_error()
    assert _dpm(lib, per_sample=1020) != 0 and b"multiple of 8" in lib.st_last_error()
    for bad in (dict(batch=0), dict(per_sample=0), dict(n_steps=0)):
        assert _dpm(lib, **bad) != 0 and b"bad sizes" in lib.st_last_error(), bad
    assert _dpm(lib, batch=70000) != 0 and b"grid" in lib.st_last_error()
    for name in ("latent", "eps", "next_in", "history"):
        assert _dpm(lib, **{name: P + 4}) != 0 and b"aligned" in lib.st_last_error(), name
    assert _dpm(lib, dtype=7) != 0 and b"dtype" in lib.st_last_error()
    assert _dpm(lib, dtype=_C.ST_F32S, guidance=P) != 0 and b"dtype" in lib.st_last_error()
    need = lib.st_cfg_step_workspace_bytes(3, 4 * 128 * 128)
    for ws, nbytes in ((None, 0), (P, need - 1)):
        rc = _dpm(lib, batch=3, per_sample=4 * 128 * 128, guidance=P, rescale=P, workspace=ws, workspace_bytes=nbytes)
        assert rc != 0 and b"workspace" in lib.st_last_error()
    rc = _dpm(lib, batch=3, per_sample=4 * 128 * 128, guidance=P, rescale=P, workspace=P + 8, workspace_bytes=need)
    assert rc != 0 and b"aligned" in lib.st_last_error()
    rc = _dpm(lib, batch=3, per_sample=4 * 128 * 128, guidance=P, rescale=P, workspace=P, workspace_bytes=need, dtype=9)
    assert rc != 0 and b"dtype" in lib.st_last_error()                  # a valid workspace: the dtype is what fails


# ------------------------------------------------------------------------------------------------ DenoiseLoop (CPU tensors)
class _NoUNet:
    """Stands in for a compiled UNet: the host-side paths below never evaluate it."""


def _loop(tables, **kw):
    return DenoiseLoop(_NoUNet(), kw.pop("batch", 2), kw.pop("hw", 16), torch.float32, "cpu", tables, cross_dim=8,
                       pooled_dim=6, tokens=3, **kw)


@pytest.mark.parametrize("guided", [False, True])
def test_loop_buffers(guided):
    kw = dict(guidance_scale=5.0, guidance_rescale=0.7) if guided else {}
    t = dpmpp_2m_tables(10, karras=True)
    lp = _loop(t, hw=(24, 16), mode="step", **kw)
    assert lp.history.shape == lp.latent.shape == (2, 4, 24, 16) and lp.history.dtype == torch.float32
    assert lp.history.is_contiguous(memory_format=torch.channels_last) and lp.history.data_ptr() != lp.latent.data_ptr()
    assert torch.equal(lp.coef, torch.from_numpy(t.coefficients())) and lp.coef.dtype == torch.float32
    assert lp.start.dtype == torch.int32 and lp.start.shape == (1,) and int(lp.start) == 0
    assert lp.dsigma is None
    assert lp.x_in.shape[0] == (4 if guided else 2)
    eu = _loop(euler_discrete_tables(10), **kw)
    assert eu.history is None and eu.coef is None and eu.start is None
    assert torch.equal(eu.dsigma, torch.from_numpy(euler_discrete_tables(10).dsigma()))


@pytest.mark.parametrize("guided", [False, True])
def test_set_noise_and_set_image(guided):
    kw = dict(guidance_scale=5.0) if guided else {}
    t = dpmpp_2m_tables(10, karras=True)
    lp = _loop(t, mode="step", **kw)
    z = torch.randn(2, 4, 16, 16)
    lp.start.fill_(7)
    lp.set_noise(z)
    assert int(lp.start) == 0 and int(lp.step) == 0
    want = (z * t.init_noise_sigma) * float(t.in_scale()[0])
    assert torch.equal(lp.x_in[:2], want)
    if guided:
        assert torch.equal(lp.x_in[2:], want)
    init = torch.randn(2, 4, 16, 16)
    left = lp.set_image(init, z, 0.5)
    assert left == 5 and int(lp.start) == 5 and int(lp.step) == 5
    assert torch.equal(lp.latent, init + z * float(t.sigmas[5]))
    assert torch.equal(lp.x_in[:2], lp.latent * float(t.in_scale()[5]))
    lp.set_image(init, z, 0.8)
    assert int(lp.start) == 2
    eager = _loop(t, mode="eager", **kw)
    assert eager.set_image(init, z, 0.3) == 3 and int(eager.start) == 7
    with pytest.raises(ValueError, match="mode='step' or 'eager'"):
        _loop(t, mode="loop", **kw).set_image(init, z, 0.5)
