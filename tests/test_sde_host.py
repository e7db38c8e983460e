"""Euler ancestral and DPM++ 2M SDE, the host side (no GPU): the counter-based generator's restatement (rng.py), the
scheduler tables, the C entry points' argument checks and DenoiseLoop's buffers and seeds."""
import math

import numpy as np
import pytest
import torch

from stabletriton_amd import _C, rng
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import (DPMSolverTables, EulerTables, SDETables, dpmpp_2m_sde_tables, dpmpp_2m_tables,
                                        euler_ancestral_tables, euler_discrete_tables)


# ------------------------------------------------------------------------------------------------ the generator
def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    """Random123's known-answer vectors for Philox4x32-10."""
    assert _hex(rng.philox4x32_10([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(rng.philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    got = rng.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])
    assert _hex(got) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_is_vectorised():
    ctr = np.array([[0, 0, 0, 0], [0xffffffff] * 4], dtype=np.uint64)
    key = np.array([[0, 0], [0xffffffff] * 2], dtype=np.uint64)
    out = rng.philox4x32_10(ctr, key)
    assert out.shape == (2, 4) and out.dtype == np.uint64
    assert _hex(out[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and _hex(out[1]) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_uniform_is_open_and_exact_in_fp32():
    u = np.array([0, 511, 512, 0xffffffff, 0x80000000], dtype=np.uint64)
    p = rng.uniform_open(u)
    assert np.all(p > 0.0) and np.all(p < 1.0)
    assert p[0] == p[1] == 2.0 ** -24 and p[3] == 1.0 - 2.0 ** -24
    np.testing.assert_array_equal(p.astype(np.float32).astype(np.float64), p)


def test_normal_layout_matches_the_definition():
    """Element j of a sample: Philox call j >> 2 under (seed lo, seed hi), counter word C, Box-Muller pairs (0,1), (2,3)."""
    seed, ctr = (7 << 32) | 123, 9
    z = rng.normal([seed], ctr, 16)[0]
    for q in range(4):
        u = rng.philox4x32_10([q, ctr, 0, 0], [123, 7])
        p = rng.uniform_open(u)
        r0, r2 = math.sqrt(-2 * math.log(p[0])), math.sqrt(-2 * math.log(p[2]))
        want = [r0 * math.cos(2 * math.pi * p[1]), r0 * math.sin(2 * math.pi * p[1]),
                r2 * math.cos(2 * math.pi * p[3]), r2 * math.sin(2 * math.pi * p[3])]
        np.testing.assert_allclose(z[4 * q:4 * q + 4], want, rtol=1e-15, atol=1e-15)
    # a longer row starts with the same values (the stream does not depend on per_sample)
    assert np.array_equal(rng.normal(seed, ctr, 64)[0, :16], z)


def test_normal_rejects_bad_arguments():
    with pytest.raises(ValueError, match="multiple of 4"):
        rng.normal(0, 0, 6)
    with pytest.raises(ValueError, match="64-bit"):
        rng.normal([-1], 0, 8)
    with pytest.raises(ValueError, match="64-bit"):
        rng.normal([1 << 64], 0, 8)
    with pytest.raises(ValueError, match="32-bit"):
        rng.normal(0, 1 << 32, 8)


N_STAT = 1 << 20


def test_normal_statistics():
    """2^20 values per stream; deterministic, so these bounds cannot flake."""
    from scipy import stats                          # imported here: collecting this module loads no extra libraries
    seeds = [0, 1 << 32, (1 << 64) - 1, 0x9E3779B97F4A7C15]
    z = rng.normal(seeds, 1, N_STAT)
    se = 1.0 / math.sqrt(N_STAT)
    for row in z:
        assert abs(row.mean()) < 4 * se
        assert abs(row.var() - 1.0) < 4 * math.sqrt(2.0) * se
        assert stats.kstest(row, "norm").pvalue > 1e-3
        assert np.abs(row).max() < 6.0
    # between seeds, between counter words, between neighbouring elements (and the two halves of a Box-Muller pair)
    c = rng.normal([seeds[0]], 2, N_STAT)[0]
    pairs = [(z[0], z[1]), (z[0], z[2]), (z[2], z[3]), (z[0], c), (z[0][:-1], z[0][1:]), (z[0][:-4], z[0][4:])]
    for a, b in pairs:
        assert abs(np.corrcoef(a, b)[0, 1]) < 5 * se
    even, odd = z[0][0::2], z[0][1::2]
    assert abs(np.corrcoef(even, odd)[0, 1]) < 5 * math.sqrt(2.0) * se


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("make", [euler_ancestral_tables, dpmpp_2m_sde_tables])
@pytest.mark.parametrize("n", [1, 2, 10, 25, 50])
@pytest.mark.parametrize("karras", [False, True])
def test_sde_tables_are_the_euler_tables(make, n, karras):
    t, e = make(n, karras=karras), euler_discrete_tables(n, karras=karras)
    assert isinstance(t, SDETables) and not isinstance(t, (DPMSolverTables, EulerTables))
    assert t.timesteps.tobytes() == e.timesteps.tobytes() and t.sigmas.tobytes() == e.sigmas.tobytes()
    assert t.init_noise_sigma == e.init_noise_sigma and t.n_steps == n
    assert t.in_scale().tobytes() == e.in_scale().tobytes()
    assert t.eta == 1.0 and t.s_noise == 1.0
    c = t.coefficients()
    assert c.shape == (n, 5) and c.dtype == np.float32
    np.testing.assert_array_equal(c[:, 0], t.sigmas[:-1])
    assert c[-1].tolist() == [float(t.sigmas[-2]), 0.0, 1.0, 0.0, 0.0]            # the last row: x = d, no noise


def test_default_step_counts():
    assert euler_ancestral_tables().n_steps == 50 and dpmpp_2m_sde_tables().n_steps == 25
    assert euler_ancestral_tables().sampler == "euler_ancestral" and dpmpp_2m_sde_tables().sampler == "dpmpp_2m_sde"
    with pytest.raises(ValueError, match="sampler"):
        SDETables(np.zeros(1, np.float32), np.zeros(2, np.float32), 1.0, "heun")
    with pytest.raises(ValueError, match="eta"):
        euler_ancestral_tables(10, eta=-1.0)


@pytest.mark.parametrize("n", [2, 10, 50])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("eta,s_noise", [(1.0, 1.0), (0.5, 1.0), (1.0, 0.8), (0.0, 1.0)])
def test_euler_ancestral_rows(n, karras, eta, s_noise):
    t = euler_ancestral_tables(n, karras=karras, eta=eta, s_noise=s_noise)
    c = t.coefficients()
    s = t.sigmas.astype(np.float64)
    for i in range(n - 1):
        sc, sn = s[i], s[i + 1]
        up = min(sn, eta * math.sqrt(sn ** 2 * (sc ** 2 - sn ** 2) / sc ** 2))
        down = math.sqrt(sn ** 2 - up ** 2)
        assert down ** 2 + up ** 2 == pytest.approx(sn ** 2, rel=1e-12)
        want = [sc, down / sc, 1.0 - down / sc, 0.0, s_noise * up]
        np.testing.assert_allclose(c[i].astype(np.float64), want, rtol=2 ** -23, atol=1e-30)
        # the row form is x + (sigma_down - s) e + sigma_up z: a x + b (x - s e) = x - b s e
        assert float(c[i, 1]) + float(c[i, 2]) == pytest.approx(1.0, abs=1e-7)
        assert -float(c[i, 2]) * sc == pytest.approx(down - sc, rel=1e-6, abs=1e-6)
    if eta == 0.0:                                                    # deterministic: the Euler step, no noise
        assert np.all(c[:, 4] == 0.0) and np.allclose(c[:-1, 1], s[1:-1] / s[:-2], rtol=1e-6)


@pytest.mark.parametrize("n", [2, 10, 25, 50])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("eta,s_noise", [(1.0, 1.0), (0.5, 0.9)])
def test_dpmpp_2m_sde_rows(n, karras, eta, s_noise):
    t = dpmpp_2m_sde_tables(n, karras=karras, eta=eta, s_noise=s_noise)
    c = t.coefficients()
    s = t.sigmas.astype(np.float64)
    for i in range(n - 1):
        h = math.log(s[i]) - math.log(s[i + 1])
        k = 0.0 if i == 0 else 1.0 / (2.0 * ((math.log(s[i - 1]) - math.log(s[i])) / h))
        want = [s[i], s[i + 1] / s[i] * math.exp(-eta * h), -math.expm1(-(1.0 + eta) * h), k,
                s_noise * s[i + 1] * math.sqrt(-math.expm1(-2.0 * eta * h))]
        np.testing.assert_allclose(c[i].astype(np.float64), want, rtol=4 * 2 ** -23, atol=0)
    assert c[0, 3] == 0.0 and np.all(c[:-1, 4] > 0.0)


@pytest.mark.parametrize("n", [1, 2, 10, 25, 50])
@pytest.mark.parametrize("karras", [False, True])
def test_dpmpp_2m_sde_eta0_is_dpmpp_2m_bit_for_bit(n, karras):
    sde = dpmpp_2m_sde_tables(n, karras=karras, eta=0.0).coefficients()
    dpm = dpmpp_2m_tables(n, karras=karras).coefficients()
    assert sde[:, :4].tobytes() == dpm.tobytes()
    assert np.all(sde[:, 4] == 0.0)


# ------------------------------------------------------------------------------------------------ the C entry points
P = 1 << 20            # fake, aligned, never dereferenced device addresses: validation happens before any launch


def _sde(lib, **kw):
    a = dict(latent=P, eps=P, next_in=P, history=P, coef=P, in_scale=P, guidance=None, rescale=None, step=P, start=P, seeds=P,
             batch=1, per_sample=1024, n_steps=25, dtype=_C.ST_BF16, workspace=None, workspace_bytes=0)
    a.update(kw)
    return lib.st_sde_step(a["latent"], a["eps"], a["next_in"], a["history"], a["coef"], a["in_scale"], a["guidance"],
                           a["rescale"], a["step"], a["start"], a["seeds"], a["batch"], a["per_sample"], a["n_steps"],
                           a["dtype"], a["workspace"], a["workspace_bytes"], None)


def test_sde_step_entry_point_validates_on_host(lib):
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    assert "st_sde_step" in _C.SIGNATURES and "st_philox_normal" in _C.SIGNATURES
    for name in ("latent", "eps", "next_in", "history", "coef", "in_scale", "step", "start", "seeds"):
        assert _sde(lib, **{name: None}) != 0 and b"null" in lib.st_last_error(), name
    assert _sde(lib, rescale=P) != 0 and b"guidance" in lib.st_last_error()
    assert _sde(lib, per_sample=1020) != 0 and b"multiple of 8" in lib.st_last_error()
    for bad in (dict(batch=0), dict(per_sample=0), dict(n_steps=0)):
        assert _sde(lib, **bad) != 0 and b"bad sizes" in lib.st_last_error(), bad
    assert _sde(lib, per_sample=(4 << 32) + 8) != 0 and b"generator" in lib.st_last_error()
    assert _sde(lib, batch=70000) != 0 and b"grid" in lib.st_last_error()
    for name in ("latent", "eps", "next_in", "history"):
        assert _sde(lib, **{name: P + 4}) != 0 and b"aligned" in lib.st_last_error(), name
    assert _sde(lib, seeds=P + 4) != 0 and b"seeds" in lib.st_last_error()
    assert _sde(lib, dtype=7) != 0 and b"dtype" in lib.st_last_error()
    assert _sde(lib, dtype=_C.ST_F32S, guidance=P) != 0 and b"dtype" in lib.st_last_error()
    need = lib.st_cfg_step_workspace_bytes(3, 4 * 128 * 128)
    for ws, nbytes in ((None, 0), (P, need - 1)):
        rc = _sde(lib, batch=3, per_sample=4 * 128 * 128, guidance=P, rescale=P, workspace=ws, workspace_bytes=nbytes)
        assert rc != 0 and b"workspace" in lib.st_last_error()
    rc = _sde(lib, batch=3, per_sample=4 * 128 * 128, guidance=P, rescale=P, workspace=P + 8, workspace_bytes=need)
    assert rc != 0 and b"aligned" in lib.st_last_error()
    rc = _sde(lib, batch=3, per_sample=4 * 128 * 128, guidance=P, rescale=P, workspace=P, workspace_bytes=need, dtype=9)
    assert rc != 0 and b"dtype" in lib.st_last_error()                  # a valid workspace: the dtype is what fails


def test_philox_normal_entry_point_validates_on_host(lib):
    def call(out=P, seeds=P, batch=2, per_sample=64, counter=0):
        return lib.st_philox_normal(out, seeds, batch, per_sample, counter, None)
    for kw in (dict(out=None), dict(seeds=None)):
        assert call(**kw) != 0 and b"null" in lib.st_last_error(), kw
    for kw in (dict(batch=0), dict(per_sample=0), dict(per_sample=-4)):
        assert call(**kw) != 0 and b"bad sizes" in lib.st_last_error(), kw
    assert call(per_sample=66) != 0 and b"multiple of 4" in lib.st_last_error()
    assert call(per_sample=(4 << 32) + 4) != 0 and b"generator" in lib.st_last_error()
    assert call(batch=70000) != 0 and b"grid" in lib.st_last_error()
    assert call(out=P + 4) != 0 and b"aligned" in lib.st_last_error()
    assert call(seeds=P + 4) != 0 and b"seeds" in lib.st_last_error()


def test_ops_reject_cpu_tensors():
    from stabletriton_amd import ops
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.philox_normal(torch.zeros(1, 4, 4, 4), torch.zeros(1, dtype=torch.int64), 0)
    lat = torch.zeros(1, 4, 4, 4)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.sde_step(lat, lat, lat, lat, torch.zeros(10, 5), torch.zeros(10), torch.zeros(1, dtype=torch.int32),
                     torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ DenoiseLoop (CPU tensors)
class _NoUNet:
    """Stands in for a compiled UNet: the host-side paths below never evaluate it."""


def _loop(tables, **kw):
    return DenoiseLoop(_NoUNet(), kw.pop("batch", 2), kw.pop("hw", 16), torch.float32, "cpu", tables, cross_dim=8,
                       pooled_dim=6, tokens=3, **kw)


@pytest.mark.parametrize("make", [euler_ancestral_tables, dpmpp_2m_sde_tables])
@pytest.mark.parametrize("guided", [False, True])
def test_loop_buffers(make, guided):
    kw = dict(guidance_scale=5.0, guidance_rescale=0.7) if guided else {}
    t = make(10, karras=True)
    lp = _loop(t, hw=(24, 16), mode="step", **kw)
    assert lp.history.shape == lp.latent.shape == (2, 4, 24, 16) and lp.history.dtype == torch.float32
    assert lp.history.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(lp.coef, torch.from_numpy(t.coefficients())) and tuple(lp.coef.shape) == (10, 5)
    assert lp.start.dtype == torch.int32 and int(lp.start) == 0
    assert lp.seeds.dtype == torch.int64 and tuple(lp.seeds.shape) == (2,) and lp.seeds.tolist() == [0, 0]
    assert lp.dsigma is None
    assert lp.x_in.shape[0] == (4 if guided else 2)
    # Euler and DPM++ keep their buffers and have no seed table until a seed is used
    eu = _loop(euler_discrete_tables(10), **kw)
    assert eu.seeds is None and eu.history is None and eu.coef is None
    dpm = _loop(dpmpp_2m_tables(10), **kw)
    assert dpm.seeds is None and tuple(dpm.coef.shape) == (10, 4)
    eu.set_seed([5, 6])
    assert eu.seeds.tolist() == [5, 6] and eu.seeds.dtype == torch.int64


def test_set_seed():
    lp = _loop(dpmpp_2m_sde_tables(10), batch=3)
    addr = lp.seeds.data_ptr()
    lp.set_seed(7)
    assert lp.seeds.tolist() == [7, 8, 9]
    lp.set_seed([1, 1 << 63, (1 << 64) - 1])
    assert lp.seeds.tolist() == [1, -(1 << 63), -1]                      # int64 holding the seeds' 64 bits
    lp.set_seed(np.uint64((1 << 64) - 1))
    assert lp.seeds.tolist() == [-1, 0, 1]                               # s + b wraps mod 2^64
    lp.set_seed((np.int64(3), 4, 5))
    assert lp.seeds.tolist() == [3, 4, 5]
    assert lp.seeds.data_ptr() == addr                                   # in place: a captured graph keeps reading it
    for bad, msg in (([1, 2], "B = 3"), ([1, 2, 3, 4], "B = 3"), (-1, "64-bit"), (1 << 64, "64-bit"),
                     ([0, 1, -2], "64-bit"), (1.5, "one int"), ([1.0, 2, 3], "integers"), (True, "one int"),
                     ("seed", "integers")):
        with pytest.raises(ValueError, match=msg):
            lp.set_seed(bad)
    assert lp.seeds.tolist() == [3, 4, 5]                                # a rejected call writes nothing


def test_set_noise_arguments():
    lp = _loop(euler_ancestral_tables(10), mode="step")
    with pytest.raises(ValueError, match="latent_unit, seed, or both"):
        lp.set_noise()
    z = torch.randn(2, 4, 16, 16)
    lp.set_noise(z, seed=[3, 4])                                         # a tensor and a seed: the tensor starts, the seed drives the steps
    assert lp.seeds.tolist() == [3, 4] and torch.equal(lp.latent, z * lp.tables.init_noise_sigma)
    lp.start.fill_(4)
    left = lp.set_image(torch.zeros(2, 4, 16, 16), z, 0.5, seed=11)
    assert left == 5 and int(lp.start) == 5 and lp.seeds.tolist() == [11, 12]
    with pytest.raises(ValueError, match="noise_unit, seed, or both"):
        lp.set_image(torch.zeros(2, 4, 16, 16), None, 0.5)
