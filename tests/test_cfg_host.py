"""Classifier-free guidance in the denoise loop, the host side (no GPU): the C entry point's argument checks and
DenoiseLoop's guidance tables and [negative | positive] conditioning rows."""
import pytest
import torch

from stabletriton_amd import _C
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables

# host-side validation happens before any launch: fake, aligned, never dereferenced device addresses
P = 1 << 20


def _cfg(lib, **kw):
    a = dict(latent=P, eps=P, next_in=P, dsigma=P, in_scale=P, guidance=P, rescale=None, step=P, batch=1, per_sample=1024,
             n_steps=50, dtype=_C.ST_BF16, workspace=None, workspace_bytes=0)
    a.update(kw)
    return lib.st_cfg_euler_step(a["latent"], a["eps"], a["next_in"], a["dsigma"], a["in_scale"], a["guidance"], a["rescale"],
                                 a["step"], a["batch"], a["per_sample"], a["n_steps"], a["dtype"], a["workspace"],
                                 a["workspace_bytes"], None)


def test_cfg_step_entry_point_validates_on_host(lib):
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    for name in ("latent", "eps", "next_in", "dsigma", "in_scale", "guidance", "step"):
        assert _cfg(lib, **{name: None}) != 0 and b"null" in lib.st_last_error(), name
    assert _cfg(lib, per_sample=1020) != 0 and b"multiple of 8" in lib.st_last_error()
    assert _cfg(lib, batch=0) != 0 and b"bad sizes" in lib.st_last_error()
    assert _cfg(lib, eps=P + 2) != 0 and b"aligned" in lib.st_last_error()
    assert _cfg(lib, dtype=7, rescale=P, workspace=P, workspace_bytes=1 << 20) != 0 and b"dtype" in lib.st_last_error()
    need = lib.st_cfg_step_workspace_bytes(3, 4 * 128 * 128)
    assert need == 3 * (4 * 128 * 128 // 2048) * 4 * 8                 # one fp64 (sum, sum of squares) x 2 slot per block
    assert lib.st_cfg_step_workspace_bytes(1, 4 * 152 * 104) == 31 * 32     # a partial last block has a slot too
    for ws, nbytes in ((None, 0), (P, need - 1)):
        rc = _cfg(lib, batch=3, per_sample=4 * 128 * 128, rescale=P, workspace=ws, workspace_bytes=nbytes)
        assert rc != 0 and b"workspace" in lib.st_last_error()
    # (the plain path needs no workspace; its launch is what a GPU test covers)


class _NoUNet:
    """Stands in for a compiled UNet: the host-side paths below never evaluate it."""


def _loop(**kw):
    return DenoiseLoop(_NoUNet(), kw.pop("batch", 2), 16, torch.float32, "cpu", euler_discrete_tables(10), cross_dim=8,
                       pooled_dim=6, tokens=3, **kw)


def test_set_guidance_tables():
    lp = _loop(guidance_scale=5.0, guidance_rescale=0.7)
    assert lp.x_in.shape[0] == lp.ehs.shape[0] == lp.text_embeds.shape[0] == lp.time_ids.shape[0] == 4 and lp.latent.shape[0] == 2
    assert torch.equal(lp.guidance, torch.full((10,), 5.0)) and torch.equal(lp.rescale, torch.full((10,), 0.7))
    ramp = [1.0 + 0.5 * i for i in range(10)]
    lp.set_guidance(ramp)
    assert torch.equal(lp.guidance, torch.tensor(ramp)) and torch.equal(lp.rescale, torch.full((10,), 0.7))    # rescale kept
    lp.set_guidance(torch.tensor(7.5), 0.0)
    assert torch.equal(lp.guidance, torch.full((10,), 7.5)) and torch.equal(lp.rescale, torch.zeros(10))
    for bad in ([5.0] * 9, [5.0] * 11, []):
        with pytest.raises(ValueError, match="10 values"):
            lp.set_guidance(bad)
        with pytest.raises(ValueError, match="10 values"):
            lp.set_guidance(5.0, bad)
    assert torch.equal(lp.guidance, torch.full((10,), 7.5))              # a rejected call writes nothing
    with pytest.raises(ValueError, match="guidance_rescale"):
        _loop(guidance_scale=5.0).set_guidance(5.0, 0.5)
    with pytest.raises(ValueError, match="guidance_scale"):
        _loop().set_guidance(5.0)
    with pytest.raises(ValueError, match="guidance_scale"):
        _loop(guidance_rescale=0.5)


def test_unguided_loop_buffers_unchanged():
    lp = _loop()
    assert lp.x_in.shape[0] == lp.ehs.shape[0] == lp.latent.shape[0] == 2
    assert lp.guidance is None and lp.rescale is None and lp.cfg_workspace is None


def test_set_conditioning_rows():
    lp = _loop(guidance_scale=5.0)
    ehs, te, ti = torch.randn(2, 3, 8), torch.randn(2, 6), torch.randn(2, 6)
    lp.set_conditioning(ehs, te, ti)
    # no negative prompt: zeros for the text state and pooled embedding (force_zeros_for_empty_prompt), the positive time ids
    assert torch.equal(lp.ehs, torch.cat([torch.zeros_like(ehs), ehs])) and torch.equal(lp.text_embeds, torch.cat([torch.zeros_like(te), te]))
    assert torch.equal(lp.time_ids, torch.cat([ti, ti]))
    nehs, nte, nti = torch.randn(2, 3, 8), torch.randn(2, 6), torch.randn(2, 6)
    lp.set_conditioning(ehs, te, ti, nehs, nte, nti)
    assert torch.equal(lp.ehs, torch.cat([nehs, ehs])) and torch.equal(lp.text_embeds, torch.cat([nte, te]))
    assert torch.equal(lp.time_ids, torch.cat([nti, ti]))
    with pytest.raises(ValueError, match="guidance_scale"):
        _loop().set_conditioning(ehs, te, ti, negative_encoder_hidden_states=nehs)


def test_set_noise_fills_both_halves():
    lp = _loop(guidance_scale=5.0)
    z = torch.randn(2, 4, 16, 16)
    lp.set_noise(z)
    s = float(lp.tables.in_scale()[0])
    want = (z * lp.tables.init_noise_sigma) * s
    assert torch.equal(lp.x_in[:2], want) and torch.equal(lp.x_in[2:], want)
