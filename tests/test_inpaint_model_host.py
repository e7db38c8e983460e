"""Nine-channel inpainting checkpoints without a GPU: st_conv_stem's rejections (before any launch), InpaintCond.write's validation,
the fx routing of the stem, the loop's refusals."""
import dataclasses

import pytest
import torch

from stabletriton_amd import _C, inpaint as I
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.optimizers.wrappers import conv2d_wrapper, conv_stem_wrapper
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.unet import TINY, UNet2DConditionModel

# never dereferenced: every call below is rejected first.  a: 2 x 5 x 7 pixels of 4 bf16 = 560 bytes, out: 2 x 35 x 32 bf16 = 4480
A, B, W, BIAS, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def _call(lib, a=A, a_px=4, a_img=140, Na=2, C0=4, b=B, b_px=5, b_img=175, Nb=1, C1=5, w=W, bias=BIAS, out=OUT, N=2, H=5, W_=7, Cout=32,
          epi=_C.EPI_BIAS, dtype=_C.ST_BF16):
    return lib.st_conv_stem(a, a_px, a_img, Na, C0, b, b_px, b_img, Nb, C1, w, bias, out, N, H, W_, Cout, epi, dtype, None)


@pytest.mark.parametrize("msg,kw", [
    (b"null pointer", dict(a=None)), (b"null pointer", dict(b=None)), (b"null pointer", dict(w=None)), (b"null pointer", dict(out=None)),
    (b"without a bias pointer", dict(bias=None)), (b"unsupported dtype", dict(dtype=_C.ST_F32S)), (b"bad shape", dict(N=0)),
    (b"bad shape", dict(H=-1)), (b"bad shape", dict(C0=0)), (b"bad shape", dict(C1=-1)), (b"bad shape", dict(Nb=0)),
    (b"at most 16", dict(C0=12, a_px=12)), (b"multiple of 16", dict(Cout=40)), (b"must divide", dict(N=3, Na=3, Nb=2)),
    (b"must divide", dict(Na=4)), (b"bad strides", dict(a_px=3)), (b"bad strides", dict(b_px=4)), (b"not 16-byte aligned", dict(out=OUT + 8)),
    (b"not aligned to its element", dict(a=A + 1)), (b"overlap source a", dict(out=A + 256)), (b"overlap source b", dict(out=B - 4480 + 16)),
    (b"only ST_EPI_BIAS", dict(epi=_C.EPI_BIAS | _C.EPI_SILU)), (b"only ST_EPI_BIAS", dict(epi=_C.EPI_RESIDUAL)),
    (b"too large", dict(H=1 << 30, W_=1 << 30)), (b"too large", dict(a_img=1 << 61)),
])
def test_conv_stem_rejections(lib, msg, kw):
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    assert _call(lib, **kw) != 0 and msg in lib.st_last_error(), lib.st_last_error()


def test_write_validates_before_it_writes():
    st = I.InpaintCond()
    st.bind(4, (6, 8), "cpu", torch.float32, batch=2)
    buf = st.cond_for(4)
    assert tuple(buf.shape) == (2, 5, 6, 8) and buf.is_contiguous(memory_format=torch.channels_last) and not buf.any()
    mask, lat = torch.ones(6, 8), torch.randn(2, 4, 6, 8)
    bad_lat = lat.clone().index_fill_(3, torch.tensor([4]), float("inf"))
    for m, l in ((torch.ones(12, 16), lat), (mask, bad_lat), (mask, torch.randn(3, 4, 6, 8)), (torch.ones(3, 6, 8), lat), (mask * 2, lat),
                 (mask, lat[:, :3])):
        with pytest.raises(ValueError):
            st.write(m, l)
        assert not buf.any(), "a rejected write must leave the buffer alone"
    st.write(mask * 0.5, lat[:1])
    assert torch.equal(buf[:, :1], torch.full((2, 1, 6, 8), 0.5)) and torch.equal(buf[:, 1:], lat[:1].expand(2, -1, -1, -1))      # mask first


@pytest.mark.parametrize("cin,stems", [(9, 1), (4, 0)])
def test_replace_conv_routes_the_stem(cin, stems):
    gm = replace_backend(UNet2DConditionModel(dataclasses.replace(TINY, in_channels=cin)).eval())
    on_conv_in = [n.target for n in gm.graph.nodes if n.op == "call_function" and n.target in (conv2d_wrapper, conv_stem_wrapper)
                  and n.args[1].target == "conv_in"]
    assert on_conv_in == [conv_stem_wrapper if stems else conv2d_wrapper]
    assert isinstance(getattr(gm, "inpaint_cond", None), I.InpaintCond) == bool(stems)


def test_loop_refusals():
    nine = replace_backend(UNet2DConditionModel(dataclasses.replace(TINY, in_channels=9)).eval(), reference_layers=(".*",))
    four = replace_backend(UNet2DConditionModel(TINY).eval())
    kw = dict(cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    with pytest.raises(ValueError, match="tile_hw cannot be combined with a nine-channel"):
        DenoiseLoop(nine, 1, (16, 24), torch.float32, "cpu", tile_hw=16, **kw)
    with pytest.raises(ValueError, match="reference=True cannot be combined with a nine-channel"):
        DenoiseLoop(nine, 1, 16, torch.float32, "cpu", reference=True, **kw)
    loop = DenoiseLoop(four, 1, 16, torch.float32, "cpu", **kw)
    with pytest.raises(ValueError, match="conv_in takes 4 input channels"):
        loop.set_inpaint_condition(torch.ones(16, 16), torch.zeros(1, 4, 16, 16))
    loop9 = DenoiseLoop(nine, 2, 16, torch.float32, "cpu", guidance_scale=5.0, **kw)
    assert tuple(loop9.x_in.shape) == (4, 4, 16, 16) and tuple(nine.inpaint_cond.cond_for(4).shape) == (2, 5, 16, 16)
    with pytest.raises(RuntimeError, match="set_inpaint_condition"):
        loop9.run_steps(1)
