"""st_conv_stem (csrc/conv_stem.hip; tile th x tw = 8 x 16, weights through LDS 64 channels at a time in groups of 32) per element
against F.conv2d in float64 on the concatenation of the rounded inputs, under the project's budget (tests/edge_util.py) with
n_terms = 9 (C0 + C1) + 1.  Shapes: 5 x 7 (one partial tile, mostly border, half a group); 9 x 33 = (th + 1) x (2 tw + 1) (ragged both
ways, `b` shared, Cout = 48); 16 x 16 (whole tiles, n % Nb, Cout = 320: several stages, every blockIdx.y chunk); one 8-channel source
(K = 72, refused by st_conv2d); one nine-channel tensor (18-byte pixels).  Every case runs in two forms of the same values - separate
tensors, one tensor, channel-slice views of one - which share one K order and must agree bit for bit."""
import pytest
import torch

from stabletriton_amd import ops
from tests import edge_util as E

pytestmark = pytest.mark.gpu

# (N, H, W, Cout, C0, C1, Nb, form, other form)
CASES = [(1, 5, 7, 16, 4, 5, 1, "two", "one"), (2, 9, 33, 48, 4, 5, 1, "two", "one"), (4, 16, 16, 320, 4, 5, 2, "two", "one"),
         (2, 9, 33, 32, 8, 0, 0, "one", "views"), (2, 9, 33, 32, 4, 5, 2, "one", "views")]
LIVE_WEIGHT_CASE = 1


def _sources(form, a, b, full, C0, dev, dtype):
    cl = lambda t: t.to(dev, dtype).contiguous(memory_format=torch.channels_last)
    if form == "two":
        return cl(a), cl(b)
    x = cl(full)
    return (x, None) if form == "one" else (x[:, :4], x[:, 4:])


@pytest.mark.parametrize("dtype", E.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_conv_stem(gpu, case, dtype):
    N, H, W, Cout, C0, C1, Nb, form, other = CASES[case]
    C = C0 + C1
    a = E.normal(f"s.a{case}", (N, C0, H, W))
    b = E.normal(f"s.b{case}", (Nb, C1, H, W)) if C1 else None
    full = a if b is None else torch.cat([a, torch.cat([b] * (N // Nb))], dim=1)      # image n reads b[n % Nb]
    w = E.normal(f"s.w{case}", (Cout, C, 3, 3), (9 * C) ** -0.5)
    bias = E.normal(f"s.bias{case}", (Cout,), 0.5)
    wg, bg = w.to(gpu, dtype).contiguous(memory_format=torch.channels_last), bias.to(gpu, dtype)
    what = f"conv_stem {CASES[case]} {dtype}"

    def run(frm):
        out, buf = E.guarded((N, Cout, H, W), dtype, gpu, channels_last=True)
        ops.conv_stem(*_sources(frm, a, b, full, C0, gpu, dtype), wg, bg, out=out)
        E.assert_margins_intact(buf, f"{what} [{frm}]")
        return out

    out = run(form)
    ref, mag = E.conv_ref64(full, w, bias, dtype, 1, 1, False)
    worst = E.assert_elementwise(out, ref, mag, 9 * C + 1, dtype, what)
    print(f"{what}: worst element at {worst:.3f} of its budget")
    assert torch.equal(run(form), out), f"{what}: a second launch must give the same bits"
    assert torch.equal(run(other), out), f"{what}: the {other!r} form of the same values must give the bits of the {form!r} form"
    if case == LIVE_WEIGHT_CASE:                               # no cached repack: an in-place update is what the next launch reads
        wg.mul_(2)
        ref2, mag2 = E.conv_ref64(full, 2 * w, bias, dtype, 1, 1, False)
        E.assert_elementwise(run(form), ref2, mag2, 9 * C + 1, dtype, what + " after weight.mul_(2)")
