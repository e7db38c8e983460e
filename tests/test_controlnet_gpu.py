"""ControlNet on the GPU: the grouped residual launch alone in guarded buffers against float64 and against the single-site entry
point, then the compiled TINY networks against the EAGER float64 module with the residuals of the eager float64 branch
(tests/controlnet_util.py) - never the compiled module.

Bounds.  Kernel: DESIGN 4g's - one rounding to the type plus 2 * 2^-24 (|x| + |s r|) for the fp32 fma; every partial within
stat_rows * 2^-24 * sum|y| (sum y^2) of the float64 sums of the STORED values.  Networks: fp32 the project's strict 1e-3; bf16 / fp16
the TINY step gates 0.1 / 0.025 times max|ref with residuals| / max|ref plain| where the residuals enlarge the output, as the
T2I-Adapter tests take them for the same comparison.  The compiled branch's own outputs: fp32 the absolute 1e-3, bf16 / fp16 the
same gates times max(1, max|residual| / max|plain UNet output|), the same rule for a tensor larger than the one the gates were set
for."""
import math

import pytest
import torch

from stabletriton_amd import _C, controlnet as CN, ops, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.unet import TINY, TINY_REFINER, UNet2DConditionModel
from tests import controlnet_util as CU
from tests import freeu_util as FU
from tests.util import rounded

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
GATES = {torch.float32: ABS_TOL_STRICT, torch.bfloat16: 0.1, torch.float16: 0.025}
ULP = 2.0 ** -24
ROUND = {torch.float32: (2.0 ** -23, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -10, 2.0 ** -24)}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (rows, C, H, W), the batch B of the row blocks, rows per statistics tile (a divisor of H * W, as a producer's tiles are)
SHAPES = [((1, 32, 4, 4), 1, 16), ((3, 320, 32, 32), 1, 256), ((2, 1280, 8, 8), 1, 64), ((2, 64, 38, 26), 1, 76), ((6, 64, 6, 6), 2, 12)]
TABLE = [0.0, 1.25, -0.7]          # the scale is read at a non-zero step index; entry 0 is "off"
SITE_COUNTS = [1, 3, 10, 16]


# ------------------------------------------------------------------------------------------------ the kernel alone
def _guarded(shape, dtype, dev, fill):
    """A channels_last tensor inside a larger buffer whose margins hold `fill`: a write out of bounds shows in the margins."""
    n = math.prod(shape)
    pad = 64
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    b, c, h, w = shape
    t = buf[pad:pad + n].view(b, h, w, c).permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=torch.channels_last)
    return t, buf, pad


def _margins_intact(buf, pad):
    return bool(torch.all(buf[:pad] == buf[0]) and torch.all(buf[-pad:] == buf[0]))


def _plan(n_sites):
    """Site k of a set: the shapes in turn (a set of one: the ragged one), r_rows 1 / B / rows in turn, every third site without
    partials; the weights are distinct, one of them an exact 0 (sets of three and more)."""
    plan = []
    for k in range(n_sites):
        shape, batch, srows = SHAPES[(k + 3) % len(SHAPES)] if n_sites == 1 else SHAPES[k % len(SHAPES)]
        r_rows = sorted({1, batch, shape[0]})[(k // len(SHAPES) + k) % len({1, batch, shape[0]})]
        plan.append((shape, srows, r_rows, k % 3 != 2))
    weights = [0.5 + 0.125 * k for k in range(n_sites)]
    if n_sites >= 3:
        weights[1] = 0.0
    return plan, weights


class _Sites:
    """The device buffers of one site set, freshly filled: x and the partials in guarded buffers."""

    def __init__(self, plan, dtype, dev):
        self.plan, self.x0, self.r0, self.x, self.r, self.stats, self.guards, self.before = plan, [], [], [], [], [], [], []
        for k, (shape, srows, r_rows, with_stats) in enumerate(plan):
            rows, C, H, W = shape
            x0 = synth.normal(f"cn.x.{k}", shape, 11 + k).to(dtype)
            r0 = (synth.normal(f"cn.r.{k}", (r_rows,) + shape[1:], 12 + k) * 0.8).to(dtype)
            x, xbuf, xpad = _guarded(shape, dtype, dev, 77.0)
            x.copy_(x0.to(dev))
            st = None
            if with_stats:
                tiles, pad = rows * H * W // srows, 64
                sbuf = torch.full((tiles * C * 2 + 2 * pad,), -5.5, dtype=torch.float32, device=dev)
                view = sbuf[pad:pad + tiles * C * 2].view(tiles, C, 2)
                view.copy_(synth.normal(f"cn.stats.{k}", (tiles, C, 2), 3).to(dev))       # "the producer's" values
                st = ops.ColStats(view, srows, C)
                self.guards.append((sbuf, pad))
            self.guards.append((xbuf, xpad))
            self.x0.append(x0); self.r0.append(r0); self.x.append(x); self.stats.append(st)
            self.r.append(r0.to(dev).contiguous(memory_format=torch.channels_last))
            self.before.append(None if st is None else st.buf.clone().cpu())

    def read(self):
        torch.cuda.synchronize()
        assert all(_margins_intact(b, p) for b, p in self.guards), "a write outside a site's buffers"
        return [x.cpu() for x in self.x], [None if s is None else s.buf.cpu() for s in self.stats]


def _grouped(gpu, dtype, n_sites, step, weights="plan"):
    plan, w = _plan(n_sites)
    s = _Sites(plan, dtype, gpu)
    table = torch.tensor(TABLE, dtype=torch.float32, device=gpu)
    wt = None if weights is None else torch.tensor(w, dtype=torch.float32, device=gpu)
    versions = [x._version for x in s.x]
    ret = ops.residual_add_grouped(s.x, s.r, table, torch.tensor([step], dtype=torch.int32, device=gpu), s.stats, wt)
    assert versions == [x._version for x in s.x], "the launch writes through the raw pointers"
    assert all((a is b) for a, b in zip(ret, s.stats)), "a site hands on the statistics it was given, or None"
    xs, stats = s.read()
    return s, ([1.0] * n_sites if weights is None else w), xs, stats


def _site_scale(step, w):
    """s_k as the kernel forms it: one fp32 product."""
    return float(torch.tensor(TABLE[step], dtype=torch.float32) * torch.tensor(w, dtype=torch.float32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_sites", SITE_COUNTS)
def test_grouped_kernel_vs_float64_and_vs_the_single_site_entry(gpu, dtype, n_sites):
    rel, absr = ROUND[dtype]
    for step in (1, 2):
        s, w, xs, stats = _grouped(gpu, dtype, n_sites, step)
        one = _Sites(s.plan, dtype, gpu)                      # (b) the same sites one by one through st_residual_add at table entry s_k
        zero = torch.zeros(1, dtype=torch.int32, device=gpu)
        for k in range(n_sites):
            ops.residual_add(one.x[k], one.r[k], torch.tensor([_site_scale(step, w[k])], dtype=torch.float32, device=gpu), zero, one.stats[k])
        xs1, stats1 = one.read()
        for k, (shape, srows, r_rows, with_stats) in enumerate(s.plan):
            rows, C, H, W = shape
            sk = _site_scale(step, w[k])
            assert torch.equal(xs[k], xs1[k]) and (not with_stats or torch.equal(stats[k], stats1[k])), f"site {k}: grouped != single-site bits"
            if sk == 0.0:                                     # (c) an exact 0 weight: the producer's bits, the neighbours change
                assert torch.equal(xs[k], s.x0[k]) and (not with_stats or torch.equal(stats[k], s.before[k]))
                continue
            assert not torch.equal(xs[k], s.x0[k]) and (not with_stats or not torch.equal(stats[k], s.before[k]))
            rx = s.r0[k].double().repeat(rows // r_rows, 1, 1, 1)             # row n reads r[n % r_rows]
            want = s.x0[k].double() + sk * rx
            err = (xs[k].double() - want).abs()
            bound = rel * want.abs() + absr + 2 * ULP * (s.x0[k].double().abs() + abs(sk) * rx.abs())
            worst = float((err / bound.clamp_min(1e-300)).max())
            line = f"{dtype} set of {n_sites} site {k} {shape} r_rows={r_rows} s_k={sk}: {worst:.2f} of the element bound"
            assert bool((err <= bound).all()), line
            if with_stats:
                yt = xs[k].double().permute(0, 2, 3, 1).reshape(rows * H * W // srows, srows, C)
                for j, v in ((0, yt), (1, yt * yt)):
                    e = (stats[k][:, :, j].double() - v.sum(1)).abs()
                    b = srows * ULP * v.abs().sum(1)
                    line += f", {float((e / b.clamp_min(1e-300)).max()):.3f} of the partial bound ({('sum', 'squares')[j]})"
                    assert bool((e <= b).all()), line
            print(line)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_sites", SITE_COUNTS)
def test_grouped_kernel_off_writes_nothing_and_two_launches_agree(gpu, dtype, n_sites):
    s, _, xs, stats = _grouped(gpu, dtype, n_sites, 0)
    assert all(torch.equal(a, b) for a, b in zip(xs, s.x0)), "table entry 0: no x is written"
    assert all(a is None or torch.equal(a, b) for a, b in zip(stats, s.before)), "table entry 0: no statistics are written"
    a = _grouped(gpu, dtype, n_sites, 2)
    b = _grouped(gpu, dtype, n_sites, 2)
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2])), "two launches give the same bits"
    assert all(p is None or torch.equal(p, q) for p, q in zip(a[3], b[3]))
    # weights None is weights of ones, and a step past the table reads its last entry
    c = _grouped(gpu, dtype, n_sites, 7, weights=None)
    one = _Sites(c[0].plan, dtype, gpu)
    ops.residual_add_grouped(one.x, one.r, torch.tensor(TABLE, device=gpu), torch.tensor([2], dtype=torch.int32, device=gpu), one.stats,
                             torch.ones(n_sites, device=gpu))
    xs1, stats1 = one.read()
    assert all(torch.equal(p, q) for p, q in zip(c[2], xs1)) and all(p is None or torch.equal(p, q) for p, q in zip(c[3], stats1))


def test_grouped_launcher_rejections_and_torch_route(gpu):
    cl = torch.channels_last
    table = torch.tensor(TABLE, device=gpu)
    step = torch.tensor([1], dtype=torch.int32, device=gpu)
    mk = lambda *shape, dtype=torch.float32: torch.zeros(*shape, device=gpu, dtype=dtype).contiguous(memory_format=cl)
    x, r = mk(2, 64, 4, 4), mk(1, 64, 4, 4).fill_(1.0)
    for n in (0, 17):                                             # (e) before any launch
        with pytest.raises(ops.BackendError, match="1..16 sites"):
            ops.residual_add_grouped([x] * n, [r] * n, table, step)
    with pytest.raises(ops.BackendError, match="one dtype"):
        ops.residual_add_grouped([x, mk(2, 64, 4, 4, dtype=torch.bfloat16)], [r, mk(1, 64, 4, 4, dtype=torch.bfloat16)], table, step)
    with pytest.raises(ops.BackendError, match="one per site"):
        ops.residual_add_grouped([x], [r], table, step, None, torch.ones(2, device=gpu))
    # overlapping byte ranges among the sites of one call: the same x twice, an r that is another site's x, shared statistics
    y = mk(2, 64, 4, 4)
    with pytest.raises(ops.BackendError, match="x of site 0 and x of site 1 overlap"):
        ops.residual_add_grouped([x, x], [r, mk(1, 64, 4, 4)], table, step)
    with pytest.raises(ops.BackendError, match="x of site 0 and r of site 1 overlap"):
        ops.residual_add_grouped([x, y], [r, x[:1]], table, step)
    st = ops.ColStats(torch.zeros(2, 64, 2, device=gpu), 16, 64)
    with pytest.raises(ops.BackendError, match="stats of site 0 and stats of site 1 overlap"):
        ops.residual_add_grouped([x, y], [r, mk(1, 64, 4, 4)], table, step, [st, st])
    # a rejected call has written nothing, a site on torch's route included: it runs only after the entry point took the launch
    routed = mk(2, 34, 4, 4)                                      # fp32: 34 channels are no whole number of 4-element vectors
    with pytest.raises(ops.BackendError, match="x of site 0 and x of site 1 overlap"):      # (sites of the LAUNCH: the routed one is not among them)
        ops.residual_add_grouped([routed, x, x], [mk(1, 34, 4, 4).fill_(1.0), r, mk(1, 64, 4, 4)], table, step)
    assert float(routed.abs().max()) == 0.0 and float(x.abs().max()) == 0.0
    lib = _C.load()                                               # the C entry's own count and dtype checks
    arr = (_C.ResidualSite * 17)(*[_C.ResidualSite(x.data_ptr(), r.data_ptr(), None, 2, 1, 16, 64, 0, 0)] * 17)
    call = lambda n, dt: lib.st_residual_add_grouped(arr, n, None, table.data_ptr(), 3, step.data_ptr(), dt, None)
    assert call(0, _C.ST_F32) != 0 and b"0 sites" in lib.st_last_error()
    assert call(17, _C.ST_F32) != 0 and b"17 sites" in lib.st_last_error()
    assert call(1, 9) != 0 and b"unsupported dtype" in lib.st_last_error()
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0 and float(y.abs().max()) == 0.0, "nothing was launched"
    # a site the kernel does not take (36 channels: no whole vector) goes through torch on its own, the others in the launch
    xs = [synth.normal(f"cn.fb.{k}", s, k).to(gpu, torch.bfloat16).contiguous(memory_format=cl) for k, s in enumerate([(2, 64, 4, 4), (2, 36, 4, 4), (2, 32, 4, 4)])]
    rs = [synth.normal(f"cn.fb.r.{k}", (1,) + tuple(t.shape[1:]), 5 + k).to(gpu, torch.bfloat16).contiguous(memory_format=cl) for k, t in enumerate(xs)]
    w = torch.tensor([0.5, 2.0, 0.25], device=gpu)
    x0 = [t.clone(memory_format=torch.preserve_format) for t in xs]
    sts = [ops.ColStats(torch.zeros(2, t.shape[1], 2, device=gpu), 16, t.shape[1]) for t in xs]
    ret = ops.residual_add_grouped(xs, rs, table, step, sts, w)
    assert ret[0] is sts[0] and ret[1] is None and ret[2] is sts[2]
    for k in range(3):
        sk = float(torch.tensor(1.25) * w[k].cpu())
        want = x0[k].double() + sk * rs[k].double()
        assert float((xs[k].double() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())
    single = x0[2].clone(memory_format=torch.preserve_format)
    ops.residual_add(single, rs[2], torch.tensor([float(torch.tensor(1.25) * w[2].cpu())], device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu))
    assert torch.equal(xs[2], single), "the launch's third site read ITS weight, not the torch-routed site's"


def test_grouped_launch_drops_the_split_note_of_every_site(gpu):
    ys = []
    for k in range(3):
        x = synth.normal(f"cn.split.{k}", (1, 64, 8, 8), k).to(gpu).contiguous(memory_format=torch.channels_last)
        ys.append(ops.group_norm(x, 32, torch.ones(64, device=gpu), torch.zeros(64, device=gpu), 1e-5, True))      # fp32 NHWC: notes its split image
    assert all(any(ent[1] == y.data_ptr() for ent in ops._split_notes(gpu)) for y in ys[-1:]), "this check needs a producer's note"
    rs = [synth.normal(f"cn.split.r.{k}", (1, 64, 8, 8), 9 + k).to(gpu).contiguous(memory_format=torch.channels_last) for k in range(3)]
    ops.residual_add_grouped(ys, rs, torch.tensor([1.0], device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu))
    assert not any(ent[1] == y.data_ptr() for ent in ops._split_notes(gpu) for y in ys)


# ------------------------------------------------------------------------------------------------ TINY networks, one step
def _unet(spec, dtype, dev):
    m = UNet2DConditionModel(spec).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


def _inputs(spec, rows, hw):
    x = synth.denoise_inputs(rows, hw, 1234, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    if spec.n_time_ids != x["time_ids"].shape[1]:
        x["time_ids"] = x["time_ids"][:, :spec.n_time_ids]
    return x


def _args(x, dev=None, dtype=None):
    mv = (lambda v: v.to(dev, dtype)) if dev is not None else (lambda v: v)
    return mv(x["latent"]), torch.tensor(500.0, device=dev), mv(x["encoder_hidden_states"]), {"text_embeds": mv(x["text_embeds"]), "time_ids": mv(x["time_ids"])}


def _copy64(cls, spec, model):
    m64 = cls(spec).eval().requires_grad_(False).double()
    m64.load_state_dict({k: v.detach().double().cpu() for k, v in model.state_dict().items()})
    return m64


def _ref64(spec, model, net, x, image, dtype, scale, freeu=None):
    """float64 on the CPU, on the weights, inputs and control image the kernels see: (plain, controlled at `scale`, the branch's
    float64 residuals)."""
    m64, n64 = _copy64(UNet2DConditionModel, spec, model), _copy64(CN.ControlNetXL, spec, net)
    xi = {k: rounded(v, dtype).double() for k, v in x.items()}
    cond = n64.embed_condition(rounded(image, dtype).double())
    res = CU.branch_residuals(n64, *_args(xi), cond)
    with torch.no_grad():
        plain = m64(*_args(xi))[0]
        if freeu is None:
            return plain, CU.controlled(m64, *_args(xi), res, scale)[0], res
        with FU.hooked(m64, **freeu):
            return plain, CU.controlled(m64, *_args(xi), res, scale)[0], res


def _gate(dtype, ref, plain):
    return GATES[dtype] if dtype == torch.float32 else GATES[dtype] * max(1.0, float(ref.abs().max() / plain.abs().max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tiny_sites_at_scale_zero_are_the_module_without_sites(gpu, dtype):
    model = _unet(TINY, dtype, gpu)
    plain = optimize_model(model, cuda_graph=False)
    gm = optimize_model(model, cuda_graph=False, controlnet=True)
    assert gm.rewrite_stats["controlnet_sites"] == 10
    assert {k: v for k, v in gm.rewrite_stats.items() if k != "controlnet_sites"} == dict(plain.rewrite_stats)
    x = _inputs(TINY, 2, 16)
    step = lambda m: m(*_args(x, gpu, dtype))[0]
    with torch.no_grad():
        gm.controlnet.bind(2, 16, gpu)
        want = step(plain)
        assert torch.equal(step(gm), want), "after bind"
        gm.controlnet.set([r.to(gpu) for r in CU.residuals(TINY, 16, rows=2)], 0.0)
        assert torch.equal(step(gm), want), "residuals set, scale 0"
        gm.controlnet.set_scale(0.7)
        assert not torch.equal(step(gm), want)
        gm.controlnet.set_site_weights([0.0] * 10)
        assert torch.equal(step(gm), want), "every site at weight 0"
        gm.controlnet.set_site_weights(None)
        gm.controlnet.clear()
        assert torch.equal(step(gm), want), "after clear"


@pytest.mark.parametrize("spec,hw,dtype", [(TINY, hw, dt) for hw in (16, (24, 16)) for dt in (torch.float32, torch.bfloat16, torch.float16)]
                         + [(TINY_REFINER, 16, torch.float32)])
def test_tiny_step_and_compiled_branch_vs_the_float64_eager_modules(gpu, dtype, spec, hw):
    model, net = _unet(spec, dtype, gpu), CU.branch(spec).to(gpu, dtype)
    gm = optimize_model(model, cuda_graph=False, controlnet=True)
    branch = optimize_model(net, cuda_graph=False)
    n = gm.rewrite_stats["controlnet_sites"]
    x, image = _inputs(spec, 2, hw), CU.control_image(2, hw)
    plain, ref, res64 = _ref64(spec, model, net, x, image, dtype, 0.7)
    moved = float((ref - plain).abs().max())
    gate = _gate(dtype, ref, plain)
    assert moved > 10 * gate, "the residuals must matter for this check to mean anything"
    with torch.no_grad():
        cond = branch.embed_condition(image.to(gpu, dtype))
        down, mid = branch(*_args(x, gpu, dtype), cond_embed=cond)
        res = list(down) + [mid]
        assert len(res) == n
        # the compiled branch alone against its eager float64 self, under the same gates: fp32 the absolute 1e-3; bf16 / fp16 the TINY
        # step gates by the T2I tests' scaling rule - they were set for a tensor of the plain UNet output's size, and a residual
        # whose maximum is k times that carries k times the rounding of a 16-bit type
        ratios = []
        for k, (a, b) in enumerate(zip(res, res64)):
            g = GATES[dtype] if dtype == torch.float32 else GATES[dtype] * max(1.0, float(b.abs().max() / plain.abs().max()))
            ratios.append(float((a.double().cpu() - b).abs().max()) / g)
        worst = max(ratios)
        assert worst <= 1.0, f"branch residuals against their gates: {[round(r, 3) for r in ratios]}"
        gm.controlnet.bind(2, hw, gpu)
        table, step = torch.tensor([0.0, 0.7], device=gpu), torch.tensor([1], dtype=torch.int32, device=gpu)
        with gm.controlnet.using(step, table, residuals=res):
            out = gm(*_args(x, gpu, dtype))[0]
        lent = float((out.double().cpu() - ref).abs().max())
        gm.controlnet.set(res, 0.7)                            # the same through the state's own buffers and scale: the same bits
        assert torch.equal(gm(*_args(x, gpu, dtype))[0], out)
    print(f"{spec.widths} {dtype} latent {hw} ControlNet at 0.7: max abs err vs float64 {lent:.2e} (gate {gate:.2e}; {lent / gate:.3f} of it; "
          f"|ref| max {float(ref.abs().max()):.2f}; the residuals move the output by {moved:.2f}); compiled branch worst {worst:.2e} "
          f"of its gate")
    assert lent <= gate


def test_tiny_step_with_freeu_compiled_in(gpu):
    """FreeU's sites read the leaf's outputs: skip tensors and a backbone that carry the residuals."""
    dtype = torch.float32
    model, net = _unet(TINY, dtype, gpu), CU.branch(TINY).to(gpu, dtype)
    gm = optimize_model(model, cuda_graph=False, controlnet=True, freeu=True)
    assert gm.rewrite_stats["controlnet_sites"] == 10 and gm.rewrite_stats["freeu_sites"] == 6 and gm.rewrite_stats["skip_cats_removed"] == 9
    x, image = _inputs(TINY, 2, 16), CU.control_image(2, 16)
    plain, ref, res64 = _ref64(TINY, model, net, x, image, dtype, 0.7, freeu=dict(FU.SDXL_VALUES, version=1))
    assert float((ref - plain).abs().max()) > 10 * ABS_TOL_STRICT
    gm.controlnet.bind(2, 16, gpu)
    gm.controlnet.set([r.to(gpu, dtype) for r in res64], 0.7)
    gm.freeu.set(**FU.SDXL_VALUES, version=1)
    with torch.no_grad():
        err = float((gm(*_args(x, gpu, dtype))[0].double().cpu() - ref).abs().max())
    print(f"tiny fp32 ControlNet at 0.7 + FreeU: max abs err vs the float64 eager module with both {err:.2e}")
    assert err <= ABS_TOL_STRICT


def test_strict_split_notes_are_dropped_for_every_site(gpu):
    """fp32: after a step the notes of the context hold no image of any tensor the leaf wrote (the decoder's readers split their
    own operands)."""
    dtype = torch.float32
    gm = optimize_model(_unet(TINY, dtype, gpu), cuda_graph=False, controlnet=True)
    gm.controlnet.bind(2, 16, gpu)
    res = [r.to(gpu) for r in CU.residuals(TINY, 16, rows=2)]
    gm.controlnet.set(res, 0.7)
    seen, launched = [], []
    inner = ops.residual_add_grouped
    lib = _C.load()
    entry = lib.st_residual_add_grouped

    def spy(xs, *a, **kw):
        out = inner(xs, *a, **kw)
        ptrs = {x.data_ptr() for x in xs}
        seen.append((len(xs), [ent for ent in ops._split_notes(xs[0].device) if ent[1] in ptrs]))
        return out

    def counted(sites, n_sites, *a):                             # what reaches the HIP entry point: a site on torch's route would be missing
        launched.append(n_sites)
        return entry(sites, n_sites, *a)

    ops.residual_add_grouped = spy
    lib.st_residual_add_grouped = counted
    try:
        with torch.no_grad():
            gm(*_args(_inputs(TINY, 2, 16), gpu, dtype))
    finally:
        ops.residual_add_grouped = inner
        lib.st_residual_add_grouped = entry
    assert launched == [10], "all ten sites went into the one HIP launch, none through torch"
    assert seen == [(10, [])], "one grouped launch of ten sites, and no note left for any of them"


def test_unbound_and_mismatched_buffers_say_what_to_do(gpu):
    gm = optimize_model(_unet(TINY, torch.bfloat16, gpu), cuda_graph=False, controlnet=True)
    x = _inputs(TINY, 2, 16)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"controlnet.bind\(rows, latent_hw, device\)"):
            gm(*_args(x, gpu, torch.bfloat16))
        gm.controlnet.bind(2, 16, gpu, dtype=torch.float32)
        with pytest.raises(ValueError, match="the activation is torch.bfloat16"):
            gm(*_args(x, gpu, torch.bfloat16))
    for other in (dict(fp8=True), dict(t2i_adapter=True)):
        with pytest.raises(ValueError, match="controlnet=True cannot be combined"):
            optimize_model(_unet(TINY, torch.bfloat16, gpu), cuda_graph=False, controlnet=True, **other)
