"""Reference-only control on the host: the fx pass's site selection and flag conflicts, a traced CPU TINY module carrying the pass
against the independent hooked eager route (tests/reference_util.py), the loop's row blocks, buffers and gate table on CPU tensors,
and the C entry point's presence.  No GPU."""
import pytest
import torch
from torch import fx

from stabletriton_amd import reference, synth
from stabletriton_amd.optimization import check_feature_combination, replace_backend
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel, UNetWithLabelVector
from tests import reference_util as RU


def _meta(spec, wrap=False):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec).eval()
        return UNetWithLabelVector(m) if wrap else m


def _ref_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target is reference.attention_reference_wrapper]


# ------------------------------------------------------------------------------------------------ 1. the pass
# TINY: mid_block 2 layers; down_blocks.1 two blocks of 1, down_blocks.2 two of 2; up_blocks.0 three of 2, up_blocks.1 three of 1
@pytest.mark.parametrize("spec,layers,want", [
    (TINY, (".*",), 17), (TINY, ("mid",), 2), (TINY, ("up_blocks",), 9), (TINY, ("down_blocks.2", "mid"), 6), (TINY, ".*", 17),
    (SDXL_BASE, (".*",), 70)])
def test_site_counts(spec, layers, want):
    gm = replace_backend(fx.symbolic_trace(_meta(spec)), reference_layers=layers)
    assert gm.rewrite_stats["reference_sites"] == want and len(_ref_nodes(gm)) == want
    assert isinstance(gm.reference, reference.ReferenceRows) and gm.reference.chunks == 0 and len(gm.reference.sites) == want
    assert all(s.endswith(".attn1") for s in gm.reference.sites)


def test_prefix_in_front_of_the_block_names_does_not_matter():
    gm = replace_backend(fx.symbolic_trace(_meta(TINY, wrap=True)), reference_layers=("mid",))
    assert gm.rewrite_stats["reference_sites"] == 2


@pytest.mark.parametrize("layers", [("nowhere",), (".*", "nowhere"), ("attn2",), (), ("",)])
def test_patterns_that_select_no_self_attention_raise(layers):
    with pytest.raises(ValueError, match="reference_layers"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), reference_layers=layers)


class _Untraceable(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("the flags are checked before the trace")


@pytest.mark.parametrize("kw", [dict(pag_layers=("mid",)), dict(seg_layers=("mid",))])
def test_flag_conflicts_raise_before_the_trace(kw):
    with pytest.raises(ValueError, match="reference_layers cannot be combined"):
        replace_backend(_Untraceable(), reference_layers=(".*",), **kw)
    with pytest.raises(ValueError, match="reference_layers cannot be combined"):
        check_feature_combination(False, None, None, kw.get("pag_layers"), kw.get("seg_layers"), False, False, (".*",))
    check_feature_combination(False, None, None, None, None, False)          # the trailing argument is defaulted
    check_feature_combination(False, None, None, ("mid",), None, False, False)


def test_default_graph_is_unchanged_and_other_passes_still_fire():
    a = replace_backend(fx.symbolic_trace(_meta(TINY)))
    b = replace_backend(fx.symbolic_trace(_meta(TINY)), reference_layers=None)
    assert a.code == b.code and "reference" not in a.code and not hasattr(a, "reference")
    on = replace_backend(fx.symbolic_trace(_meta(TINY)), reference_layers=(".*",))
    assert {k: v for k, v in on.rewrite_stats.items() if k != "reference_sites"} == dict(a.rewrite_stats)
    from stabletriton_amd.optimizers.wrappers import ln_linear_wrapper
    for n in _ref_nodes(on):      # q, k and v: slices of ONE fused, LayerNorm-folded q|k|v projection, as every other self-attention
        srcs = {arg.args[0] for arg in n.args[:3]}
        assert len(srcs) == 1
        prod = srcs.pop()
        assert prod.target is ln_linear_wrapper and len(prod.args[3]) == 3


def test_fp8_plan_is_what_it_is_without_the_pass():
    a = replace_backend(fx.symbolic_trace(_meta(TINY).to(torch.bfloat16)), fp8=True)
    on = replace_backend(fx.symbolic_trace(_meta(TINY).to(torch.bfloat16)), fp8=True, reference_layers=(".*",))
    assert {k: v for k, v in on.rewrite_stats.items() if k != "reference_sites"} == dict(a.rewrite_stats)


# ------------------------------------------------------------------------------------------------ 2. TINY on the CPU
def _tiny():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def _call(mod, x):
    with torch.no_grad():
        return mod(x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]


def _traced_with_only_the_pass(m, layers):
    """fuse_attention + insert_reference on a traced module; the unselected attention_wrapper leaves (no CPU route) get eager ones."""
    from stabletriton_amd.optimizers import fuse_attention, insert_reference
    from stabletriton_amd.optimizers.wrappers import attention_wrapper
    from stabletriton_amd.pag import identity_attention_reference
    gm = fx.symbolic_trace(m)
    n_att = fuse_attention(gm)
    sites = insert_reference(gm, layers)
    for n in list(gm.graph.nodes):
        if n.op == "call_function" and n.target is attention_wrapper:
            with gm.graph.inserting_before(n):
                new = gm.graph.call_function(identity_attention_reference, (n.args[0], n.args[1], n.args[2], n.args[5], n.args[4], 0))
            n.replace_all_uses_with(new)
            gm.graph.erase_node(n)
    gm.recompile()
    return gm, n_att, sites


@pytest.mark.parametrize("layers,want_sites", [((".*",), 17), (("mid", "up_blocks.0"), 8)])
def test_traced_cpu_module_with_the_pass_equals_the_hook_route(layers, want_sites):
    m = _tiny()
    x = synth.denoise_inputs(6, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    plain = _call(m, x)
    gm, n_att, sites = _traced_with_only_the_pass(m, layers)
    assert sites == want_sites and n_att > sites
    bound = 2e-5 * float(plain.abs().max())                 # fp32 rounding: a few 100 ulp of the output's size (tests/test_pag_host.py)
    for chunks in (3, 2):
        with RU.hooked(m, layers, chunks):
            want = _call(m, x)
        with gm.reference.using(chunks):
            got = _call(gm, x)
        assert gm.reference.chunks == 0 and gm.reference.gate is None, "the context manager restores the previous values"
        n = 6 // chunks
        moved = float((want[:6 - n] - plain[:6 - n]).abs().max())
        assert moved > 1e-2, "the reference must matter for this check to mean anything"
        assert torch.equal(want[6 - n:], plain[6 - n:]), "reference rows run ordinary self-attention"
        err = float((got - want).abs().max())
        print(f"chunks {chunks}: traced vs hooked max abs diff {err:.2e}; the reference moves the other rows by {moved:.2e}")
        assert err < bound, f"chunks {chunks}"
        # the device gate on the CPU leaf: off = the untouched module, on = the same as without a gate
        step, table = torch.zeros(1, dtype=torch.int32), torch.tensor([0.0, 1.0])
        with gm.reference.using(chunks, step=step, table=table):
            assert float((_call(gm, x) - plain).abs().max()) < bound
            step.fill_(1)
            assert torch.equal(_call(gm, x), got)
    got0 = _call(gm, x)                                     # chunks 0
    assert float((got0 - plain).abs().max()) < bound
    with gm.reference.using(1):                            # every row a reference row: ordinary attention
        assert torch.equal(_call(gm, x), got0)
    with gm.reference.using(4), pytest.raises(ValueError, match="chunks"):
        _call(gm, x)                                         # 6 % 4 != 0


def test_chunks_zero_leaf_is_the_plain_statement_bit_for_bit():
    st = reference.ReferenceRows()
    q, k, v = (torch.randn(6, 5, 8, generator=torch.Generator().manual_seed(i)) for i in range(3))
    from stabletriton_amd.pag import identity_attention_reference
    plain = identity_attention_reference(q, k, v, 2, 0.5, 0)
    assert torch.equal(reference.attention_reference_wrapper(q, k, v, None, 0.5, 2, 4, st), plain)
    with st.using(3):
        on = reference.attention_reference_wrapper(q, k, v, None, 0.5, 2, 4, st)
    assert torch.equal(on[4:], plain[4:]) and not torch.equal(on[:4], plain[:4])
    # rows 0 and 2 read reference row 4, rows 1 and 3 row 5
    want = reference.joint_attention_reference(q[:4], k[:4], v[:4], k[4:], v[4:], 2, 0.5, 4)
    assert torch.equal(on[:4], want)
    one = reference.joint_attention_reference(q[1:2], k[1:2], v[1:2], k[5:6], v[5:6], 2, 0.5, 1)
    assert float((on[1:2] - one).abs().max()) < 1e-6


def test_state_validation_and_state_of():
    st = reference.ReferenceRows()
    assert st.label == "reference" and st.chunks == 0 and st.reference_count(6) == 0
    for bad in (-1, 1.5, True, None, "3"):
        with pytest.raises(ValueError, match="reference"):
            st.set_chunks(bad)
    with st.using(3) as inside:
        assert inside is st and st.reference_count(6) == 2 and st.gate is None
        step, table = torch.zeros(1, dtype=torch.int32), torch.ones(4)
        with st.using(2, step=step, table=table):
            assert st.chunks == 2 and st.gate[0] is step and st.gate[1] is table
        assert st.chunks == 3 and st.gate is None
    assert st.chunks == 0
    with pytest.raises(ValueError, match="together"):
        with st.using(2, step=torch.zeros(1, dtype=torch.int32)):
            pass
    own = st.own_gate(torch.device("cpu"))
    assert own is st.own_gate(torch.device("cpu")) and int(own[0]) == 0 and own[1].tolist() == [1.0]
    with pytest.raises(ValueError, match="reference_layers"):
        reference.state_of(torch.nn.Linear(2, 2), "enable_reference")


# ------------------------------------------------------------------------------------------------ 3. DenoiseLoop (CPU tensors)
class _NoUNet:
    """Stands in for a compiled UNet: the host-side paths below never evaluate it."""

    def __init__(self, **states):
        self.reference = reference.ReferenceRows()
        for k, v in states.items():
            setattr(self, k, v)


def _loop(unet=None, **kw):
    from stabletriton_amd.pipeline import DenoiseLoop
    from stabletriton_amd.scheduler import euler_discrete_tables
    return DenoiseLoop(unet or _NoUNet(), 2, 16, torch.float32, "cpu", euler_discrete_tables(10), cross_dim=8, pooled_dim=6, tokens=3, **kw)


@pytest.mark.parametrize("guided", [False, True])
def test_loop_rows_conditioning_input_blocks_and_table(guided):
    kw = dict(guidance_scale=5.0) if guided else {}
    lp = _loop(reference=True, mode="step", **kw)
    blocks = 3 if guided else 2
    assert lp.x_in.shape[0] == lp.ehs.shape[0] == lp.text_embeds.shape[0] == lp.time_ids.shape[0] == 2 * blocks
    assert lp._reference_chunks == blocks and lp._lead_rows == 2 * (blocks - 1) and lp.pag is None
    assert torch.equal(lp.reference_table, torch.zeros(10)), "all 0 = off until set_reference"
    assert lp.sigma_next.shape == (10,) and float(lp.sigma_next[-1]) == 0.0
    pos = (torch.randn(2, 3, 8), torch.randn(2, 6), torch.randn(2, 6))
    neg = (torch.randn(2, 3, 8), torch.randn(2, 6), torch.randn(2, 6))
    lp.set_conditioning(*pos, *(neg if guided else ()))
    for buf, p, q in zip((lp.ehs, lp.text_embeds, lp.time_ids), pos, neg):
        assert torch.equal(buf[-2:], p) and torch.equal(buf[-4:-2], p), "the reference block carries the positive conditioning"
        if guided:
            assert torch.equal(buf[:2], q)
    ref, rz, z = torch.randn(1, 4, 16, 16), torch.randn(2, 4, 16, 16), torch.randn(2, 4, 16, 16)
    table = lp.reference_table
    lp.set_reference(ref, rz)
    assert lp.reference_table is table and torch.equal(table, torch.ones(10)), "an in-place write: captured graphs read this table by address"
    lp.set_noise(z)
    s0, sc0 = float(lp.tables.sigmas[0]), float(lp.tables.in_scale()[0])
    for r in range(blocks - 1):
        assert torch.equal(lp.x_in[2 * r:2 * r + 2], (z * lp.tables.init_noise_sigma) * sc0)
    assert torch.equal(lp.x_in[-2:], (ref.expand(2, -1, -1, -1) + rz * s0) * sc0), "the reference block: (init + sigma[0] * noise) * in_scale[0]"
    lp.set_reference(ref, rz, start=0.2, end=0.5)
    assert lp.reference_table.tolist() == [0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    lp.set_reference(ref, rz, start=0.5)
    assert lp.reference_table.tolist() == [0.0] * 5 + [1.0] * 5
    left = lp.set_image(torch.zeros(2, 4, 16, 16), z, 0.5)          # the trajectory starts at step 5
    assert left == 5
    assert torch.equal(lp.x_in[-2:], (ref.expand(2, -1, -1, -1) + rz * float(lp.tables.sigmas[5])) * float(lp.tables.in_scale()[5]))
    lp.set_reference(None)
    assert lp.reference_table is table and torch.equal(table, torch.zeros(10))
    for bad in (dict(start=0.6, end=0.5), dict(start=-0.1), dict(end=1.5)):
        with pytest.raises(ValueError, match="set_reference"):
            lp.set_reference(ref, rz, **bad)
    with pytest.raises(ValueError, match="set_reference"):
        lp.set_reference(torch.randn(3, 4, 16, 16), rz)
    with pytest.raises(ValueError, match="noise or seed"):
        lp.set_reference(ref)
    with pytest.raises(ValueError, match="noise or seed"):
        lp.set_reference(ref, rz, seed=3)


def test_constructor_refusals():
    from stabletriton_amd import controlnet, ip_adapter, pag, regions, seg, t2i_adapter

    class Plain:
        pass

    with pytest.raises(ValueError, match="reference_layers"):
        _loop(Plain(), reference=True)
    with pytest.raises(ValueError, match="reference=True cannot be combined"):
        _loop(_NoUNet(pag=pag.PAG()), reference=True, pag_scale=3.0)
    with pytest.raises(ValueError, match="reference=True cannot be combined"):
        _loop(_NoUNet(seg=seg.SEG()), reference=True, seg_scale=3.0)
    with pytest.raises(ValueError, match="reference=True cannot be combined"):
        _loop(reference=True, tile_hw=8)
    for name, cls in (("regions", regions.Regions), ("ip_adapter", ip_adapter.IPAdapter), ("t2i_adapter", t2i_adapter.T2IAdapterState),
                      ("controlnet", controlnet.ControlNetState)):
        state = cls.__new__(cls)                              # (only its type is looked at, before anything is bound)
        torch.nn.Module.__init__(state)
        with pytest.raises(ValueError, match=f"compiled with {name}"):
            _loop(_NoUNet(**{name: state}), reference=True)
    with pytest.raises(ValueError, match="reference=True"):
        _loop().set_reference(torch.zeros(1, 4, 16, 16), torch.zeros(1, 4, 16, 16))
    plain = _loop(guidance_scale=5.0)                        # without the flag nothing about the loop changes
    assert plain.reference_table is None and plain.x_in.shape[0] == 4 and plain._reference is None and plain.sigma_next is None
    assert plain._x_lead is plain.x_step


# ------------------------------------------------------------------------------------------------ 4. the C entry point
P = 1 << 20            # a fake, aligned, never dereferenced device address: validation happens before any launch


def test_entry_point_exists_and_validates_on_the_host(lib):
    from stabletriton_amd import _C
    assert hasattr(lib, "st_attention_joint") and lib.st_abi_version() == _C.ABI_VERSION == 18

    def joint(**kw):
        a = dict(q=P, k=P, v=P, k2=P, v2=P, out=P, B=3, T=256, S1=256, S2=256, B2=1, lead=2, H=2, D=64, ldq=384, ldk=384, ldv=384, ldk2=384,
                 ldv2=384, bsk2=0, bsv2=0, ldo=128, table=None, step=None, n=0, dtype=_C.ST_BF16)
        a.update(kw)
        return lib.st_attention_joint(a["q"], a["k"], a["v"], a["k2"], a["v2"], a["out"], a["B"], a["T"], a["S1"], a["S2"], a["B2"], a["lead"],
                                      a["H"], a["D"], a["ldq"], a["ldk"], a["ldv"], a["ldk2"], a["ldv2"], a["bsk2"], a["bsv2"], a["ldo"], 0.125,
                                      a["table"], a["step"], a["n"], a["dtype"], None)

    for name in ("q", "k", "v", "k2", "v2", "out"):
        assert joint(**{name: None}) != 0 and b"attention_joint: null" in lib.st_last_error(), name
    assert joint(S1=255) != 0 and b"S1" in lib.st_last_error()
    assert joint(D=32) != 0 and b"head_dim" in lib.st_last_error()
    assert joint(dtype=_C.ST_F32) != 0 and b"16-bit" in lib.st_last_error()
    assert joint(S2=0) != 0 and b"bad shape" in lib.st_last_error()
    assert joint(B2=0) != 0 and b"bad shape" in lib.st_last_error()
    assert joint(lead=4) != 0 and b"lead" in lib.st_last_error()
    assert joint(lead=-1) != 0 and b"lead" in lib.st_last_error()
    assert joint(ldk2=388) != 0 and b"16-byte" in lib.st_last_error()
    assert joint(ldk2=64) != 0 and b"second-source" in lib.st_last_error()
    assert joint(bsv2=-8) != 0 and b"second-source" in lib.st_last_error()
    assert joint(v2=P + 8) != 0 and b"16-byte" in lib.st_last_error()
    assert joint(table=P) != 0 and b"gate" in lib.st_last_error()
    assert joint(table=P, step=P, n=0) != 0 and b"gate table" in lib.st_last_error()
    assert joint(table=P + 2, step=P, n=4) != 0 and b"misaligned" in lib.st_last_error()


def test_ops_entry_on_cpu_tensors_is_the_plain_statement():
    from stabletriton_amd import ops
    q, k, v = (torch.randn(3, 5, 8, generator=torch.Generator().manual_seed(i)) for i in range(3))
    k2, v2 = (torch.randn(1, 4, 8, generator=torch.Generator().manual_seed(9 + i)) for i in range(2))
    want = reference.joint_attention_reference(q, k, v, k2, v2, 2, 0.5, 2)
    assert torch.equal(ops.attention_joint(q, k, v, k2, v2, 2, 0.5, lead=2), want)
    step, table = torch.zeros(1, dtype=torch.int32), torch.tensor([0.0, 1.0])
    off = ops.attention_joint(q, k, v, k2, v2, 2, 0.5, lead=2, gate=(step, table))
    assert torch.equal(off, reference.joint_attention_reference(q, k, v, k2, v2, 2, 0.5, 0))
    step.fill_(9)                                            # clamps to the last entry
    assert torch.equal(ops.attention_joint(q, k, v, k2, v2, 2, 0.5, lead=2, gate=(step, table)), want)
    with pytest.raises(ops.BackendError, match="lead"):
        ops.attention_joint(q, k, v, k2, v2, 2, 0.5, lead=4)
