"""HyperTile's host side (stabletriton_amd/hypertile.py, optimizers/insert_hypertile.py): the divisor draw, the drops, table
validation, the pass's site selection and the refused flag combinations.  No GPU."""
import pytest
import torch
from torch import fx

from stabletriton_amd import hypertile as ht
from stabletriton_amd.optimization import check_feature_combination, replace_backend
from stabletriton_amd.unet import TINY, UNet2DConditionModel


@pytest.mark.parametrize("g,swap,want", [(64, 1, [32]), (64, 2, [32, 64]), (64, 3, [32, 64]), (96, 1, [32]), (96, 2, [32, 48]), (96, 3, [32, 48, 96]),
                                         (128, 1, [32]), (128, 2, [32, 64]), (128, 3, [32, 64, 128]), (24, 2, [24])])
def test_candidates(g, swap, want):
    assert ht.candidates(g, 32, swap) == want


def test_dropped_candidates():
    assert ht.site_sides((64, 64), 256, 32, 2) == ([32, 64], [32, 64])
    assert ht.site_sides((32, 32), 128, 16, 1) == ([16], [16])
    assert ht.site_sides((48, 48), 96, 12, 3) == ([24], [16, 24])                      # width 12: no multiple of 8; heights 12, 16: 16 x 16 is no multiple of 96 rows
    assert ht.site_sides((32, 32), 256, 8, 3) == ([16, 32], [16, 32])                  # 8 x 8 ... 8 x 32 windows: no multiple of 256 rows
    assert ht.site_sides((36, 24), 96, 12, 2) is None                                  # width 12, then heights 12 and 18 (18 x 24 rows) go: the whole grid is left
    for grid, rows in (((32, 32), 128), ((32, 12), 96), ((8, 16), 128), ((20, 20), None), ((30, 32), 128)):
        assert ht.site_sides(grid, rows, 32, 2) is None, f"{grid}: ordinary attention"     # whole grid only / width % 8 / T < 256 / no form / 128 does not divide 960


def test_draw_is_seeded_and_gated():
    sides = ([16, 32], [16, 32])
    a = ht.draw_table((32, 32), sides, 20, seed=3, site=1)
    assert a == ht.draw_table((32, 32), sides, 20, seed=3, site=1)
    assert a != ht.draw_table((32, 32), sides, 20, seed=4, site=1) and a != ht.draw_table((32, 32), sides, 20, seed=3, site=2)
    assert set(a) <= {(1, 1), (1, 2), (2, 1), (2, 2)} and len(set(a)) > 1
    half = ht.draw_table((32, 32), ([16], [16]), 10, 0, 0, start=0.2, end=0.5)
    assert half == [(1, 1)] * 2 + [(2, 2)] * 3 + [(1, 1)] * 5
    assert ht.draw_table((32, 32), None, 3, 0, 0) == [(1, 1)] * 3
    with pytest.raises(ValueError, match="start"):
        ht.draw_table((32, 32), sides, 10, 0, 0, start=0.6, end=0.5)


@pytest.mark.parametrize("tiling,rows,word", [((3, 1), None, "does not divide"), ((1, 0), None, "does not divide"), ((True, 1), None, "does not divide"),
                                              ((1, 8), 128, "multiples of 8"), ((4, 4), 128, "query rows per block"), ((2, 2), 96, "query rows per block")])
def test_table_validation(tiling, rows, word):
    with pytest.raises(ValueError, match=word):
        ht.check_tiling((32, 32), tiling, rows)
    assert ht.check_tiling((32, 32), (2, 2), 256) == (2, 2)


def _traced():
    with torch.device("meta"):
        return fx.symbolic_trace(UNet2DConditionModel(TINY).eval())


def test_pass_selects_sites_and_refuses_combinations():
    gm = replace_backend(_traced(), hypertile_layers=("down_blocks.1",))
    assert gm.rewrite_stats["hypertile_sites"] == len(gm.hypertile.sites) == 2 and all("down_blocks.1" in s for s in gm.hypertile.sites)
    every = replace_backend(_traced(), hypertile_layers=(".*",))
    assert every.rewrite_stats["hypertile_sites"] == 17
    with pytest.raises(ValueError, match="hypertile_layers"):
        replace_backend(_traced(), hypertile_layers=("nowhere",))
    for other in ("pag_layers", "seg_layers", "reference_layers"):
        with pytest.raises(ValueError, match="hypertile_layers cannot be combined"):
            check_feature_combination(False, None, None, *((("mid",) if n == other else None) for n in ("pag_layers", "seg_layers")), False,
                                      reference_layers=("mid",) if other == "reference_layers" else None, hypertile_layers=(".*",))
    state = gm.hypertile
    with pytest.raises(ValueError, match="n_steps"):
        state.bind(0)
    with pytest.raises(ValueError, match="swap"):
        state.set(32, 0)
