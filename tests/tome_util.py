"""Inputs and C-ABI callers of the token-merging tests.  A site with an unambiguous plan: dst tokens are N(0, 1); src s is
dst[pi(s)] + eps_s * noise, the noise orthogonal to the row's dst tokens and as long as dst[pi(s)]: cos(src s, dst pi(s)) =
1 / sqrt(1 + eps_s^2) is one of S evenly spaced values in [cos_lo, COS_HI] (eps increasing over a shuffled s).  All rounded to the dtype first."""
import functools

import torch

from stabletriton_amd import _C, tome
from tests import edge_util as eu

# GAP: what the tests assert of the float64 reference (best - second best of a row; between sorted node_max)
COS_HI, COS_LO, GAP = 0.999, 0.02, 1e-3      # 768 levels 1.28e-3 apart at the largest site; a site of few src takes a higher floor (unit scale)


@functools.lru_cache(maxsize=None)
def site(grid, C, dtype, rand_off, cos_lo=COS_LO, B=2):
    (h, w), D, S = grid, grid[0] * grid[1] // 4, grid[0] * grid[1] // 4 * 3      # -> (x (B, N, C) in dtype on the CPU, off (1, D) uint8)
    gen = torch.Generator().manual_seed(h * 1000 + w * 10 + C)
    off = tome.draw_offsets(grid, 1, 11 if rand_off else None)
    dst_tok, src_tok = tome.site_tokens(grid, off[0])
    dst = torch.randn((B, D, C), generator=gen, dtype=torch.float64)
    noise = torch.randn((B, S, C), generator=gen, dtype=torch.float64)
    q = torch.linalg.qr(dst.transpose(1, 2)).Q                                     # (B, C, D): the span of the row's dst tokens
    noise = noise - (noise @ q) @ q.transpose(1, 2)
    pi = torch.randint(0, D, (B, S), generator=gen)
    d = torch.gather(dst, 1, pi[..., None].expand(-1, -1, C))
    noise = noise * (d.norm(dim=-1, keepdim=True) / noise.norm(dim=-1, keepdim=True))
    levels = torch.linspace(COS_HI, cos_lo, S, dtype=torch.float64)
    cos = torch.stack([levels[torch.randperm(S, generator=gen)] for _ in range(B)])
    x = torch.empty((B, h * w, C), dtype=torch.float64)
    x[:, dst_tok] = dst
    x[:, src_tok] = d + (1.0 / cos ** 2 - 1.0).sqrt()[..., None] * noise
    return x.to(dtype), off


@functools.lru_cache(maxsize=None)
def match64(grid, C, dtype, rand_off, cos_lo=COS_LO):
    x, off = site(grid, C, dtype, rand_off, cos_lo)
    dst_tok, src_tok = tome.site_tokens(grid, off[0])
    xn = torch.nn.functional.normalize(x.double(), dim=-1)
    top = (xn[:, src_tok] @ xn[:, dst_tok].transpose(1, 2)).topk(2, dim=-1).values
    assert float((top[..., 0] - top[..., 1]).min()) >= GAP, "best and second-best cosine of a row are too close"
    node_max, node_idx = tome.match_reference(x.double(), grid, off[0])
    assert float(node_max.sort(dim=-1).values.diff(dim=-1).min()) >= GAP, "two node_max are too close for an unambiguous rank"
    return node_max, node_idx


def norm_affine(C, dtype):
    g = torch.Generator().manual_seed(C)
    return (1.0 + 0.25 * torch.randn(C, generator=g)).to(dtype), (0.25 * torch.randn(C, generator=g)).to(dtype)


_guard = lambda shape, dtype, dev: eu.guarded(shape, dtype, dev, fill=None if dtype.is_floating_point else -7)


def match_into(x, grid, off):
    B, S = x.shape[0], x.shape[1] // 4 * 3
    (nm, b0), (ni, b1) = _guard((B, S), torch.float32, x.device), _guard((B, S), torch.int32, x.device)
    _C.check(_C.load().st_tome_match(x.data_ptr(), x.stride(1), off.data_ptr(), None, off.shape[0], B, grid[0], grid[1], x.shape[2], nm.data_ptr(),
                                     ni.data_ptr(), _C.dtype_code(x.dtype), _C.stream_ptr()), "tome_match")
    return (nm, ni), (b0, b1)


def select_into(node_max, node_idx, grid, r, off):
    B, S = node_max.shape
    outs = [_guard(s, torch.int32, node_max.device) for s in ((B, grid[0] * grid[1]), (B, S), (B, S))]
    _C.check(_C.load().st_tome_select(node_max.data_ptr(), node_idx.data_ptr(), off.data_ptr(), None, off.shape[0], B, grid[0], grid[1], r,
                                      *(t.data_ptr() for t, _ in outs), _C.stream_ptr()), "tome_select")
    return [t for t, _ in outs], [b for _, b in outs]


def merge_into(x, gamma, beta, eps, grid, r, assign, kept, off):
    B, N, C = x.shape
    y, buf = _guard((B, N - r, C), x.dtype, x.device)
    _C.check(_C.load().st_tome_merge_norm(x.data_ptr(), x.stride(1), gamma.data_ptr(), beta.data_ptr(), eps, off.data_ptr(), None, off.shape[0],
                                          assign.data_ptr(), kept.data_ptr(), B, grid[0], grid[1], C, r, y.data_ptr(), _C.dtype_code(x.dtype),
                                          _C.stream_ptr()), "tome_merge_norm")
    return y, buf


def unmerge_into(x, y, where):
    B, N, C = x.shape
    (out, b0), (stats, b1) = _guard((B, N, C), x.dtype, x.device), _guard((B * N, 2), torch.float32, x.device)
    _C.check(_C.load().st_tome_unmerge_add(x.data_ptr(), x.stride(1), y.data_ptr(), where.data_ptr(), B, N, y.shape[1], C, out.data_ptr(),
                                           stats.data_ptr(), _C.dtype_code(x.dtype), _C.stream_ptr()), "tome_unmerge_add")
    return (out, stats), (b0, b1)
