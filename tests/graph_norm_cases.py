"""Shared by tests/test_graph_norm_host.py (CPU) and tests/test_gpu_graph_norm_kernels.py (GPU): the graph-size lists, the seeded
inputs, the oracle reference in fp64 and fp32, and the fp64-twin bound applied to every graph separately.  Imports no HIP.

Why per graph: PairNorm and the graph LayerNorm statistics normalise each graph on its own, and the kernel form is chosen by the
AVERAGE graph size — so one launch holds 1-row graphs beside 600-row ones, at input scales of 0.1 to 10.  One max-norm over the whole
tensor lets a wrong small graph hide under the large graph's bound; here every graph answers to the rounding noise and magnitude of its
own rows (``assert_fp32_parity``'s rule and its k = 8, unchanged)."""
import functools
import os
import zlib

import torch

import oracle.glam_oracle as O
from tests.conftest import EPS32, assert_fp32_parity  # noqa: F401  (assert_fp32_parity: the rule restated per graph below)

# ---- size lists ----------------------------------------------------------------------------------------------------------------
# wave per graph (N // B = 34): leading, inner and trailing empty graphs; exactly one 32-row register pass, one row more, two passes,
# a partial fourth pass (97); a 600-row graph in a small-mean batch; every remainder of colsum's 4-way unroll (1, 2, 3, 4, 5, 7, 8)
WAVE = [0, 1, 32, 33, 0, 64, 65, 97, 5, 600, 2, 3, 4, 7, 8] + [11, 19, 26, 14, 9, 30, 22, 17] * 3 + [0]
# block per graph (N // B = 153): fewer rows than the 16 row groups, the edges of block_colsum's 64-row unroll, empty and 1-row graphs
BLOCK = [300, 1, 0, 16, 15, 17, 48, 49, 63, 64, 65, 113, 700, 2, 1000, 0]
# a padded resident batch: ten molecules and the one phantom graph that holds the padding rows
PHANTOM = [20] * 10 + [6000]
# more graphs than one grid holds (2 048 blocks of 4 waves, or 2 048 blocks): the grid-stride loops wrap
STRIDE_WAVE = [1, 2, 3] * 3000
STRIDE_BLOCK = [64] * 2100
UNALIGNED = [5, 40, 300]
# a graph of all-zero rows (the second one) beside ordinary ones and a 1-row graph
ZERO_WAVE = [11, 40, 1, 19]
ZERO_BLOCK = [70, 300, 1, 90]

SIZE_LISTS = {"WAVE": WAVE, "BLOCK": BLOCK, "PHANTOM": PHANTOM, "STRIDE_WAVE": STRIDE_WAVE, "STRIDE_BLOCK": STRIDE_BLOCK,
              "UNALIGNED": UNALIGNED, "ZERO_WAVE": ZERO_WAVE, "ZERO_BLOCK": ZERO_BLOCK}
_SMALL_MEAN = {"WAVE": True, "BLOCK": False, "PHANTOM": False, "STRIDE_WAVE": True, "STRIDE_BLOCK": False, "UNALIGNED": False,
               "ZERO_WAVE": True, "ZERO_BLOCK": False}
for _name, _sizes in SIZE_LISTS.items():          # each list asserts its own side of the wave / block threshold
    assert (sum(_sizes) // len(_sizes) < 64) == _SMALL_MEAN[_name], _name
assert sum(WAVE) // len(WAVE) == 34 and sum(BLOCK) // len(BLOCK) == 153

# ---- settings: (kind, scale, eps); kind "pair" = PairNorm (mode 0), "layer" = graph LayerNorm statistics (mode 1) ------------------
SETTINGS = [("pair", 1.0, 1e-5), ("pair", 2.5, 1e-3), ("layer", 1.0, 1e-5)]
MODE = {"pair": 0, "layer": 1}


def setting_id(s):
    return f"{s[0]}-s{s[1]:g}-e{s[2]:g}"


# ---- the (size list, D) pairs of the GPU file, by the form they must reach; the host test runs every one of them ---------------------
PARITY_CASES = ([("WAVE", D) for D in (4, 60, 64)] + [("BLOCK", D) for D in (4, 60, 64)] + [("PHANTOM", D) for D in (4, 60, 64)]
                + [(n, D) for n in ("WAVE", "BLOCK") for D in (45, 65, 92, 256)] + [("PHANTOM", 92)])
IDENTITY_CASES = [("WAVE", 60), ("BLOCK", 60), ("WAVE", 92), ("BLOCK", 92)]
STRIDE_CASES = [("STRIDE_WAVE", 8), ("STRIDE_WAVE", 6), ("STRIDE_BLOCK", 4)]
ZERO_CASES = [("ZERO_WAVE", 60), ("ZERO_WAVE", 45), ("ZERO_BLOCK", 60)]
UNALIGNED_CASES = [("UNALIGNED", 60)]
DROP_CASES = [("WAVE", D) for D in (4, 60, 64)]
ALL_CASES = sorted(set(PARITY_CASES + IDENTITY_CASES + STRIDE_CASES + ZERO_CASES + UNALIGNED_CASES + DROP_CASES))


def batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


@functools.lru_cache(maxsize=None)
def inputs(sizes_name, D):
    """``(x, cot, cot_identity)`` fp32 on the CPU, seeded by the case: per-graph ``sd = exp(U(-2.3, 2.3))`` (0.1 to 10), a per-graph
    per-channel offset ``U(-3, 3)`` in units of ``sd`` (means that matter beside the spread), ``x = (randn + offset) * sd``; unit normal
    cotangents.  The ZERO lists get their second graph zeroed.  Shared: do not modify the tensors."""
    sizes = SIZE_LISTS[sizes_name]
    g = torch.Generator().manual_seed(zlib.crc32(f"{sizes_name}/{D}".encode()))
    batch, B = batch_of(sizes), len(sizes)
    N = batch.numel()
    sd = torch.exp(torch.empty(B, 1).uniform_(-2.3, 2.3, generator=g))
    offset = torch.empty(B, D).uniform_(-3.0, 3.0, generator=g)
    x = (torch.randn(N, D, generator=g) + offset[batch]) * sd[batch]
    cot = torch.randn(N, D, generator=g)
    cot_id = torch.randn(N, D, generator=g)
    if sizes_name.startswith("ZERO"):
        x[batch == 1] = 0.0
    return x, cot, cot_id


def oracle_fn(setting, batch, B):
    """The oracle's norm (weight = 1, bias = 0 for the LayerNorm: its statistics part) as ``f(x)``."""
    kind, scale, eps = setting
    if kind == "pair":
        return lambda x: O.pair_norm(x, batch, B, scale=scale, eps=eps)
    return lambda x: O.graph_layer_norm(x, x.new_ones(x.size(1)), x.new_zeros(x.size(1)), batch, B, eps=eps)


def run_oracle(setting, sizes, x, cot, dtype, cot_id=None):
    """``(y, dx)`` of the oracle with autograd on the CPU in ``dtype``; ``cot_id``: the identity output ``x`` is used as well, under that
    cotangent (``loss = <y, cot> + <x, cot_id>``)."""
    batch, B = batch_of(sizes), len(sizes)
    xr = x.to(dtype).requires_grad_(True)
    y = oracle_fn(setting, batch, B)(xr)
    loss = (y * cot.to(dtype)).sum()
    if cot_id is not None:
        loss = loss + (xr * cot_id.to(dtype)).sum()
    (dx,) = torch.autograd.grad(loss, [xr])
    return y.detach(), dx


@functools.lru_cache(maxsize=None)
def reference(sizes_name, D, setting, identity=False):
    """``{fp64: (y, dx), fp32: (y, dx)}`` of the case, computed once and shared (do not modify)."""
    x, cot, cot_id = inputs(sizes_name, D)
    sizes = SIZE_LISTS[sizes_name]
    return {dt: run_oracle(setting, sizes, x, cot, dt, cot_id if identity else None) for dt in (torch.float64, torch.float32)}


def reverse_rows(sizes):
    """The row permutation that reverses the order of the rows inside every graph (an involution; ``batch`` is unchanged by it)."""
    cnt = torch.tensor(sizes, dtype=torch.long)
    end = torch.cumsum(cnt, 0)
    beg = end - cnt
    batch = batch_of(sizes)
    return beg[batch] + end[batch] - 1 - torch.arange(batch.numel())


# ---- the bound -------------------------------------------------------------------------------------------------------------------
def _segment_amax(v, batch, B):
    """max over the rows of each graph and all channels of the non-negative ``v[N, D]``; 0 for an empty graph."""
    rows = v.reshape(v.size(0), -1).amax(dim=1) if v.numel() else v.new_zeros(v.size(0))
    return torch.zeros(B, dtype=v.dtype).scatter_reduce_(0, batch, rows, "amax", include_self=True)


def per_graph_ratio(got, ref64, ref32, sizes, k=8.0):
    """``(err_g, bound_g)`` per graph: ``assert_fp32_parity``'s rule ``bound = k * max(noise, 4 ulp(max(scale, 1)))`` with ``noise``
    (|fp32 oracle - fp64 oracle|) and ``scale`` (|fp64 oracle|) taken over that graph's rows alone."""
    g, r64, r32 = got.detach().cpu().double(), ref64.detach().cpu().double(), ref32.detach().cpu().double()
    assert g.shape == r64.shape == r32.shape, f"shape {tuple(g.shape)} vs {tuple(r64.shape)}"
    batch, B = batch_of(sizes), len(sizes)
    err = _segment_amax((g - r64).abs(), batch, B)
    noise = _segment_amax((r32 - r64).abs(), batch, B)
    scale = _segment_amax(r64.abs(), batch, B)
    bound = k * torch.maximum(noise, 4 * EPS32 * scale.clamp(min=1.0))
    nan = _segment_amax(torch.isnan(g).double(), batch, B) > 0          # amax's NaN handling is not relied upon
    err = torch.where(nan, torch.full_like(err, float("inf")), err)
    return err, bound


def assert_per_graph_parity(got, ref64, ref32, sizes, what, k=8.0, cap=1.0):
    """Every graph's error within ``cap`` times its own bound.  A failure names the worst graph, its size, error and bound; under
    ``GLAM_PARITY_REPORT`` the worst ratio is printed (as ``assert_fp32_parity`` does).  Returns the worst ratio."""
    err, bound = per_graph_ratio(got, ref64, ref32, sizes, k)
    ratio = err / bound
    worst = int(torch.argmax(ratio))
    if os.environ.get("GLAM_PARITY_REPORT"):
        print(f"[parity/graph] {what}: worst graph {worst} ({sizes[worst]} rows) err {err[worst]:.3e} bound {bound[worst]:.3e} "
              f"({ratio[worst]:.2f})", flush=True)
    bad = int((ratio > cap).sum())
    assert bad == 0, (f"{what}: {bad} of {len(sizes)} graphs outside {cap:g} x their bound; worst graph {worst} ({sizes[worst]} rows): "
                      f"max|d| = {err[worst]:.3e} > {cap:g} x {bound[worst]:.3e} (k = {k:g})")
    return float(ratio[worst])
