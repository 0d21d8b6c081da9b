"""The GCN aggregation of csrc/gcn.hip restated in numpy, and the edge lists its tests run on.

``gcn_ref`` / ``gcn_bwd_ref`` are the three formulas of include/glam_hip.h word for word (``deg``, ``out``, ``d_xw``) in the dtype asked
for; tests/test_gcn_cases_host.py pins them to ``oracle.glam_oracle.gcn_conv`` and its autograd and shows that six subtly wrong variants
fail the bound of the GPU test (tests/test_gpu_gcn_inline.py) on the main case.  No GPU here."""
import functools

import numpy as np
import torch

WIDTHS = (1, 4, 30, 60, 92)      # scalar (G = 16), 16-byte, scalar, 16-byte (G = 16), 16-byte (G = 32)


def _scale(edge_index, N, dtype, *, keep_loops=False, implicit=1.0, out_degree=False, once=False):
    src, dst = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    keep = np.ones(src.size, dtype=bool) if keep_loops else src != dst
    s, d = src[keep], dst[keep]
    if once:
        pairs = np.unique(np.stack([s, d]), axis=1)
        s, d = pairs[0], pairs[1]
    deg = np.full(N, implicit, dtype=dtype)
    np.add.at(deg, s if out_degree else d, 1)
    with np.errstate(divide="ignore"):
        dis = (1.0 / np.sqrt(deg)).astype(dtype)
    dis[~np.isfinite(dis)] = 0
    return s, d, dis


def gcn_ref(xw, edge_index, dtype=np.float64, **wrong):
    """``out[i] = dis[i] * (dis[i] * xw[i] + sum_{e -> i, src_e != i} dis[src_e] * xw[src_e])``, ``dis = (1 + #{e -> i : src_e != i})^-1/2``.
    ``wrong``: the switches of ``WRONG`` (each one a bug a kernel could have)."""
    drop_src, own = wrong.pop("drop_src", False), wrong.pop("own", True)
    xw = np.asarray(xw, dtype=dtype)
    N = xw.shape[0]
    s, d, dis = _scale(edge_index, N, dtype, **wrong)
    acc = dis[:, None] * xw if own else np.zeros_like(xw)
    w = np.ones(s.size, dtype=dtype) if drop_src else dis[s]
    np.add.at(acc, d, w[:, None] * xw[s])
    return dis[:, None] * acc


def gcn_bwd_ref(g, edge_index, dtype=np.float64):
    """``d_xw[j] = dis[j] * (dis[j] * g[j] + sum_{e : j -> i, i != j} dis[i] * g[i])``."""
    g = np.asarray(g, dtype=dtype)
    N = g.shape[0]
    s, d, dis = _scale(edge_index, N, dtype)
    acc = dis[:, None] * g
    np.add.at(acc, s, dis[d][:, None] * g[d])
    return dis[:, None] * acc


# six wrong variants (name -> switches of gcn_ref): each must FAIL the GPU test's bound on the main case
WRONG = {
    "loops kept": dict(keep_loops=True),                        # existing self-loops counted beside the implicit one
    "no implicit loop": dict(implicit=0.0, own=False),                   # neither the +1 of deg nor the own term
    "out-degree normalisation": dict(out_degree=True),
    "deg without the +1": dict(implicit=0.0),    # the own term is there, the degree forgets it
    "duplicates counted once": dict(once=True),
    "dis[src] dropped": dict(drop_src=True),
}


@functools.lru_cache(maxsize=None)
def main_case():
    """``(edge_index int64 [2, E], N)``: node 0 isolated; node 1 whose only in-edge is a self-loop; node 2 with in-degree 1 (one-way, from
    1); nodes 3 .. 6 with in-degrees 63, 64, 65, 300 and 20 .. 27 with 15, 16, 17, 31, 32, 33, 47, 48 (one lane short of, at and past every
    round of 16 / 32 index entries), all one-way; node 7 with a run of 200 self-loops cut in two by a real in-edge, three real in-edges in
    all, one of them a duplicate (8 -> 7 twice); a symmetric random part over nodes 40 .. 339 with its own duplicates and loops.  The
    edges are shuffled except node 7's run, which stays consecutive in the list (the CSR is stable: it is a run there too)."""
    rng = np.random.default_rng(7)
    N = 340
    edges = [(1, 1), (1, 2)]
    for node, deg in ((3, 63), (4, 64), (5, 65), (6, 300), (20, 15), (21, 16), (22, 17), (23, 31), (24, 32), (25, 33), (26, 47), (27, 48)):
        edges += [(40 + k, node) for k in range(deg)]
    a = rng.integers(40, N, 900)
    b = rng.integers(40, N, 900)                       # (a == b now and then: loops inside the random part)
    edges += list(zip(a.tolist(), b.tolist())) + list(zip(b.tolist(), a.tolist()))
    edges += [(int(a[0]), int(b[0]))] * 2              # duplicates
    edges = [edges[i] for i in rng.permutation(len(edges))]
    run = [(7, 7)] * 100 + [(8, 7)] + [(7, 7)] * 100 + [(9, 7), (8, 7)]
    cut = len(edges) // 2
    edges = edges[:cut] + run + edges[cut:]
    ei = torch.tensor(edges, dtype=torch.int64).t().contiguous()
    return ei, N


@functools.lru_cache(maxsize=None)
def single_case():
    """N = 1 with no edges."""
    return torch.zeros(2, 0, dtype=torch.int64), 1


def cases():
    return {"main": main_case(), "single": single_case()}


def inputs(N, D, seed=0):
    """``(xw, cot)`` fp32 ``[N, D]``."""
    g = torch.Generator().manual_seed(1000 * D + seed)
    return torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)


def run_ref(xw, cot, edge_index, dtype):
    """``(out, [d_xw])`` of the restatement in ``dtype`` (torch.float32 / torch.float64), as torch tensors — the ``run`` of
    ``assert_twin_parity``."""
    nd = np.float32 if dtype == torch.float32 else np.float64
    ei = edge_index.numpy()
    out = gcn_ref(xw.numpy().astype(nd), ei, nd)
    d = gcn_bwd_ref(cot.numpy().astype(nd), ei, nd)
    return torch.from_numpy(out), [torch.from_numpy(d)]
