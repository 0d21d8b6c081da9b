"""CPU: the graph builders and the restatement of tests/triplet_cases.py, which tests/test_gpu_triplet_kernels.py holds the HIP kernels
against.  Three things are established here, without a GPU:

* the builders deliver the degree classes, the self-loops, the duplicate and the isolated ends they promise;
* ``aggregate_ref`` in fp64 IS the oracle's ``triplet_aggregate`` / ``triplet_light_aggregate`` (1e-12) once the parameters are mapped
  as ``TripletMessage._staged_weights()`` maps them;
* the cases discriminate: seven wrong kernels, written as mutations of the restatement and evaluated in fp32, each fail the very
  bound the GPU tests apply (``assert_fp32_parity``, k = 8) on a named case."""
import functools

import pytest
import torch
import torch.nn.functional as F

import oracle.glam_oracle as O
from tests import triplet_cases as T
from tests.conftest import assert_fp32_parity


# ---------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("seed", [0, 3])
def test_degree_ladder_delivers(seed, flip):
    g = T.degree_ladder(T.LADDER, seed, flip=flip)
    ei, N = g.edge_index, g.N
    assert N % 2 == 1 and all(N % m for m in (16, 32, 64)) and N < 400
    din, dout = T.degrees(ei, N)
    walked = dout if flip else din                    # the degree the ladder is on
    assert walked[:len(T.LADDER)].tolist() == T.LADDER
    assert walked[len(T.LADDER):-1].tolist() == [2] * (N - len(T.LADDER) - 1)
    for n in g.isolated:                              # first and last node: neither source nor target
        assert n in (0, N - 1) and din[n] == 0 and dout[n] == 0
    src, dst = (ei[1], ei[0]) if flip else (ei[0], ei[1])
    loops = (src == dst).nonzero().view(-1)
    assert sorted(src[loops].tolist()) == sorted([g.loop_only, g.loop_in])
    assert walked[g.loop_only] == 1 and walked[g.loop_in] >= 5
    pairs = torch.stack([src, dst], 1)
    uniq, cnt = torch.unique(pairs, dim=0, return_counts=True)
    assert uniq[cnt > 1].tolist() == [[g.dup_src, g.dup]] and cnt.max() == 2      # exactly one duplicated edge
    assert walked[g.dup] >= 7
    # shuffled: the edges are not grouped by the node whose segment they belong to
    assert (dst[1:] < dst[:-1]).any()
    assert not torch.equal(T.degree_ladder(T.LADDER, seed + 1, flip=flip).edge_index, ei)


def test_degree_ladder_undirected():
    g = T.degree_ladder(T.LADDER, 1, directed=False)
    din, dout = T.degrees(g.edge_index, g.N)
    assert torch.equal(din, dout) and (din[:len(T.LADDER)] >= torch.tensor(T.LADDER)).all()
    assert din[0] == 0 and din[-1] == 0


def test_stride_graph():
    N, hub = 1003, 900
    ei = T.stride_graph(N, hub, seed=2)
    din, _ = T.degrees(ei, N)
    want = torch.arange(N) % 4
    want[hub] = 130
    assert torch.equal(din, want) and int(ei.max()) < N and int(ei.min()) >= 0


@pytest.mark.parametrize("kind,in_le4,out_le4", [("a", True, True), ("b", True, False), ("c", False, True)])
def test_ell_mix_delivers(kind, in_le4, out_le4):
    ei, ea, N = T.ell_mix(kind)
    din, dout = T.degrees(ei, N)
    assert (int(din.max()) <= 4) == in_le4 and (int(dout.max()) <= 4) == out_le4
    assert N < 400 and ea.shape == (ei.size(1), 4)
    assert ((ea == 0) | (ea == 1)).all() and (ea.sum(1) == 1).all()              # one-hot rows of width 4
    if kind == "a":
        assert torch.equal(din, dout) and int(din.max()) == 4
    if kind == "b":
        assert int((dout == 5).sum()) == 1 and int(dout.max()) == 5
    if kind == "c":
        assert int((din == 5).sum()) == 1 and int(din.max()) == 5


# ---------------------------------------------------------------------------------------------
# the restatement against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("H,C,De", [(3, 10, 4), (1, 7, 6), (4, 5, 8), (2, 12, 3)])
def test_aggregate_ref_is_the_oracle(H, C, De, flip):
    g = T.degree_ladder(T.LADDER, 5, flip=flip)
    gen = torch.Generator().manual_seed(H * 100 + C)
    f64 = dict(dtype=torch.float64, generator=gen)
    x, ea = torch.randn(g.N, C, **f64), torch.randn(g.edge_index.size(1), De, **f64)
    wn, we, att = torch.randn(C, H * C, **f64), torch.randn(De, H * C, **f64), torch.randn(1, H, 3 * C, **f64)
    xw, a_ij, w_edge, M = T.staged_operands(x, ea, wn, we, att, H)
    got = T.aggregate_ref(xw, a_ij, ea, w_edge, M, g.edge_index, H, C, 0.2, True)
    ref = O.triplet_aggregate(xw, g.edge_index, ea @ we, att, H, 0.2).reshape(g.N, H * C)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
    din = T.degrees(g.edge_index, g.N)[0]
    assert (got[din == 0] == 0).all() and (din == 0).sum() >= 2


@pytest.mark.parametrize("C,De", [(9, 4), (16, 7)])
def test_light_aggregate_ref_is_the_oracle(C, De):
    g = T.degree_ladder(T.LADDER, 6)
    gen = torch.Generator().manual_seed(C)
    f64 = dict(dtype=torch.float64, generator=gen)
    x, ea = torch.randn(g.N, C, **f64), torch.randn(g.edge_index.size(1), De, **f64)
    wn, att = torch.randn(C, C, **f64), torch.randn(1, 2 * C + De, **f64)
    xw, a_ij, _, M = T.staged_operands(x, ea, wn, None, att, 1)
    got = T.aggregate_ref(xw, a_ij, ea, None, M, g.edge_index, 1, C, 0.2, False)
    ref = O.triplet_light_aggregate(xw, g.edge_index, ea, att, 0.2)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_tied_logits_give_the_mean():
    """``kind="ties"``: alpha is 1 / in-degree, the aggregate the plain mean of the messages (what the GPU test asserts)."""
    g = T.degree_ladder(T.LADDER, 7)
    inp = T.aggregate_inputs(g.edge_index, g.N, 2, 8, 4, True, 7, "ties")
    out, _ = T.run_aggregate_ref(inp, g.edge_index, 2, 8, 0.2, True, torch.float64)
    msg = (inp["edge_attr"].double() @ inp["w_edge"].double()) * inp["xw"].double().index_select(0, g.edge_index[0])
    assert (out - O.scatter(msg, g.edge_index[1], g.N, "mean")).abs().max().item() <= 1e-12


# ---------------------------------------------------------------------------------------------
# the cases discriminate: wrong kernels as mutations of the restatement
# ---------------------------------------------------------------------------------------------
def _segment_order(dst):
    """Per edge: its rank inside its target's CSR segment (the CSR is stable: edge-id order) and the segment's length."""
    order = torch.sort(dst, stable=True).indices
    deg = torch.bincount(dst)
    start = torch.cumsum(deg, 0) - deg
    rank = torch.empty_like(dst)
    rank[order] = torch.arange(dst.numel()) - start[dst[order]]
    return rank, deg[dst]


def _body(xw, a_ij, ea, we, M, ei, H, Cp, slope, emul, ai_from_src=False, softmax=O.segment_softmax):
    """``aggregate_ref`` with two switchable faults (where ``a_i`` is read; the softmax)."""
    src, dst = ei[0], ei[1]
    N = xw.size(0)
    logit = a_ij[:, :H].index_select(0, src if ai_from_src else dst) + (ea @ M)[:, :H] + a_ij[:, 4:4 + H].index_select(0, src)
    alpha = softmax(F.leaky_relu(logit, slope), dst, N)
    msg = alpha.unsqueeze(-1) * xw.index_select(0, src).view(-1, H, Cp)
    if emul:
        msg = msg * (ea @ we).view(-1, H, Cp)
    return O.scatter(msg, dst, N, "sum").reshape(N, H * Cp)


def _softmax_max_as_zero(l, idx, n):
    p = l.exp()
    return p / (O.scatter(p, idx, n, "sum").index_select(0, idx) + 1e-16)


def _softmax_ties_not_renormalised(l, idx, n):
    lo = -O.scatter(-l, idx, n, "max").index_select(0, idx)
    hi = O.scatter(l, idx, n, "max").index_select(0, idx)
    return torch.where(hi == lo, (l - hi).exp(), O.segment_softmax(l, idx, n))


def _mutation(kind, CH):
    """The wrong kernel ``kind`` as a function with ``aggregate_ref``'s signature; ``CH``: the edges per chunk of the kernel form."""
    def fn(xw, a_ij, ea, we, M, ei, H, Cp, slope, emul):
        rank, deg = _segment_order(ei[1])
        last = rank == deg - 1
        kw = {}
        if kind == "last edge of a multi-chunk segment dropped":
            keep = ~(last & (deg > CH))
            ei, ea = ei[:, keep], ea[keep]
        elif kind == "masked slot of a partial chunk counted":
            again = last & (deg % CH != 0)
            ei, ea = torch.cat([ei, ei[:, again]], 1), torch.cat([ea, ea[again]])
        elif kind == "stats max taken as 0":
            kw["softmax"] = _softmax_max_as_zero
        elif kind == "a_i read from the source":
            kw["ai_from_src"] = True
        elif kind == "self-loop skipped":
            keep = ei[0] != ei[1]
            ei, ea = ei[:, keep], ea[keep]
        elif kind == "duplicate edge counted once":
            key = ei[0] * xw.size(0) + ei[1]
            first = torch.ones_like(key, dtype=torch.bool)
            order = torch.sort(key, stable=True).indices
            first[order[1:]] = key[order[1:]] != key[order[:-1]]
            ei, ea = ei[:, first], ea[first]
        elif kind == "alpha not renormalised when all logits tie":
            kw["softmax"] = _softmax_ties_not_renormalised
        else:
            raise ValueError(kind)
        return _body(xw, a_ij, ea, we, M, ei, H, Cp, slope, emul, **kw)
    return fn


_H, _CP, _DE = 2, 8, 4
_CASES = {"ladder/normal": (False, "normal"), "flip/normal": (True, "normal"), "ladder/ties": (False, "ties"),
          "ladder/wide": (False, "wide")}


@functools.lru_cache(maxsize=None)
def _case(name):
    flip, kind = _CASES[name]
    g = T.degree_ladder(T.LADDER, 11, flip=flip)
    inp = T.aggregate_inputs(g.edge_index, g.N, _H, _CP, _DE, True, 11, kind)
    twin = {dt: T.run_aggregate_ref(inp, g.edge_index, _H, _CP, 0.2, True, dt) for dt in (torch.float64, torch.float32)}
    return g, inp, twin


def _caught(kind, CH, name):
    """Does the fp32 evaluation of the mutation fail the fp64-twin bound of the true restatement on case ``name`` (output or any
    gradient)?  Returns the quantities that fail."""
    g, inp, twin = _case(name)
    out, grads = T.run_aggregate_ref(inp, g.edge_index, _H, _CP, 0.2, True, torch.float32, fn=_mutation(kind, CH))
    (o64, g64), (o32, g32) = twin[torch.float64], twin[torch.float32]
    failed = []
    for what, got, r64, r32 in [("out", out, o64, o32)] + [(n, a, b, c) for n, a, b, c in zip(T.AGG_NAMES, grads, g64, g32)]:
        try:
            assert_fp32_parity(got, r64, r32, what, out_tol=1e-5 if what == "out" else None)
        except AssertionError:
            failed.append(what)
    return failed


# mutation -> the case that must catch it (and, where the point is that ordinary inputs do NOT, the case that must let it pass)
_MUTATIONS = [
    ("last edge of a multi-chunk segment dropped", "ladder/normal", None),
    ("masked slot of a partial chunk counted", "ladder/normal", None),
    ("stats max taken as 0", "ladder/wide", "ladder/normal"),               # logits of order 1 never needed the shift
    ("a_i read from the source", "ladder/normal", None),
    ("self-loop skipped", "ladder/normal", None),
    ("duplicate edge counted once", "ladder/normal", None),
    ("alpha not renormalised when all logits tie", "ladder/ties", "ladder/normal"),
]


@pytest.mark.parametrize("CH", [4, 2])
@pytest.mark.parametrize("kind,catcher,blind", _MUTATIONS, ids=[m[0].replace(" ", "_") for m in _MUTATIONS])
def test_cases_catch_the_wrong_kernel(kind, catcher, blind, CH):
    failed = _caught(kind, CH, catcher)
    assert "out" in failed, f"{kind} (CH={CH}): case {catcher} lets the forward pass"
    assert len(failed) >= 3, f"{kind} (CH={CH}): case {catcher} fails only {failed}"          # the gradients see it too
    if blind is not None:
        assert _caught(kind, CH, blind) == [], f"{kind}: expected to pass unseen on {blind} (the reason {catcher} exists)"
    if "chunk" in kind or "self-loop" in kind or "duplicate" in kind:
        assert "out" in _caught(kind, CH, "flip/normal")        # the by-source ladder holds the same classes in its in-degrees' place


def test_the_true_restatement_passes_its_own_bound():
    """The control of the mutation test: the unmutated fp32 restatement sits inside the bound on every case."""
    for name in _CASES:
        g, inp, twin = _case(name)
        out, grads = T.run_aggregate_ref(inp, g.edge_index, _H, _CP, 0.2, True, torch.float32, fn=_body)
        (o64, g64), (o32, g32) = twin[torch.float64], twin[torch.float32]
        assert torch.isfinite(out).all()
        assert_fp32_parity(out, o64, o32, f"{name} out", out_tol=1e-5)
        for n, a, b, c in zip(T.AGG_NAMES, grads, g64, g32):
            assert_fp32_parity(a, b, c, f"{name} {n}")
