"""GPU (MI355X): every dispatch form of the fused gather / softmax / scatter kernels of ``TripletMessage`` (csrc/triplet_kernels.h,
triplet_h1..h4.hip, triplet.hip, layer.hip, triplet_ws.hip, triplet_ws_b1.hip) against a plain restatement evaluated in fp64 and fp32
(``assert_twin_parity``, k = 8, forward 1e-5), on the graphs of tests/triplet_cases.py: one node on each side of every chunk edge of the
CSR walk, directed edges, self-loops, a duplicated edge, isolated nodes at both ends.  tests/test_triplet_cases_host.py shows on the CPU
that seven subtly wrong kernels fail this very bound on these cases.

Which kernel runs is decided at run time (width class, head count, edge width, in- / out-degree <= 4, one-hot bond rows, ``d_edge_attr``
wanted or not); every test reads the launches back from ``_lib.kernel_timer().records()`` — ``(label, grid, us)`` — and asserts the form
it names in its docstring.  The labelled launches of the general kernels do not carry their template arguments: ``(H, De, EMUL)`` are
the call's own arguments and ``(G, ITER)`` follow from ``Cp`` alone (``pick_shape``), so the class is pinned by the shape and, for
``G``, by ``grid == ceil(N / (256 / G))``.  ``k_reduce_partials`` has no label of its own: it appears under its kernel name.

No kernel here uses atomics: two HIP runs of every case must agree bit for bit."""
import os
import re

import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, layer, ops
from tests import triplet_cases as T
from tests.conftest import assert_twin_parity

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glam_amd", "csrc")


def _constant(fname, pattern):
    """An integer constant of the HIP sources, read from the source so that a case derived from it moves when it does."""
    with open(os.path.join(_CSRC, fname)) as f:
        m = re.search(pattern, f.read())
    assert m, f"{fname}: {pattern} not found"
    return int(m.group(1))


K_BLOCK = _constant("common.h", r"constexpr int kBlock = (\d+);")                  # threads per block
K_MAX_BLOCKS = _constant("common.h", r"constexpr int kMaxBlocks = (\d+);")          # cap of forward, B2 and dea (unfused)
K_BWD_BLOCKS = _constant("common.h", r"constexpr int kBwdBlocks = (\d+);")          # cap of B1 = rows of its partial buffer
K_FUSED_BLOCKS = _constant("triplet.hip", r"constexpr int kFusedBlocks = (\d+);")   # cap of the forms with a GEMM inside
K_WS_BLOCKS = _constant("triplet_pipe.h", r"int v = e \? atoi\(e\) : (\d+);")       # ws_grid_cap: the warp-specialised kernels

# pick_shape (csrc/triplet_kernels.h): Q = Cp / 4 -> (G, ITER); CH = 4 edges per chunk at ITER == 1, else 2
_SHAPE = {16: (4, 1), 20: (8, 1), 32: (8, 1), 36: (16, 1), 48: (16, 1), 96: (8, 3), 128: (16, 2), 256: (16, 4)}


def _grid(N, G, cap):
    return max(1, min(cap, -(-N // (K_BLOCK // G))))


def _labels(records):
    return [r[0] for r in records]


# ---------------------------------------------------------------------------------------------
# op level: ops.triplet_aggregate / ops.light_aggregate against aggregate_ref
# ---------------------------------------------------------------------------------------------
def _check_op(name, device, edge_index, N, H, Cp, De, emul, inp, slope=0.2, dea=False):
    """``ops.triplet_aggregate`` (``emul``) / ``ops.light_aggregate`` on ``inp`` (tests/triplet_cases.aggregate_inputs): the output and
    d_xw, d_a_ij, d_w_edge, d_M (and d_edge_attr with ``dea``) inside the fp64-twin bound of ``aggregate_ref``; two HIP runs bit-equal.
    Returns ``(aggr, {name: grad}, records of the second run)``."""
    gi = ops.GraphIndex(edge_index.to(device), N)
    runs = []
    for _ in range(2):
        ts = {n: (inp[n].to(device).requires_grad_(n != "edge_attr" or dea) if inp[n] is not None else None) for n in T.AGG_NAMES}
        with _lib.kernel_timer() as kt:
            if emul:
                out = ops.triplet_aggregate(ts["xw"], ts["a_ij"], ts["edge_attr"], ts["w_edge"], ts["M"], gi, H, Cp, slope)
            else:
                out = ops.light_aggregate(ts["xw"], ts["a_ij"], ts["edge_attr"], ts["M"], gi, Cp, slope)
            leaves = [n for n in T.AGG_NAMES if ts[n] is not None and ts[n].requires_grad]
            gs = dict(zip(leaves, torch.autograd.grad((out * inp["cot"].to(device)).sum(), [ts[n] for n in leaves])))
            torch.cuda.synchronize()
        runs.append((out.detach(), gs, kt.records()))
    (o1, g1, _), (o2, g2, rec) = runs
    assert torch.equal(o1, o2) and all(torch.equal(g1[n], g2[n]) for n in g1), f"{name}: two runs differ"

    def run(dt):
        return T.run_aggregate_ref(inp, edge_index, H, Cp, slope, emul, dt, want_dea=dea)
    assert_twin_parity(run, o1, [g1.get(n) for n in T.AGG_NAMES], name, list(T.AGG_NAMES))
    return o1, g1, rec


def _assert_op_forms(rec, N, H, Cp, De, emul, dea):
    """The four launches of the op (five with ``dea``), their order, and the grid that pins ``G``."""
    G, _ = _SHAPE[Cp]
    want = ["k_triplet_fwd", "k_triplet_bwd_dst", "k_reduce_partials"] + (["k_triplet_bwd_dea"] if dea else []) + ["k_triplet_bwd_src"]
    got = [n for n in _labels(rec) if "triplet" in n or "reduce" in n]
    assert got == want, got
    P = (De * H * Cp if emul else 0) + De * 4
    grids = {n: g for n, g, _ in rec}
    assert grids["k_triplet_fwd"] == _grid(N, G, K_MAX_BLOCKS) and grids["k_triplet_bwd_src"] == _grid(N, G, K_MAX_BLOCKS)
    assert grids["k_triplet_bwd_dst"] == _grid(N, G, K_BWD_BLOCKS)
    assert grids["k_reduce_partials"] == -(-P // 16)
    if dea:
        assert grids["k_triplet_bwd_dea"] == _grid(N, G, K_MAX_BLOCKS)


def _op_heads(Cp):
    """H = 3 up to the widest aggregate the package itself asks for (``ops.wide_layer_supported``: H * Cp + 8 <= 320), H = 1 beyond."""
    return 3 if 3 * Cp + 8 <= 320 else 1


@pytest.mark.parametrize("dea", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("Cp", [16, 20, 32, 36, 48, 96, 128, 256])
def test_aggregate_shape_classes(device, Cp, flip, dea):
    """``k_triplet_fwd`` / ``_bwd_dst`` / ``_bwd_src`` (and ``_bwd_dea``) ``<H, G, ITER, 4, true>`` + ``k_reduce_partials``: one width per
    live ``(G, ITER)`` class — Cp 16 (4,1), 32 (8,1), 48 (16,1), 96 (8,3), 128 (16,2), 256 (16,4) — and the class edges Cp 20 (Q = 5) and
    36 (Q = 9); H = 3 up to Cp = 96, H = 1 at 128 and 256.  The ladder puts degrees 0..9, 63..65 and 130 under the by-target walk
    (forward, B1, dea), ``flip`` under the by-source walk (B2): CH = 4 and CH = 2 meet odd, even, CH - 1, CH, CH + 1, 2 CH + 1."""
    H, De = _op_heads(Cp), 4
    g = T.degree_ladder(T.LADDER, Cp, flip=flip)
    inp = T.aggregate_inputs(g.edge_index, g.N, H, Cp, De, True, Cp + flip)
    out, _, rec = _check_op(f"aggregate Cp={Cp} H={H} flip={flip} dea={dea}", device, g.edge_index, g.N, H, Cp, De, True, inp, dea=dea)
    _assert_op_forms(rec, g.N, H, Cp, De, True, dea)
    din = T.degrees(g.edge_index, g.N)[0]
    assert (out[(din == 0).to(device)] == 0).all()


_HEAD_CASES = [(H, De, True) for H in (1, 2, 3, 4) for De in (4, 8)] + [(1, 4, False), (1, 8, False)]


@pytest.mark.parametrize("dea", [False, True])
@pytest.mark.parametrize("Cp", [48, 16])
@pytest.mark.parametrize("H,De,emul", _HEAD_CASES)
def test_aggregate_heads_and_edge_widths(device, H, De, emul, Cp, dea):
    """The ``H`` = 1..4, ``DE`` = 4 / 8 and ``EMUL`` instantiations of all four kernels (``emul = 0``: ``ops.light_aggregate``, H = 1, the
    message is ``alpha * x_j`` and ``w_edge`` does not exist) at Cp = 48 (G = 16, CH = 4) and Cp = 16 (G = 4), on the ladder;
    ``k_triplet_bwd_dea`` at every H and De with ``dea``."""
    g = T.degree_ladder(T.LADDER, 100 + H)
    inp = T.aggregate_inputs(g.edge_index, g.N, H, Cp, De, emul, 10 * H + De + emul)
    _, _, rec = _check_op(f"aggregate H={H} De={De} emul={emul} Cp={Cp} dea={dea}", device, g.edge_index, g.N, H, Cp, De, emul, inp, dea=dea)
    _assert_op_forms(rec, g.N, H, Cp, De, emul, dea)


@pytest.mark.parametrize("flip", [False, True])
def test_aggregate_padded_columns_stay_zero(device, flip):
    """Cp = 48 holding C = 45 (columns 45..47 of every head of ``xw`` and ``w_edge`` zero, as the layer pads them): the padded columns of
    ``aggr`` and ``d_xw`` are exactly zero, whatever the cotangent holds there."""
    H, Cp, De = 3, 48, 4
    g = T.degree_ladder(T.LADDER, 45, flip=flip)
    inp = T.aggregate_inputs(g.edge_index, g.N, H, Cp, De, True, 45, pad_from=45)
    out, gs, _ = _check_op(f"aggregate padded flip={flip}", device, g.edge_index, g.N, H, Cp, De, True, inp, dea=True)
    assert (out.view(g.N, H, Cp)[:, :, 45:] == 0).all() and (gs["xw"].view(g.N, H, Cp)[:, :, 45:] == 0).all()


@pytest.mark.parametrize("flip", [False, True])
def test_aggregate_grid_stride(device, flip):
    """N just above ``kMaxBlocks * 16`` at H = 1, Cp = 36 (G = 16: 16 nodes per block): forward, B2 and dea run ``kMaxBlocks`` blocks and
    B1 ``kBwdBlocks`` (its cap is lower: it wraps four times), so each block makes a second trip; every node has 0..3 incoming edges and
    one node BEHIND the wrap has 130 (``flip``: outgoing, under B2).  All of it against fp64 — not a sample."""
    H, Cp, De = 1, 36, 4
    G = _SHAPE[Cp][0]
    N = K_MAX_BLOCKS * (K_BLOCK // G) + 21
    ei = T.stride_graph(N, N - 16, seed=3)
    ei = ei.flip(0).contiguous() if flip else ei
    inp = T.aggregate_inputs(ei, N, H, Cp, De, True, 3)
    _, _, rec = _check_op(f"aggregate grid-stride flip={flip}", device, ei, N, H, Cp, De, True, inp, dea=True)
    _assert_op_forms(rec, N, H, Cp, De, True, True)
    grids = {n: g for n, g, _ in rec}
    assert grids["k_triplet_fwd"] == grids["k_triplet_bwd_src"] == grids["k_triplet_bwd_dea"] == K_MAX_BLOCKS
    assert grids["k_triplet_bwd_dst"] == K_BWD_BLOCKS


def test_aggregate_without_edges_and_without_nodes(device):
    """E = 0 with N = 5: ``aggr`` and every gradient exactly zero; N = 0: empty outputs, zero parameter gradients (no launch)."""
    H, Cp, De = 3, 48, 4
    for N in (5, 0):
        ei = torch.zeros(2, 0, dtype=torch.long)
        inp = T.aggregate_inputs(ei, N, H, Cp, De, True, N)
        out, gs, _ = _check_op(f"aggregate E=0 N={N}", device, ei, N, H, Cp, De, True, inp, dea=True)
        assert out.shape == (N, H * Cp) and (out == 0).all()
        for n in T.AGG_NAMES:
            assert gs[n].shape == inp[n].shape and (gs[n] == 0).all(), n


@pytest.mark.parametrize("Cp", [48, 96])
def test_aggregate_tied_logits(device, Cp):
    """``M = 0``, ``a_ij = 0``: every logit ties, alpha is exactly 1 / in-degree — ``aggr`` against the plain mean of the messages (and
    the twin bound as everywhere); CH = 4 (Cp = 48) and CH = 2 (Cp = 96).  B1 recomputes these alpha from ``stats``."""
    H, De = 3, 4
    g = T.degree_ladder(T.LADDER, 7)
    inp = T.aggregate_inputs(g.edge_index, g.N, H, Cp, De, True, 7, "ties")
    out, _, _ = _check_op(f"aggregate ties Cp={Cp}", device, g.edge_index, g.N, H, Cp, De, True, inp, dea=True)
    msg = (inp["edge_attr"].double() @ inp["w_edge"].double()) * inp["xw"].double().index_select(0, g.edge_index[0])
    mean = O.scatter(msg, g.edge_index[1], g.N, "mean")
    scale = max(1.0, mean.abs().max().item())
    assert (out.cpu().double() - mean).abs().max().item() <= 1e-5 * scale


@pytest.mark.parametrize("slope", [0.2, 0.01])
@pytest.mark.parametrize("Cp", [48, 96])
def test_aggregate_wide_logits(device, Cp, slope):
    """``a_ij`` scaled by 25: logits of about +-60 with a tail past 88.7, where ``exp`` leaves fp32 — finite, and inside the twin bound
    (the fp32 restatement subtracts the segment maximum too, so its own noise follows the range)."""
    H, De = 3, 4
    g = T.degree_ladder(T.LADDER, 8)
    inp = T.aggregate_inputs(g.edge_index, g.N, H, Cp, De, True, 8, "wide")
    logit = (inp["a_ij"][:, :H][g.edge_index[1]] + inp["a_ij"][:, 4:4 + H][g.edge_index[0]] + (inp["edge_attr"] @ inp["M"])[:, :H])
    assert logit.max() > 88.7 and logit.min() < -88.7 and logit.abs().median() > 15
    out, gs, _ = _check_op(f"aggregate wide Cp={Cp} slope={slope}", device, g.edge_index, g.N, H, Cp, De, True, inp, slope=slope, dea=True)
    assert torch.isfinite(out).all() and all(torch.isfinite(v).all() for v in gs.values())


# ---------------------------------------------------------------------------------------------
# layer level: layer.TripletMessage against layer_ref (O.triplet_message)
# ---------------------------------------------------------------------------------------------
_ROUTES = ["python", "default"]           # the Python autograd node (ops.USE_TORCH_EXT = False) / the default route (the C++ node)


def _set_route(monkeypatch, route):
    monkeypatch.setattr(ops, "USE_TORCH_EXT", False if route == "python" else "auto")


def _check_layer(name, device, C, H, De, edge_index, edge_attr, N, seed, dea=False, identity=False, att_scale=None):
    """``layer.TripletMessage(C, De, heads=H)`` on the device against ``O.triplet_message`` in fp64 / fp32: the output and the
    gradients of ``x``, the five parameters (and ``edge_attr`` with ``dea``).  ``identity``: through ``forward_with_identity``, with a
    second cotangent on the handed-back input — d_x is then the gradient of ``<out, cot> + <x, cot2>``.  ``att_scale`` multiplies
    ``weight_triplet_att`` (0: every logit ties; large: wide logits).  Two HIP runs bit-equal.  Returns ``(out, grads, records)``."""
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    conv = layer.TripletMessage(C, De, heads=H)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(C, generator=gen) * 0.1)
        if att_scale is not None:
            conv.weight_triplet_att.mul_(att_scale)
    names = [n for n, _ in conv.named_parameters()]
    ps0 = [p.detach().clone() for p in conv.parameters()]
    x0 = torch.randn(N, C, generator=gen)
    cot, cot2 = torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)

    def run(dt):
        xo = x0.to(dt).requires_grad_(True)
        ea = edge_attr.to(dt).requires_grad_(dea)
        ps = [p.to(dt).requires_grad_(True) for p in ps0]
        o = T.layer_ref(xo, edge_index, ea, *ps, heads=H)
        loss = (o * cot.to(dt)).sum() + ((xo * cot2.to(dt)).sum() if identity else 0)
        return o.detach(), list(torch.autograd.grad(loss, [xo] + ps + ([ea] if dea else [])))

    conv = conv.to(device)
    ei_d = edge_index.to(device)
    runs = []
    for _ in range(2):
        x = x0.to(device).requires_grad_(True)
        ea = edge_attr.to(device).requires_grad_(dea)
        with _lib.kernel_timer() as kt:
            if identity:
                out, ident = conv.forward_with_identity(x, ei_d, ea)
                loss = (out * cot.to(device)).sum() + (ident * cot2.to(device)).sum()
            else:
                out = conv(x, ei_d, ea)
                loss = (out * cot.to(device)).sum()
            gs = list(torch.autograd.grad(loss, [x] + list(conv.parameters()) + ([ea] if dea else [])))
            torch.cuda.synchronize()
        runs.append((out.detach(), gs, kt.records()))
    (o1, g1, _), (o2, g2, rec) = runs
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2)), f"{name}: two runs differ"
    assert_twin_parity(run, o1, g1, name, ["x"] + names + (["edge_attr"] if dea else []))
    return o1, g1, rec


_FUSED = ["k_triplet_fwd+update", "d_aggr+k_triplet_bwd_dst", "k_triplet_bwd_src+dx"]
_UNFUSED = ["k_triplet_fwd", "k_triplet_bwd_dst", "k_triplet_bwd_src"]
_LADDER_LAYERS = [  # (C, H, De, the aggregate launches expected)
    (60, 3, 4, _FUSED),         # Q = 15: fused update / d_aggr / d_x forms
    (45, 3, 8, _FUSED),         # Cp = 48 (Q = 12) on zero-padded rows, De = 8
    (64, 2, 4, _FUSED),         # Q = 16, the widest fused class
    (30, 3, 4, _UNFUSED),       # Cp = 32 (8, 1): k_ts_gemm -> k_triplet_fwd -> k_ts_gemm, unfused d_aggr and d_x
    (15, 3, 4, _UNFUSED),       # Cp = 16 (4, 1): the same chain
    (44, 4, 4, _FUSED),         # H * Cp + 8 = 184 <= 192: still the fused layer, at four heads
    (48, 4, 4, _UNFUSED),       # H * Cp + 8 = 200 > 192: fused_layer_supported is False, layer.py takes ops.triplet_layer_wide
]


@pytest.mark.parametrize("route", _ROUTES)
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("C,H,De,forms", _LADDER_LAYERS, ids=[f"C{c}-H{h}-De{d}" for c, h, d, _ in _LADDER_LAYERS])
def test_layer_on_the_ladder(device, monkeypatch, C, H, De, forms, flip, route):
    """``TripletMessage`` with continuous ``edge_attr`` (the general kernels) on the ladder and its ``flip``, both routes.  C = 60 / 45
    / 64 and C = 44 at H = 4: ``k_triplet_fwd+update``, ``d_aggr+k_triplet_bwd_dst``, ``k_triplet_bwd_src+dx`` (G = 16, the GEMMs inside).
    C = 30 / 15: the unfused chain ``k_ts_gemm`` -> ``k_triplet_fwd`` -> ``k_ts_gemm`` and the unfused backward.  C = 48 at H = 4 leaves
    the dense-kernel table (H * Cp + 8 = 200 > 192): ``layer.py`` takes ``ops.triplet_layer_wide`` — the plain aggregate kernels between
    library GEMMs — which is asserted from ``ops.fused_layer_supported`` and the labels."""
    _set_route(monkeypatch, route)
    g = T.degree_ladder(T.LADDER, C + H, flip=flip)
    ea = torch.randn(g.edge_index.size(1), De, generator=torch.Generator().manual_seed(C))
    _, _, rec = _check_layer(f"layer C={C} H={H} De={De} flip={flip} {route}", device, C, H, De, g.edge_index, ea, g.N, C + 7 * H)
    assert ops.fused_layer_supported(C, H, De) == (C != 48) and ops.wide_layer_supported(48, 4, 4)
    got = [n for n in _labels(rec) if "k_triplet" in n]
    assert got == forms, got
    if forms is _UNFUSED and C != 48:
        # the four dense products stand around the aggregate launches (k_ts_gemm or k_tall_x3, by the product's shape): node product and
        # update around the forward, d_aggr before B1, d_x behind B2
        names = _labels(rec)
        dense = lambda n: n.startswith(("k_ts_gemm", "k_tall_x3"))
        f, b1, b2 = (names.index(n) for n in _UNFUSED)
        assert dense(names[f - 1]) and dense(names[f + 1]) and dense(names[b1 - 1]) and any(dense(n) for n in names[b2 + 1:]), names


def test_layer_fused_grid_stride(device, monkeypatch):
    """C = 60, H = 3, N just above ``kFusedBlocks * 16``: the general fused forms (continuous ``edge_attr``; a node of in-degree 130
    behind the wrap) run ``kFusedBlocks`` / ``kBwdBlocks`` blocks, the warp-specialised forms (one-hot rows on a degree-4 ring lattice)
    ``ws_grid_cap`` = 256 blocks of 16-node tiles: every block wraps.  Both against fp64, not against each other."""
    _set_route(monkeypatch, "python")
    N = K_FUSED_BLOCKS * 16 + 21
    ei = T.stride_graph(N, N - 16, seed=5)
    ea = torch.randn(ei.size(1), 4, generator=torch.Generator().manual_seed(5))
    _, _, rec = _check_layer("layer fused grid-stride general", device, 60, 3, 4, ei, ea, N, 5)
    grids = {n: g for n, g, _ in rec}
    assert grids["k_triplet_fwd+update"] == K_FUSED_BLOCKS and grids["k_triplet_bwd_src+dx"] == K_FUSED_BLOCKS
    assert grids["d_aggr+k_triplet_bwd_dst"] == K_BWD_BLOCKS
    ei, ea, N = T.ring_lattice(N, seed=6)
    _, _, rec = _check_layer("layer fused grid-stride ws", device, 60, 3, 4, ei, ea, N, 6)
    grids = {n: g for n, g, _ in rec}
    assert N > 16 * K_WS_BLOCKS
    assert grids["k_triplet_fwd_ws+update"] == grids["d_aggr+k_triplet_bwd_dst_ws"] == grids["k_triplet_bwd_src_ws+dx"] == K_WS_BLOCKS


def _mixed_forms(rec):
    names = _labels(rec)
    return (any(n.startswith("k_triplet_fwd_ws") for n in names), any("k_triplet_bwd_src_ws" in n for n in names),
            any("k_triplet_bwd_dst_ws" in n for n in names), "k_triplet_bwd_dea" in names)


_MIXED = [("a", 60, 3), ("a", 45, 3), ("b", 60, 3), ("b", 45, 3), ("c", 60, 3), ("c", 45, 3), ("c", 44, 4)]


@pytest.mark.parametrize("route", _ROUTES)
@pytest.mark.parametrize("kind,C,H", _MIXED)
def test_layer_mixed_forms(device, monkeypatch, kind, C, H, route):
    """Forward and backward from different kernel families (one-hot bond rows of width 4, tests/triplet_cases.ell_mix), both routes:

    * (a) a symmetric molecule batch with ``d_edge_attr`` wanted: ``k_triplet_fwd_ws+update``, then the general
      ``d_aggr+k_triplet_bwd_dst`` + ``k_triplet_bwd_dea`` + ``k_triplet_bwd_src+dx`` on the ``aggr`` / ``stats`` the warp-specialised
      forward stored;
    * (b) in-degree <= 4, one out-degree 5: the same forward, both backward launches general;
    * (c) one in-degree 5, out-degree <= 4: the general ``k_triplet_fwd+update`` and ``d_aggr+k_triplet_bwd_dst``, then
      ``k_triplet_bwd_src_ws+dx``; also at H = 4 (C = 44), where B1 has no warp-specialised form.

    ``d_aggr+k_triplet_bwd_dst_ws`` runs in none of them."""
    _set_route(monkeypatch, route)
    ei, ea, N = T.ell_mix(kind, seed=C)
    assert _lib.api().glam_triplet_layer_ws_supported(H, (C + 3) // 4 * 4, 4, 1) == 1
    _, _, rec = _check_layer(f"layer mixed ({kind}) C={C} H={H} {route}", device, C, H, 4, ei, ea, N, C + ord(kind), dea=kind == "a")
    fwd_ws, src_ws, dst_ws, dea = _mixed_forms(rec)
    assert (fwd_ws, src_ws, dst_ws, dea) == (kind in "ab", kind == "c", False, kind == "a"), _labels(rec)
    assert "d_aggr+k_triplet_bwd_dst" in _labels(rec)
    assert ("k_triplet_fwd+update" in _labels(rec)) == (kind == "c") and ("k_triplet_bwd_src+dx" in _labels(rec)) == (kind != "c")


@pytest.mark.parametrize("C,H", [(60, 3), (45, 3), (44, 4)])
def test_layer_mixed_form_c_with_the_skip_addend(device, monkeypatch, C, H):
    """(c) through ``ops.triplet_layer(..., with_identity=True)`` (``forward_with_identity``, Python node) with a cotangent on the
    handed-back input: the addend joins d_x in the epilogue of ``k_triplet_bwd_src_ws+dx`` behind a GENERAL B1 — d_x is the fp64
    gradient of ``out + x``."""
    _set_route(monkeypatch, "python")
    ei, ea, N = T.ell_mix("c", seed=C)
    _, _, rec = _check_layer(f"layer mixed (c) + identity C={C} H={H}", device, C, H, 4, ei, ea, N, C + 1, identity=True)
    assert _mixed_forms(rec) == (False, True, False, False), _labels(rec)
    assert "d_aggr+k_triplet_bwd_dst" in _labels(rec)


def test_block_of_two_applications_on_mixed_form_c(device, monkeypatch):
    """(c) as a ``MessageBlock`` applied twice inside ``ops.weight_scope()`` (Python node, gradient carry; 520 atoms and more, from which
    on the applications park their weight-gradient operands): each application's data half is ``glam_triplet_layer_bwd_data_ell``
    (general ``d_aggr+k_triplet_bwd_dst`` + ``k_triplet_bwd_src_ws+dx``, twice), the parameter half ONE ``k_param_grads<sets>`` behind
    ``glam_triplet_layer_param_grads_sets``.  Against ``O.message_block`` twice: outputs, d_x and every parameter gradient."""
    _set_route(monkeypatch, "python")
    C = 60
    ei, ea, N = T.ell_mix("c", seed=9, sizes=(13, 9, 21, 17, 8, 25, 11, 19, 15, 23) * 4)
    assert N >= ops._WGRAD_BATCH_MIN_ROWS and ops.GRU_WGRAD_BATCH
    torch.manual_seed(9)
    blk = layer.MessageBlock(C, C, 4, norm="_None", dropout="_None()", conv="_TripletMessage", act="ReLU", res=True)
    sd0 = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    names = [n for n, _ in blk.named_parameters()]
    gen = torch.Generator().manual_seed(9)
    x0, cot, cot_h = torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)

    def run(dt):
        sd = {k: v.to(dt).requires_grad_(True) for k, v in sd0.items()}
        xo = x0.to(dt).requires_grad_(True)
        x1, h1 = O.message_block(sd, "", xo, ei, ea.to(dt), None, None, None)
        x2, h2 = O.message_block(sd, "", x1, ei, ea.to(dt), h1, None, None)
        gs = torch.autograd.grad((x2 * cot.to(dt)).sum() + (h2 * cot_h.to(dt)).sum(), [xo] + [sd[n] for n in names])
        return torch.cat([x2, h2], 1).detach(), list(gs)

    blk = blk.to(device)
    ei_d, ea_d = ei.to(device), ea.to(device)
    runs = []
    for _ in range(2):
        x = x0.to(device).requires_grad_(True)
        with _lib.kernel_timer() as kt, ops.weight_scope():
            x1, h1 = blk(x, ei_d, ea_d, h=None, batch=None)
            x2, h2 = blk(x1, ei_d, ea_d, h=h1, batch=None)
            gs = list(torch.autograd.grad((x2 * cot.to(device)).sum() + (h2.squeeze(0) * cot_h.to(device)).sum(), [x] + list(blk.parameters())))
            torch.cuda.synchronize()
        runs.append((torch.cat([x2, h2.squeeze(0)], 1).detach(), gs, kt.records()))
    (o1, g1, _), (o2, g2, rec) = runs
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2)), "two runs differ"
    assert_twin_parity(run, o1, g1, "block x2 on mixed (c)", ["x"] + names)
    names_l = _labels(rec)
    assert names_l.count("k_triplet_fwd+update") == 2 and names_l.count("d_aggr+k_triplet_bwd_dst") == 2
    assert names_l.count("k_triplet_bwd_src_ws+dx") == 2 and names_l.count("k_param_grads<sets>") == 1 and "k_param_grads" not in names_l
    assert not any("k_triplet_fwd_ws" in n or "k_triplet_bwd_dst_ws" in n for n in names_l), names_l


@pytest.mark.parametrize("att_scale", [0.0, 40.0])
def test_layer_ties_and_wide_logits_on_the_warp_specialised_route(device, monkeypatch, att_scale):
    """C = 60, H = 3, one-hot rows, degree <= 4 (``k_triplet_fwd_ws+update``, ``d_aggr+k_triplet_bwd_dst_ws`` — which recomputes alpha from
    ``stats`` in triplet_ws_b1.hip — and ``k_triplet_bwd_src_ws+dx``): ``weight_triplet_att = 0`` (every logit ties) and scaled by 40
    (logits of tens of units)."""
    _set_route(monkeypatch, "python")
    ei, ea, N = T.ell_mix("a", seed=2)
    out, gs, rec = _check_layer(f"layer ws att x {att_scale:g}", device, 60, 3, 4, ei, ea, N, 2, att_scale=att_scale)
    assert _mixed_forms(rec) == (True, True, True, False), _labels(rec)
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in gs)
