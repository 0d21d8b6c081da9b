"""GPU (MI355X): every dispatch form of the readout and neighbour-sum kernels (csrc/pool.hip, csrc/pairpool.hip, and the block tail /
LSTM gate kernels of csrc/block.hip behind them) against a plain restatement evaluated in fp64 and fp32 (``assert_twin_parity``).

Each entry point picks among two to four kernel forms by width, alignment, segment length and ``K``; the shapes below are chosen so
that every form is launched (each test's docstring names the forms it reaches).  The restatements are the oracle's functions where it
has one, else a few lines of torch here with a citation of the behaviour they restate.  None of them calls the HIP library.

Ties under ``max`` are pinned to torch_scatter.scatter_max's routing (PyG 1.7.2, hence the reference): the lowest-index maximal row
takes the whole upstream gradient.  Every kernel here reduces in a fixed order, so each op is also checked to be bit-reproducible."""
import copy

import pytest
import torch
import torch.nn.functional as F

import oracle.glam_oracle as O
from glam_amd import layer, ops
from glam_amd._lib import GlamHipError
from tests.conftest import assert_twin_parity

pytestmark = pytest.mark.gpu


def _grads(out, cot, tensors):
    gs = torch.autograd.grad((out * cot).sum(), tensors, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(gs, tensors)]


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


def _unaligned(t):
    """A contiguous view of ``t``'s values at a 4-byte storage offset of a real allocation (16-byte alignment broken, in bounds;
    differentiable: the gradient arrives at ``t``)."""
    flat = torch.cat([t.new_zeros(1), t.reshape(-1)])
    u = flat[1:].view(t.shape)
    assert u.data_ptr() % 16 != 0
    return u


def _check(name, ref, dev, inputs, diff, cot, device, k=8.0):
    """``ref(*tensors) -> out`` (plain torch, CPU) and ``dev(*tensors) -> out`` (the HIP op); ``inputs`` are CPU tensors, ``diff`` the
    indices of those that carry a gradient.  The HIP output and gradients must sit within the fp64-twin bound, and two HIP runs must
    agree bit for bit."""
    def run(dt):
        ts = [t.to(dt) if t.is_floating_point() else t for t in inputs]
        ts = [t.requires_grad_(True) if i in diff else t for i, t in enumerate(ts)]
        o = ref(*ts)
        return o.detach(), _grads(o, cot.to(dt), [ts[i] for i in diff])

    results = []
    for _ in range(2):
        ts = [t.to(device) for t in inputs]
        ts = [t.requires_grad_(True) if i in diff else t for i, t in enumerate(ts)]
        o = dev(*ts)
        results.append((o.detach(), _grads(o, cot.to(device), [ts[i] for i in diff])))
    (o1, g1), (o2, g2) = results
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2)), f"{name}: two runs differ"
    assert_twin_parity(run, o1, g1, name, [str(i) for i in diff], k=k)
    return o1, g1


# ---------------------------------------------------------------------------------------------
# segment_pool: k_segment_pool_fwd / _bwd <0, 1, 2>
# ---------------------------------------------------------------------------------------------
_POOL_SIZES = [0, 3, 1, 0, 500, 7, 0, 64, 65, 1, 0]        # leading, inner and trailing empty segments; 1- and 500-row segments


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("D", [1, 45, 64, 65, 130])
def test_segment_pool(device, reduce, D):
    """``k_segment_pool_fwd/bwd<0|1|2>`` (sum / mean / max): the second lane pass starts at channel 65; empty segments give 0 (max:
    0 with no gradient, mean: no division by zero).  Restatement: the oracle's ``scatter`` (torch_scatter semantics)."""
    torch.manual_seed(D)
    sizes = _POOL_SIZES
    batch, B = _batch(sizes), len(sizes)
    x = torch.randn(batch.numel(), D)
    cot = torch.randn(B, D)
    sp = ops.SegmentPtr(batch.to(device), B)
    out, _ = _check(f"segment_pool {reduce} D={D}", lambda t: O.scatter(t, batch, B, reduce),
                    lambda t: ops.segment_pool(t, sp, reduce), [x], [0], cot, device)
    assert (out[torch.tensor(sizes) == 0] == 0).all()


def test_segment_pool_squeezed_and_grid_stride(device):
    """9 000 single-row graphs (more than the 2 048 x 4 waves of one grid: the grid-stride loop wraps), 1-D input (the squeezed form),
    every mode."""
    torch.manual_seed(1)
    B = 9000
    batch = torch.arange(B)
    sp = ops.SegmentPtr(batch.to(device), B)
    for reduce in ("sum", "mean", "max"):
        x = torch.randn(B)
        _check(f"segment_pool {reduce} B=9000 1-D", lambda t: O.scatter(t, batch, B, reduce),
               lambda t: ops.segment_pool(t, sp, reduce), [x], [0], torch.randn(B), device)
    x = torch.randn(B, 3)
    _check("segment_pool max B=9000 D=3", lambda t: O.scatter(t, batch, B, "max"),
           lambda t: ops.segment_pool(t, sp, "max"), [x], [0], torch.randn(B, 3), device)


@pytest.mark.parametrize("D", [2, 70])
def test_segment_pool_max_ties_route_to_the_first_row(device, D):
    """``k_segment_pool_fwd/bwd<2>`` on tied maxima (a dead channel: every row 0; repeated values): the lowest-index maximal row takes
    the whole gradient, every other row 0 — torch_scatter.scatter_max's arg routing, asserted element by element."""
    sizes = [4, 0, 6, 1]
    batch, B = _batch(sizes), len(sizes)
    N = batch.numel()
    x = torch.randint(-2, 3, (N, D)).float()
    x[:, 0] = 0.0                                        # dead channel
    x = x.to(device).requires_grad_(True)
    sp = ops.SegmentPtr(batch.to(device), B)
    out = ops.segment_pool(x, sp, "max")
    cot = torch.randn(B, D, device=device)
    (gx,) = torch.autograd.grad((out * cot).sum(), [x])
    xc, gx = x.detach().cpu(), gx.cpu()
    ref = torch.zeros(N, D)
    beg = 0
    for g, n in enumerate(sizes):
        for c in range(D):
            if n:
                col = xc[beg:beg + n, c]
                first = beg + int((col == col.max()).nonzero()[0])
                ref[first, c] = cot[g, c].item()
                assert out[g, c].item() == col.max().item()
            else:
                assert out[g, c].item() == 0.0
        beg += n
    assert torch.equal(gx, ref)


# ---------------------------------------------------------------------------------------------
# segment_attention: k_segment_attn_fwd/bwd_v4<16>, <32>, scalar
# ---------------------------------------------------------------------------------------------
def _attn_ref(batch, B):
    """GlobalAttention's read (PyG 1.7.2): ``softmax(gate, batch)`` (max-shifted, ``+1e-16``) then a segment sum of ``a * v``."""
    def f(gate, v):
        a = O.segment_softmax(gate.view(-1, 1), batch, B)
        return O.scatter(a * v, batch, B, "sum")
    return f


_ATTN_SIZES = [0, 1, 63, 64, 65, 800, 0, 5]


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("D", [30, 60, 90, 120, 180, 256])
def test_segment_attention(device, D, aligned):
    """``glam_segment_attn_fwd/bwd``: D = 60 -> ``v4<16>``, 120 -> ``v4<32>``, 30 / 90 / 180 / 256 -> scalar; an unaligned ``v`` (a view
    at a 4-byte offset) forces the scalar ``k_segment_attn_fwd/bwd`` at every width.  Segments of 0, 1, 63, 64, 65 and 800 rows; gate
    logits of +-80 (the max shift keeps the output finite).  Output, ``d_gate``, ``d_v``."""
    torch.manual_seed(D + aligned)
    batch, B = _batch(_ATTN_SIZES), len(_ATTN_SIZES)
    N = batch.numel()
    gate = torch.randn(N)
    gate[0] = 80.0                                       # the single-row segment
    gate[70:75] = torch.tensor([80.0, -80.0, 79.5, -80.0, 80.0])
    gate[300:310] = -80.0
    v = torch.randn(N, D)
    cot = torch.randn(B, D)
    sp = ops.SegmentPtr(batch.to(device), B)
    wrap = (lambda t: t) if aligned else _unaligned
    out, _ = _check(f"segment_attention D={D} aligned={aligned}", _attn_ref(batch, B),
                    lambda g, t: ops.segment_attention(g, wrap(t), sp), [gate, v], [0, 1], cot, device)
    assert torch.isfinite(out).all()


def test_segment_attention_grid_stride(device):
    """9 000 single-row graphs through ``v4<16>`` and the scalar form (D = 3): the grid-stride loop wraps."""
    torch.manual_seed(2)
    B = 9000
    batch = torch.arange(B)
    sp = ops.SegmentPtr(batch.to(device), B)
    for D in (8, 3):
        _check(f"segment_attention B=9000 D={D}", _attn_ref(batch, B), lambda g, t: ops.segment_attention(g, t, sp),
               [torch.randn(B) * 20, torch.randn(B, D)], [0, 1], torch.randn(B, D), device)


@pytest.mark.parametrize("C,sizes", [(15, [3, 20, 1, 0, 9]), (30, [12, 40, 2]), (45, [25, 7, 66, 1]), (60, [20, 13, 1, 28]),
                                     (90, [30, 4, 17]), (45, [310, 520, 1, 260])])
def test_global_lapool_widths(device, C, sizes):
    """``GlobalLAPool(C)`` end to end at the search space's widths (hid_dim_alpha 1, 2, 3, 4, 6): D = 2C = 30 / 90 / 180 -> scalar
    ``k_segment_attn_*``, 60 -> ``v4<16>``, 120 -> ``v4<32>``; the last case has protein-sized segments.
    Against ``O.global_attention``: output and every parameter gradient."""
    torch.manual_seed(70 + C)
    batch, B = _batch(sizes), len(sizes)
    ro = layer.GlobalLAPool(C)
    ps0 = [p.detach().clone() for p in ro.parameters()]
    names = [n for n, _ in ro.named_parameters()]
    x0 = torch.randn(batch.numel(), C)
    cot = torch.randn(B, 2 * C)

    def run(dt):
        xo = x0.to(dt).requires_grad_(True)
        pd = {n: p.to(dt).requires_grad_(True) for n, p in zip(names, ps0)}
        o = O.global_attention(xo, batch, B, pd["pool.gate_nn.weight"], pd["pool.gate_nn.bias"], pd["pool.nn.weight"], pd["pool.nn.bias"])
        return o.detach(), _grads(o, cot.to(dt), [xo] + [pd[n] for n in names])
    ro = ro.to(device)
    x = x0.to(device).requires_grad_(True)
    out = ro(x, batch.to(device), B)
    assert_twin_parity(run, out, _grads(out, cot.to(device), [x] + list(ro.parameters())), f"GlobalLAPool C={C}", ["x"] + names)


# ---------------------------------------------------------------------------------------------
# Set2Set: lstm_cell (k_lstm_cell_*) and query_attention (k_s2s_attn_*<16>, <32>)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_c", [True, False])
@pytest.mark.parametrize("C", [4, 16, 64, 68, 128])
def test_lstm_cell(device, C, use_c):
    """``k_lstm_cell_fwd/bwd``: torch.nn.LSTM's cell (gate order i | f | g | o); ``use_c=False`` leaves ``d_c`` unset (null)."""
    torch.manual_seed(C)
    B = 37
    gates, c0 = torch.randn(B, 4 * C) * 3, torch.randn(B, C)
    cot_h, cot_c = torch.randn(B, C), torch.randn(B, C)

    def cell(g, c):                               # torch.nn.LSTM cell: c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c')
        i, f, gg, o = g.chunk(4, dim=1)
        cn = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        return torch.sigmoid(o) * torch.tanh(cn), cn

    def both(fn):
        def f(g, c):
            h, cn = fn(g, c)
            return torch.cat([h, cn * cot_c.to(h.device, h.dtype)], 1) if use_c else h
        return f
    cot = torch.cat([cot_h, torch.ones(B, C)], 1) if use_c else cot_h
    _check(f"lstm_cell C={C} use_c={use_c}", both(cell), both(ops.lstm_cell), [gates, c0], [0, 1], cot, device)


def _s2s_attn_ref(batch, B):
    """Set2Set's read (PyG 1.7.2 Set2Set.forward): ``e = <x_n, q_g>``, ``a = softmax(e, batch)``, ``r = scatter_add(a * x, batch)``."""
    def f(x, q):
        e = (x * q.index_select(0, batch)).sum(-1, keepdim=True)
        return O.scatter(O.segment_softmax(e, batch, B) * x, batch, B, "sum")
    return f


@pytest.mark.parametrize("D", [4, 16, 64, 68, 128])
def test_query_attention(device, D):
    """``k_s2s_attn_fwd/bwd<16>`` (D <= 64) and ``<32>``: segments of 0 to 800 rows (one and several 32-row register passes)."""
    torch.manual_seed(D)
    sizes = [0, 1, 31, 32, 33, 200, 800, 3]
    batch, B = _batch(sizes), len(sizes)
    x, q = torch.randn(batch.numel(), D), torch.randn(B, D) * 0.5
    sp = ops.SegmentPtr(batch.to(device), B)
    _check(f"query_attention D={D}", _s2s_attn_ref(batch, B), lambda t, u: ops.query_attention(t, u, sp), [x, q], [0, 1],
           torch.randn(B, D), device)


@pytest.mark.parametrize("C,steps", [(64, 1), (68, 2), (16, 3), (15, 3), (130, 3)])
def test_set2set_steps_and_unfused_width(device, C, steps):
    """``Set2Set(C, steps)``: 1 to 3 fused steps (``lstm_cell`` + ``query_attention``); at C = 130 ``glam_s2s_attn_fwd`` refuses the
    width before any launch (GlamHipError) and the module takes its unfused path (scalar ``k_segment_attn_*``) — still the oracle's
    ``set2set``."""
    torch.manual_seed(C + steps)
    sizes = [12, 1, 70, 0, 33] if C != 130 else [12, 1, 70, 5]
    batch, B = _batch(sizes), len(sizes)
    if C == 130:
        sp = ops.SegmentPtr(batch.to(device), B)
        with pytest.raises(GlamHipError):
            ops.query_attention(torch.randn(batch.numel(), C, device=device), torch.randn(B, C, device=device), sp)
        assert not ops.query_attention_supported(132)
    ro = layer.Set2Set(C, steps)
    lstm_ref = copy.deepcopy(ro.lstm)
    names = [n for n, _ in lstm_ref.named_parameters()]
    x0 = torch.randn(batch.numel(), C)
    cot = torch.randn(B, 2 * C)

    def run(dt):
        l2 = copy.deepcopy(lstm_ref).to(dt)
        xr = x0.to(dt).requires_grad_(True)
        o = O.set2set(xr, batch, B, l2, steps=steps)
        return o.detach(), _grads(o, cot.to(dt), [xr] + [p for _, p in l2.named_parameters()])
    ro = ro.to(device)
    x = x0.to(device).requires_grad_(True)
    out = ro(x, batch.to(device), B)
    assert_twin_parity(run, out, _grads(out, cot.to(device), [x] + list(ro.lstm.parameters())), f"Set2Set C={C} steps={steps}",
                       ["x"] + names)


# ---------------------------------------------------------------------------------------------
# edge_reduce: k_edge_reduce_fwd / _bwd <0, 1, 2>
# ---------------------------------------------------------------------------------------------
def _edges(N, E, hub_deg=0, isolated=(), seed=0):
    """Random ``edge_index[2, E + hub_deg]``: node 0 receives ``hub_deg`` extra edges; no edge targets the ``isolated`` nodes."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E + hub_deg,), generator=g)
    dst = torch.randint(0, N, (E,), generator=g)
    for n in isolated:
        dst[dst == n] = 0
    dst = torch.cat([dst, torch.zeros(hub_deg, dtype=torch.long)])
    return torch.stack([src, dst])


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("D", [1, 64, 130])
def test_edge_reduce(device, reduce, D):
    """``k_edge_reduce_fwd/bwd<0|1|2>`` over the CSR by target: isolated targets (out 0), a hub of in-degree 1 000, D = 1 as a 1-D
    tensor (the squeezed form), D = 130.  Restatement: the oracle's ``scatter`` over ``edge_index[1]``."""
    torch.manual_seed(D)
    N = 300
    ei = _edges(N, 900, hub_deg=1000, isolated=(5, 6, 299), seed=D)
    E = ei.size(1)
    msg = torch.randn(E) if D == 1 else torch.randn(E, D)
    cot = torch.randn(N) if D == 1 else torch.randn(N, D)
    gi = ops.GraphIndex(ei.to(device), N)
    out, _ = _check(f"edge_reduce {reduce} D={D}", lambda m: O.scatter(m, ei[1], N, reduce), lambda m: ops.edge_reduce(m, gi, reduce),
                    [msg], [0], cot, device)
    assert (out[[5, 6, 299]] == 0).all()


def test_edge_reduce_no_edges_and_grid_stride(device):
    """E = 0 (every target isolated: zeros); 10 000 x 64 outputs, more than one grid of 2 048 x 256 threads (grid-stride wrap)."""
    gi0 = ops.GraphIndex(torch.zeros(2, 0, dtype=torch.long, device=device), 7)
    for reduce in ("sum", "mean", "max"):
        m = torch.zeros(0, 5, device=device, requires_grad=True)
        out = ops.edge_reduce(m, gi0, reduce)
        assert out.shape == (7, 5) and (out == 0).all()
        (g,) = torch.autograd.grad(out.sum(), [m])
        assert g.shape == (0, 5)
    torch.manual_seed(3)
    N = 10000
    ei = _edges(N, 20000, seed=3)
    gi = ops.GraphIndex(ei.to(device), N)
    for reduce in ("sum", "max"):
        _check(f"edge_reduce {reduce} N=10000", lambda m: O.scatter(m, ei[1], N, reduce), lambda m: ops.edge_reduce(m, gi, reduce),
               [torch.randn(ei.size(1), 64)], [0], torch.randn(N, 64), device)


def test_edge_reduce_max_ties_route_to_the_first_edge(device):
    """``k_edge_reduce_*<2>`` on tied messages: the lowest edge id among the maximal ones takes the gradient (scatter_max)."""
    N, D = 6, 3
    ei = torch.tensor([[0, 1, 2, 3, 4, 5, 0, 1], [1, 1, 1, 2, 2, 4, 4, 4]])
    msg = torch.tensor([[1.0, 0, 2], [3, 0, 2], [3, 0, 1], [0, 0, 0], [0, 0, 0], [5, 0, -1], [5, 1, -1], [4, 0, -1]])
    m = msg.to(device).requires_grad_(True)
    gi = ops.GraphIndex(ei.to(device), N)
    out = ops.edge_reduce(m, gi, "max")
    cot = torch.arange(1.0, 1.0 + N * D).view(N, D)
    (g,) = torch.autograd.grad((out * cot.to(device)).sum(), [m])
    ref = torch.zeros_like(msg)
    for n in range(N):
        es = (ei[1] == n).nonzero().view(-1)
        for c in range(D):
            if es.numel():
                col = msg[es, c]
                ref[es[int((col == col.max()).nonzero()[0])], c] = cot[n, c]
    assert torch.equal(g.cpu(), ref)
    assert torch.equal(out.detach().cpu(), O.scatter(msg, ei[1], N, "max"))


# ---------------------------------------------------------------------------------------------
# edge_weighted_sum: k_edge_wsum1_*_v4, k_edge_wsum_*<1, 4, 8>, k_edge_wsum_*_v4<4, 8>, glam_edge_wsum_bwd_add
# ---------------------------------------------------------------------------------------------
def _wsum_ref(ei, N, K, mean, self_slot):
    """``S[n,k,:] = (1/deg_n) sum_{e -> n} w[e,k] x[src_e,:]`` (PyG propagate with per-relation edge weights, aggr 'add' / 'mean');
    ``self_slot``: slot K of every node is its own row."""
    def f(x, w):
        msg = w.view(-1, K, 1) * x.index_select(0, ei[0]).unsqueeze(1)
        s = O.scatter(msg, ei[1], N, "mean" if mean else "sum")
        return torch.cat([s, x.unsqueeze(1)], 1) if self_slot else s
    return f


_WSUM_CASES = [  # (K, D, unaligned operands, mean, self_slot, with_identity)
    (1, 64, "", False, False, False),       # k_edge_wsum1_*_v4
    (1, 64, "x", True, False, False),       # k_edge_wsum_fwd<1> (unaligned x), k_edge_wsum1_bwd_v4
    (1, 45, "", True, False, False),        # k_edge_wsum_*<1>
    (4, 60, "", True, False, False),        # k_edge_wsum_*_v4<4>
    (4, 60, "", False, True, True),         # v4<4>, self_slot, glam_edge_wsum_bwd_add
    (8, 32, "", True, True, False),         # v4<8>, self_slot
    (8, 64, "", False, False, True),        # v4<8>, glam_edge_wsum_bwd_add
    (4, 45, "", False, False, False),       # k_edge_wsum_*<4>
    (8, 60, "xw", True, False, False),      # k_edge_wsum_*<8> (unaligned x and w)
    (4, 64, "w", False, False, True),       # k_edge_wsum_*<4> (unaligned w) with the identity: bwd_add refuses it, the add follows
]


@pytest.mark.parametrize("K,D,unaligned,mean,self_slot,with_identity", _WSUM_CASES)
def test_edge_weighted_sum(device, K, D, unaligned, mean, self_slot, with_identity):
    """``glam_edge_wsum_fwd/bwd`` (and ``_bwd_add`` when the identity output is used): every kernel form, isolated nodes and a hub of
    in-degree 1 000; ``d_x`` (``w`` is edge data: no gradient)."""
    torch.manual_seed(K * 100 + D)
    N = 200
    ei = _edges(N, 700, hub_deg=1000, isolated=(3, 4, 199), seed=K + D)
    E = ei.size(1)
    x, w = torch.randn(N, D), torch.randn(E, K)
    KS = K + int(self_slot)
    cot_s = torch.randn(N, KS, D)
    cot_id = torch.randn(N, D)
    ref_s = _wsum_ref(ei, N, K, mean, self_slot)
    gi = ops.GraphIndex(ei.to(device), N)

    def dev(xx, ww):
        xx = _unaligned(xx) if "x" in unaligned else xx
        ww = _unaligned(ww) if "w" in unaligned else ww
        if with_identity:
            s, ident = ops.edge_weighted_sum(xx, ww, gi, mean=mean, self_slot=self_slot, with_identity=True)
            return torch.cat([s.reshape(N, -1), ident], 1)
        return ops.edge_weighted_sum(xx, ww, gi, mean=mean, self_slot=self_slot).reshape(N, -1)

    def ref(xx, ww):
        s = ref_s(xx, ww).reshape(N, -1)
        return torch.cat([s, xx], 1) if with_identity else s
    cot = torch.cat([cot_s.reshape(N, -1), cot_id], 1) if with_identity else cot_s.reshape(N, -1)
    _check(f"edge_weighted_sum K={K} D={D} unaligned={unaligned!r} mean={mean} self={self_slot} id={with_identity}", ref, dev, [x, w], [0],
           cot, device)


def test_edge_weighted_sum_grid_stride(device):
    """40 000 x 16 float4 work items (v4 forms) and 10 000 x 60 scalar ones: more than one grid of 2 048 x 256 threads."""
    torch.manual_seed(4)
    for N, K, D in ((40000, 1, 64), (40000, 4, 64), (10000, 4, 61)):
        ei = _edges(N, 2 * N, seed=N + K)
        gi = ops.GraphIndex(ei.to(device), N)
        _check(f"edge_weighted_sum N={N} K={K} D={D}", lambda xx, ww: _wsum_ref(ei, N, K, True, False)(xx, ww).reshape(N, -1),
               lambda xx, ww: ops.edge_weighted_sum(xx, ww, gi, mean=True).reshape(N, -1),
               [torch.randn(N, D), torch.randn(ei.size(1), K)], [0], torch.randn(N, K * D), device)


# ---------------------------------------------------------------------------------------------
# pool5 / global_sort_pool: k_pool5_fwd (scalar), _v4<16>, _v4<32>, _block; k_pool5_bwd, _v4<16|32>, _block and its fallback
# ---------------------------------------------------------------------------------------------
def _pool5_ref(batch, B, k):
    """``mean || add || sort-pool(k)`` (GlobalPool5, src_1gp/layer.py:201-203, at any k): the oracle's mean / add, and PyG
    ``global_sort_pool`` restated without the per-graph loop — rows by last channel descending, node order on ties (stable, as
    ``O.global_sort_pool``), the first ``k`` per graph, zero rows behind a graph of fewer than ``k`` nodes."""
    N = batch.numel()
    cnt = torch.bincount(batch, minlength=B)
    start = torch.cumsum(cnt, 0) - cnt

    def f(x):
        D = x.size(1)
        order = torch.sort(x[:, -1].detach(), descending=True, stable=True).indices
        order = order[torch.sort(batch[order], stable=True).indices]          # by graph, then value descending, then node order
        rank = torch.arange(N) - start[batch[order]]
        keep = rank < k
        rows = order[keep]
        slot = batch[rows] * k + rank[keep]
        top = x.new_zeros(B * k, D).index_add(0, slot, x.index_select(0, rows)).view(B, k * D)
        return torch.cat([O.global_mean_pool(x, batch, B), O.global_add_pool(x, batch, B), top], 1)
    return f


_POOL5_CASES = [  # (D, padded_from, k, sizes): the forms reached
    (45, None, 3, [5, 1, 0, 2, 40, 9]),          # scalar fwd / bwd: unpadded odd width
    (132, None, 8, [9, 3, 0, 20, 1]),            # scalar: width above 128, k = 8, graphs with fewer than k rows
    (180, None, 1, [4, 70, 1, 0]),               # scalar, k = 1
    (45, 48, 3, [5, 1, 0, 2, 40, 9]),            # v4<16> on zero-padded rows (ld 48)
    (60, None, 8, [5, 1, 0, 2, 140, 9]),         # v4<16>, k = 8
    (90, 92, 1, [5, 1, 0, 2, 80, 9]),            # v4<32> on padded rows, k = 1
    (128, None, 3, [7, 0, 2, 65]),               # v4<32>
    (60, None, 3, [100, 64, 130, 90]),           # block fwd / bwd (N / B >= 64, D % 4 == 0, D <= 64)
    (4, None, 8, [70, 3, 200, 2, 81]),           # block, k = 8, graphs with fewer than k rows
]


@pytest.mark.parametrize("D,padded_from,k,sizes", _POOL5_CASES)
def test_pool5_forms(device, D, padded_from, k, sizes):
    """``glam_pool5_padded_fwd/bwd``: scalar ``k_pool5_fwd/bwd`` (unpadded odd widths, widths above 128), ``_v4<16>``, ``_v4<32>``
    (padded and unpadded rows), ``k_pool5_fwd_block`` / ``k_pool5_bwd_block``; k in {1, 3, 8}."""
    torch.manual_seed(D + k)
    batch, B = _batch(sizes), len(sizes)
    x = torch.randn(batch.numel(), D)
    sp = ops.SegmentPtr(batch.to(device), B)

    def dev(t):
        if padded_from:
            t = ops.slice_cols(F.pad(t, (0, padded_from - D)), D)    # the padded flow of odd widths: rows of ld floats
        return ops.pool5(t, sp, k)
    _check(f"pool5 D={D} ld={padded_from or D} k={k}", _pool5_ref(batch, B, k), dev, [x], [0], torch.randn(B, (2 + k) * D), device)


def test_pool5_block_backward_fallback(device):
    """``B * kPool5BwdChunks >= 65536`` with N / B >= 64: the forward is ``k_pool5_fwd_block``, the backward leaves
    ``k_pool5_bwd_block`` for ``k_pool5_bwd_v4<16>`` (8 192 graphs of 64 rows, D = 4)."""
    torch.manual_seed(5)
    B, n = 8192, 64
    batch = torch.arange(B).repeat_interleave(n)
    sp = ops.SegmentPtr(batch.to(device), B)
    _check("pool5 B=8192 block fallback", _pool5_ref(batch, B, 3), lambda t: ops.pool5(t, sp, 3), [torch.randn(B * n, 4)], [0],
           torch.randn(B, 20), device)


def test_global_sort_pool_k(device):
    """``global_sort_pool`` (layer.py) at k = 1 and 8, tied last channels included: node order on ties, zero rows behind short graphs."""
    sizes = [3, 12, 1, 9]
    batch, B = _batch(sizes), len(sizes)
    x = torch.randn(batch.numel(), 6)
    x[3:9, -1] = 0.5                                     # ties in the second graph
    for k in (1, 8):
        out = layer.global_sort_pool(x.to(device), batch.to(device), k)
        assert torch.equal(out.cpu(), O.global_sort_pool(x, batch, B, k)), f"k={k}"


# ---------------------------------------------------------------------------------------------
# pair_pool / pair_pool5 (dot_and_global_pool2 / 5): k_pair_max_partial + k_pair_finish, k_pair_pool_fwd, k_pair_stats5*
# ---------------------------------------------------------------------------------------------
def _pair_ref(mb, pb, P, stats):
    def f(mol, pro):
        return O.dot_and_global_pool(mol, pro, mb, pb, P, stats)
    return f


@pytest.mark.parametrize("with_identity", [False, True])
@pytest.mark.parametrize("D", [15, 45, 60, 90, 92])
def test_pair_pool(device, D, with_identity):
    """``glam_pair_pool_fwd/bwd``: widths with D % 4 == 0 and D <= 64 (60) take the split path (``k_pair_max_partial`` +
    ``k_pair_finish``, ``k_pair_pool_bwd_split``, and ``glam_pair_pool_bwd_add`` when the identities are used); the rest
    ``k_pair_pool_fwd`` / ``k_pair_pool_bwd``.  A one-residue protein graph.  Against ``O.dot_and_global_pool(stats=2)``."""
    torch.manual_seed(D + with_identity)
    ms, ps = [20, 7, 33, 1], [300, 1, 70, 129]
    mb, pb, P = _batch(ms), _batch(ps), len(ms)
    mol, pro = torch.randn(mb.numel(), D), torch.randn(pb.numel(), D)
    msp, psp = ops.SegmentPtr(mb.to(device), P), ops.SegmentPtr(pb.to(device), P)
    c_m, c_p = torch.randn(mb.numel(), D), torch.randn(pb.numel(), D)

    def pack(out, a, b):
        return torch.cat([out.reshape(-1), a.reshape(-1), b.reshape(-1)]) if with_identity else out

    def dev(a, b):
        if with_identity:
            return pack(*ops.pair_pool(a, b, msp, psp, with_identity=True))
        return ops.pair_pool(a, b, msp, psp)

    def ref(a, b):
        return pack(_pair_ref(mb, pb, P, 2)(a, b), a, b)
    cot = torch.randn(P, 2)
    if with_identity:
        cot = torch.cat([cot.reshape(-1), c_m.reshape(-1), c_p.reshape(-1)])
    _check(f"pair_pool D={D} id={with_identity}", ref, dev, [mol, pro], [0, 1], cot, device)


@pytest.mark.parametrize("D,C", [(16, 15), (48, 45), (60, 60), (92, 90), (92, 92)])
def test_pair_pool5(device, D, C):
    """``k_pair_stats5`` / ``k_pair_stats5_bwd`` (max, mean, median, min, std): D <= 64 and the wider form; odd widths padded with zero
    columns (``pad_cols``: a zero column changes no score).  A one-residue protein graph.  Against ``O.dot_and_global_pool(stats=5)``."""
    torch.manual_seed(D + C)
    ms, ps = [20, 7, 33, 4], [300, 1, 70, 129]
    mb, pb, P = _batch(ms), _batch(ps), len(ms)
    msp, psp = ops.SegmentPtr(mb.to(device), P), ops.SegmentPtr(pb.to(device), P)
    _check(f"pair_pool5 D={D} C={C}", _pair_ref(mb, pb, P, 5),
           lambda a, b: ops.pair_pool5(F.pad(a, (0, D - C)), F.pad(b, (0, D - C)), msp, psp),
           [torch.randn(mb.numel(), C), torch.randn(pb.numel(), C)], [0, 1], torch.randn(P, 5), device)


@pytest.mark.parametrize("D", [8, 12, 45])
def test_pair_pool_max_ties_route_to_the_first_flattened_pair(device, D):
    """Tied dot products (repeated ligand rows and residue rows, small integers: exact in any order): the maximum's gradient goes to
    the first flattened occurrence ``a * n_res + b`` of the pair's score matrix (pairpool.hip: ``bidx``), like a flattened argmax —
    split path (D = 8, 12) and one-block path (D = 45); the mean's gradient is unaffected."""
    ms, ps = [4, 3], [5, 6]
    mb, pb, P = _batch(ms), _batch(ps), len(ms)
    g = torch.Generator().manual_seed(D)
    mol = torch.randint(-1, 2, (mb.numel(), D), generator=g).float()
    pro = torch.randint(-1, 2, (pb.numel(), D), generator=g).float()
    mol[3], mol[6] = mol[0], mol[4]                        # repeated ligand rows: tied rows of S
    for a, b in [(1, 0), (3, 2), (4, 0), (6, 5), (8, 7), (10, 9)]:
        pro[a] = pro[b]                                    # every residue row twice: any maximum is tied
    m, p = mol.to(device).requires_grad_(True), pro.to(device).requires_grad_(True)
    msp, psp = ops.SegmentPtr(mb.to(device), P), ops.SegmentPtr(pb.to(device), P)
    out = ops.pair_pool(m, p, msp, psp)
    cot = torch.tensor([[1.5, 0.25], [-2.0, 0.5]])
    gm, gp = torch.autograd.grad((out * cot.to(device)).sum(), [m, p])

    mol64, pro64 = mol.double().requires_grad_(True), pro.double().requires_grad_(True)
    outs = []
    for i in range(P):
        S = mol64[mb == i] @ pro64[pb == i].T
        flat = S.reshape(-1)
        first = int(torch.argmax(flat.detach()))          # torch.argmax: the first maximal element
        assert flat[first] == flat.max() and (flat == flat.max()).sum() > 1, "the case must hold a tie"
        outs.append(torch.stack([flat[first], S.mean()]))
    ref = torch.stack(outs)
    rm, rp = torch.autograd.grad((ref * cot.double()).sum(), [mol64, pro64])
    assert torch.equal(out.detach().cpu()[:, 0].double(), ref.detach()[:, 0])      # the maximum is exact (small integers)
    assert (out.detach().cpu()[:, 1].double() - ref.detach()[:, 1]).abs().max() <= 1e-6
    assert (gm.cpu().double() - rm).abs().max() <= 1e-5 and (gp.cpu().double() - rp).abs().max() <= 1e-5


# ---------------------------------------------------------------------------------------------
# bias_res_act: k_bias_res_act_fwd / _bwd
# ---------------------------------------------------------------------------------------------
_ACTS = {"none": lambda t, s: t, "relu": lambda t, s: F.relu(t), "leaky": lambda t, s: F.leaky_relu(t, s), "celu": lambda t, s: F.celu(t)}


@pytest.mark.parametrize("has_bias,has_id", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("act", ["none", "relu", "leaky", "celu"])
@pytest.mark.parametrize("C", [15, 60, 130])
def test_bias_res_act(device, C, act, has_bias, has_id):
    """``k_bias_res_act_fwd/bwd`` (the GCN / GAT block tail ``act(y + bias + identity)``), the four deterministic activation codes; the
    rrelu code — and Dropout behind every code — is covered under its exact noise by ``test_elementwise_*`` in
    tests/test_gpu_training_noise.py (``glam_bias_res_act_rng_fwd / _bwd``).  A quarter
    of the pre-activations are exactly 0 (and -0.0 without bias / identity): the derivative the backward takes from ``out`` must follow
    torch's convention at 0 (ReLU 0, LeakyReLU ``slope``, CELU 1).  Values are multiples of 1/8, so the zeros are exact in any order."""
    torch.manual_seed(C)
    N, slope = 50, 0.01
    y = torch.randint(-16, 17, (N, C)).float() / 8
    bias = torch.randint(-8, 9, (C,)).float() / 8
    ident = torch.randint(-8, 9, (N, C)).float() / 8
    zero = torch.rand(N, C) < 0.25
    pre_other = (bias if has_bias else 0) + (ident if has_id else 0)
    y = torch.where(zero, -pre_other if (has_bias or has_id) else torch.full_like(y, -0.0), y)
    inputs, diff = [y], [0]
    if has_bias:
        inputs.append(bias)
    if has_id:
        inputs.append(ident)
    diff = list(range(len(inputs)))

    def split(ts):
        it = iter(ts[1:])
        return ts[0], (next(it) if has_bias else None), (next(it) if has_id else None)

    def ref(*ts):
        yy, b, i = split(ts)
        pre = yy + (b if b is not None else 0) + (i if i is not None else 0)
        return _ACTS[act](pre, slope)

    def dev(*ts):
        yy, b, i = split(ts)
        return ops.bias_res_act(yy, b, i, act, slope)
    out, grads = _check(f"bias_res_act C={C} {act} bias={has_bias} id={has_id}", ref, dev, inputs, diff, torch.randn(N, C), device)
    # at the exact zeros the derivative is torch's: compare d_y there bit for bit with torch on the same cotangent
    cot = torch.randn(N, C)
    yd = y.to(device).requires_grad_(True)
    args = [t.to(device) for t in inputs[1:]]
    o = dev(yd, *args)
    (gy,) = torch.autograd.grad((o * cot.to(device)).sum(), [yd])
    yr = y.clone().requires_grad_(True)
    (gr,) = torch.autograd.grad((ref(yr, *inputs[1:]) * cot).sum(), [yr])
    assert torch.equal(gy.cpu()[zero], gr[zero]), f"{act}: derivative at 0"
