"""GPU (MI355X): the attention export (``glam_amd.explain``, ``csrc/attn_export.hip``) against plain-torch restatements on the CPU in
fp32 and fp64 (``tests/explain_restated.py``, ``oracle/glam_oracle.py``).

fp32 bounds come from the restatement's own fp64 twin (tests/conftest.py: ``assert_fp32_parity``, k = 8).  The export is tied to what
the fused kernels compute: a layer's / readout's output REBUILT on the CPU in fp64 from the exported weights must lie within the
fp64-twin bound of the module's own HIP output."""
import functools

import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, explain, layer, model, ops
from glam_amd._lib import GlamHipError, ptr, stream
from glam_amd.data import synth_batch
from tests import explain_restated as R
from tests.conftest import EPS32, assert_fp32_parity

pytestmark = pytest.mark.gpu

IN_DEGREES = [0, 1, 4, 5, 63, 64, 65, 130, 0, 2]      # none; molecular; the group of 8 + 1... ; a wave -1 / = / +1; several passes


@functools.lru_cache(maxsize=None)
def _hub_graph():
    """One graph of ten nodes with IN_DEGREES, random sources among nodes 0..8 (node 9 sends nothing), edge order shuffled."""
    g = torch.Generator().manual_seed(7)
    dst = torch.repeat_interleave(torch.arange(10), torch.tensor(IN_DEGREES))
    src = torch.randint(0, 9, (dst.numel(),), generator=g)
    perm = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[perm], dst[perm]])


@functools.lru_cache(maxsize=None)
def _hub_inputs(De):
    g = torch.Generator().manual_seed(11 + De)
    E = _hub_graph().size(1)
    return 20 * torch.randn(10, 8, generator=g), torch.randn(E, De, generator=g), 3 * torch.randn(De, 4, generator=g)


def _twin_bound(r64, r32, k=8.0):
    """The bound ``assert_fp32_parity`` derives from a restatement's fp64 / fp32 twins."""
    r64, r32 = r64.detach().double(), r32.detach().double()
    return k * max((r32 - r64).abs().max().item(), 4 * EPS32 * max(r64.abs().max().item(), 1.0))


def _rows_sum_to_one(alpha, dst, N, what):
    """For every target of in-degree >= 1 and every head: |sum alpha - 1| <= 1e-5, summed in fp64."""
    a = alpha.detach().cpu().double()
    tot = O.scatter(a, dst.cpu(), N, "sum")
    has = O.scatter(torch.ones(dst.numel(), dtype=torch.float64), dst.cpu(), N, "sum") > 0
    err = (tot[has] - 1).abs().max().item() if bool(has.any()) else 0.0
    print(f"  {what}: max|sum alpha - 1| = {err:.2e}")
    assert err <= 1e-5, f"{what}: max|sum alpha - 1| = {err:.3e} > 1e-5"
    assert bool((tot[~has] == 0).all())


# ---------------------------------------------------------------------------------------------
# 1. the edge kernel on every in-degree class
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("De", [4, 8])
@pytest.mark.parametrize("H", [1, 3, 4])
def test_edge_attention_kernel_every_in_degree(device, H, De):
    ei = _hub_graph()
    a_ij, ea, M = _hub_inputs(De)
    E = ei.size(1)
    gi = ops.GraphIndex(ei.to(device), 10)
    args = (a_ij.to(device), ea.to(device), M.to(device), gi, H)
    alpha = explain.edge_attention(*args)
    assert alpha.shape == (E, H)
    ref = {dt: R.separable_alpha(a_ij.to(dt), ea.to(dt), M.to(dt), ei, 10, H) for dt in (torch.float32, torch.float64)}
    logit = (a_ij[ei[1], :H] + ea @ M[:, :H] + a_ij[ei[0], 4:4 + H])
    assert logit.abs().max() > 40, "the inputs are meant to make the max shift matter"
    err, bound = assert_fp32_parity(alpha, ref[torch.float64], ref[torch.float32], f"edge_attention H={H} De={De}", k=8)
    print(f"  edge_attention H={H} De={De}: max|d| = {err:.2e} (bound {bound:.2e}), max|logit| = {logit.abs().max():.1f}")
    storage = torch.as_strided(alpha, (E, 4), (4, 1))
    assert bool((storage[:, H:] == 0).all()), "columns H..3 of the [E, 4] storage are written as zero"
    assert torch.equal(storage[:, :H], alpha)
    again = explain.edge_attention(*args)
    assert torch.equal(again, alpha), "two runs are bit-equal"
    _rows_sum_to_one(alpha, ei[1], 10, f"edge_attention H={H} De={De}")
    ref_sum = O.scatter(ref[torch.float32].double(), ei[1], 10, "sum")[torch.tensor(IN_DEGREES) > 0]
    assert (ref_sum - 1).abs().max() <= 1e-5        # (the fp32 restatement itself: within 5e-7 on these inputs)


# ---------------------------------------------------------------------------------------------
# 2. grid-stride and empty problems
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [9000, 70000])           # 70 000: more groups than one sweep of the largest grid (2 048 blocks x 32 nodes)
def test_edge_attention_ring_every_alpha_is_one(device, N):
    g = torch.Generator().manual_seed(N)
    idx = torch.arange(N)
    ei = torch.stack([idx, (idx + 1) % N]).to(device)
    gi = ops.GraphIndex(ei, N)
    alpha = explain.edge_attention((5 * torch.randn(N, 8, generator=g)).to(device), torch.randn(N, 4, generator=g).to(device),
                                   torch.randn(4, 4, generator=g).to(device), gi, 3)
    assert alpha.shape == (N, 3) and bool((alpha == 1).all()), "in-degree 1: the softmax of one logit"
    sent = explain.attention_sent(alpha, gi)
    assert sent.shape == (N, 3) and bool((sent == 1).all())


def test_edge_attention_empty_problems(device):
    none = torch.zeros(2, 0, dtype=torch.int64, device=device)
    for N in (5, 0):
        gi = ops.GraphIndex(none, N)
        alpha = explain.edge_attention(torch.randn(N, 8, device=device), torch.zeros(0, 4, device=device), torch.randn(4, 4, device=device), gi, 3)
        assert alpha.shape == (0, 3)
        sent = explain.attention_sent(alpha, gi)
        assert sent.shape == (N, 3) and bool((sent == 0).all())
    sp = ops.SegmentPtr(torch.zeros(0, dtype=torch.int64, device=device), 0)
    assert explain.segment_softmax(torch.zeros(0, device=device), sp).shape == (0,)
    assert explain.query_softmax(torch.zeros(0, 16, device=device), torch.zeros(0, 16, device=device), sp).shape == (0,)


# ---------------------------------------------------------------------------------------------
# 3. attention sent
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 3, 4])
def test_attention_sent_is_the_scatter_by_source(device, H):
    ei = _hub_graph()
    a_ij, ea, M = _hub_inputs(4)
    gi = ops.GraphIndex(ei.to(device), 10)
    alpha = explain.edge_attention(a_ij.to(device), ea.to(device), M.to(device), gi, H)
    sent = explain.attention_sent(alpha, gi)
    assert sent.shape == (10, H)
    a = alpha.cpu()
    err, bound = assert_fp32_parity(sent, O.scatter(a.double(), ei[0], 10, "sum"), O.scatter(a, ei[0], 10, "sum"), f"attention_sent H={H}", k=8)
    print(f"  attention_sent H={H}: max|d| = {err:.2e} (bound {bound:.2e})")
    assert bool((sent[9] == 0).all()), "out-degree 0"
    assert torch.equal(explain.attention_sent(alpha, gi), sent)
    # a plain [E, H] tensor (not the view edge_attention returns) takes the same path after one pad
    assert torch.equal(explain.attention_sent(alpha.clone(), gi), sent)
    wide = torch.cat([alpha, alpha[:, :1] * 0.5, alpha], dim=1)                # more than four heads: groups of four
    got = explain.attention_sent(wide, gi)
    assert torch.equal(got[:, :H], sent) and torch.equal(got[:, H + 1:], sent)


# ---------------------------------------------------------------------------------------------
# 4. segment softmax: gate form and query form
# ---------------------------------------------------------------------------------------------
SEGMENTS = [0, 3, 1, 0, 500, 7, 0, 64, 65, 1, 0]


def _segments(device):
    batch = torch.repeat_interleave(torch.arange(len(SEGMENTS)), torch.tensor(SEGMENTS))
    return batch, ops.SegmentPtr(batch.to(device), len(SEGMENTS))


def _graphs_sum_to_one(w, batch, what):
    tot = O.scatter(w.detach().cpu().double(), batch, len(SEGMENTS), "sum")
    err = (tot[torch.tensor(SEGMENTS) > 0] - 1).abs().max().item()
    print(f"  {what}: max|sum w - 1| = {err:.2e}")
    assert err <= 1e-5


def test_segment_softmax_gate_form(device):
    batch, sp = _segments(device)
    gate = 10 * torch.randn(batch.numel(), generator=torch.Generator().manual_seed(3))
    w = explain.segment_softmax(gate.to(device), sp)
    assert w.shape == (batch.numel(),)
    ref = {dt: O.segment_softmax(gate.to(dt).view(-1, 1), batch, len(SEGMENTS)).view(-1) for dt in (torch.float32, torch.float64)}
    err, bound = assert_fp32_parity(w, ref[torch.float64], ref[torch.float32], "segment_softmax(gate)", k=8)
    print(f"  segment_softmax(gate): max|d| = {err:.2e} (bound {bound:.2e})")
    _graphs_sum_to_one(w, batch, "segment_softmax(gate)")
    assert torch.equal(explain.segment_softmax(gate.to(device), sp), w)


@pytest.mark.parametrize("D", [16, 60, 128, 15])       # 16 lanes per row, the same at full width, 32 lanes per row, an odd width on ld = 16
def test_segment_softmax_query_form(device, D):
    batch, sp = _segments(device)
    g = torch.Generator().manual_seed(D)
    x, q = torch.randn(batch.numel(), D, generator=g), torch.randn(len(SEGMENTS), D, generator=g)
    w = explain.query_softmax(x.to(device), q.to(device), sp)
    ref = {dt: O.segment_softmax((x.to(dt) * q.to(dt)[batch]).sum(-1, keepdim=True), batch, len(SEGMENTS)).view(-1)
           for dt in (torch.float32, torch.float64)}
    err, bound = assert_fp32_parity(w, ref[torch.float64], ref[torch.float32], f"query_softmax D={D}", k=8)
    print(f"  query_softmax D={D}: max|d| = {err:.2e} (bound {bound:.2e})")
    _graphs_sum_to_one(w, batch, f"query_softmax D={D}")
    assert torch.equal(explain.query_softmax(x.to(device), q.to(device), sp), w)
    if D % 4:
        # rows "hold D channels": whatever sits in columns D..ld of x and q does not enter the logit
        ld = (D + 3) // 4 * 4
        xg = torch.cat([x, 50 * torch.randn(x.size(0), ld - D, generator=g)], dim=1).to(device).contiguous()
        qg = torch.cat([q, 50 * torch.randn(q.size(0), ld - D, generator=g)], dim=1).to(device).contiguous()
        wg = torch.zeros_like(w)
        _lib.api().glam_segment_softmax(None, ptr(xg), ptr(qg), ptr(sp.ptr), sp.N, sp.B, D, ld, ptr(wg), stream())
        assert torch.equal(wg, w)


def test_segment_softmax_query_form_refuses_130_channels(device):
    batch, sp = _segments(device)
    with pytest.raises(GlamHipError, match="glam_segment_softmax"):
        explain.query_softmax(torch.randn(batch.numel(), 130, device=device), torch.randn(len(SEGMENTS), 130, device=device), sp)


# ---------------------------------------------------------------------------------------------
# 5. modules against the concatenated form (src_1gp/layer.py:48-51), and the fused layer rebuilt from the exported alpha
# ---------------------------------------------------------------------------------------------
def _star_graph():
    """Ten atoms, node 0 with in-degree 9 (no ELL form), every spoke answered, a few ring edges; directed both ways like a molecule."""
    spokes = [(k, 0) for k in range(1, 10)] + [(0, k) for k in range(1, 10)]
    ring = [(k, k + 1) for k in range(1, 9)] + [(k + 1, k) for k in range(1, 9)]
    return torch.tensor(spokes + ring).t().contiguous()


@functools.lru_cache(maxsize=None)
def _module_graph(graph):
    if graph == "star":
        ei = _star_graph()
        return ei, 10
    b = synth_batch(6, seed=5)
    return b.edge_index, b.x.size(0)


def _edge_features(E, De, seed):
    ea = torch.zeros(E, De)
    ea[torch.arange(E), torch.randint(0, De, (E,), generator=torch.Generator().manual_seed(seed))] = 1.0
    return ea


CONVS = {
    "triplet60x3": lambda: layer.TripletMessage(60, 4, heads=3),
    "triplet15": lambda: layer.TripletMessage(15, 4),
    "triplet60x6_de8": lambda: layer.TripletMessage(60, 8, heads=6),
    "light60": lambda: layer.TripletMessageLight(60, 4),
    "gat60": lambda: layer.GATConv(60, 60),
}


@pytest.mark.parametrize("graph", ["molecules", "star"])
@pytest.mark.parametrize("name", list(CONVS))
def test_conv_attention_against_the_concatenated_form(device, name, graph):
    torch.manual_seed(3)
    conv = CONVS[name]()
    ei, N = _module_graph(graph)
    E = ei.size(1)
    C = conv.node_channels if hasattr(conv, "node_channels") else 60
    De = getattr(conv, "edge_channels", 4)
    g = torch.Generator().manual_seed(17)
    x, ea = torch.randn(N, C, generator=g), _edge_features(E, De, 23)
    with torch.no_grad():
        conv.bias.normal_(0, 0.1, generator=g)
    P = {dt: {n: p.detach().to(dt) for n, p in conv.named_parameters()} for dt in (torch.float32, torch.float64)}

    def restated(dt):
        """(edge list, alpha, the layer's output by the oracle, a function rebuilding that output in this dtype from a given alpha)"""
        p, xd, ead = P[dt], x.to(dt), ea.to(dt)
        if isinstance(conv, layer.TripletMessage):
            a, e_ij, x_j = R.triplet_alpha(xd, ei, ead, p["weight_node"], p["weight_edge"], p["weight_triplet_att"], conv.heads)
            out = O.triplet_message(xd, ei, ead, p["weight_node"], p["weight_edge"], p["weight_triplet_att"], p["weight_scale"], p["bias"], conv.heads)
            return ei, a, out, lambda al: R.triplet_out_from_alpha(al, e_ij, x_j, ei, N, p["weight_scale"], p["bias"])
        if isinstance(conv, layer.TripletMessageLight):
            a, x_j = R.light_alpha(xd, ei, ead, p["weight_node"], p["weight_triplet_att"])
            out = O.triplet_message_light(xd, ei, ead, p["weight_node"], p["weight_triplet_att"], p["bias"])
            return ei, a, out, lambda al: O.scatter(al * x_j, ei[1], N, "sum") + p["bias"]
        ei2, a, x_j = R.gat_alpha(xd, ei, p["lin_l.weight"], p["att_l"], p["att_r"])
        out = O.gat_conv(xd, ei, p["lin_l.weight"], p["att_l"], p["att_r"], p["bias"])
        return ei2, a, out, lambda al: O.scatter(al * x_j, ei2[1], N, "sum") + p["bias"]

    ei32, a32, o32, _ = restated(torch.float32)
    ei64, a64, o64, rebuild64 = restated(torch.float64)

    conv = conv.to(device)
    xd, eid, ead = x.to(device), ei.to(device), ea.to(device)
    used, alpha = explain.conv_attention(conv, xd, eid) if isinstance(conv, layer.GATConv) else explain.conv_attention(conv, xd, eid, ead)
    H = getattr(conv, "heads", 1)
    assert alpha.shape == (ei64.size(1), H)
    assert torch.equal(used.cpu(), ei64), "the edge list the weights speak about (GATConv: with the self loops its forward adds)"
    if isinstance(conv, layer.GATConv):
        assert used.size(1) == E + N and torch.equal(used[:, E:].cpu(), torch.arange(N).repeat(2, 1)), "one self loop per node, appended"
    err, bound = assert_fp32_parity(alpha, a64, a32, f"{name}/{graph} alpha", k=8)
    print(f"  {name}/{graph}: alpha max|d| = {err:.2e} (bound {bound:.2e})")
    _rows_sum_to_one(alpha, used[1], N, f"{name}/{graph}")

    # consistency with the fused layer: its HIP output lies within its own fp64-twin bound of the output rebuilt from the EXPORTED alpha
    with torch.no_grad():
        out = conv(xd, eid) if isinstance(conv, layer.GATConv) else conv(xd, eid, ead)
    rebuilt = rebuild64(alpha.cpu().double())
    bound = _twin_bound(o64, o32)
    err = (out.cpu().double() - rebuilt).abs().max().item()
    print(f"  {name}/{graph}: |conv(x) - rebuilt from exported alpha| = {err:.2e} (fp64-twin bound of conv(x): {bound:.2e})")
    assert err <= bound
    # the wrapper of the same module gives the same weights
    if name == "triplet60x3":
        wrap = layer._TripletMessage(60, 60, 4).to(device)
        wrap.conv = conv
        assert torch.equal(explain.conv_attention(wrap, xd, eid, ead)[1], alpha)


def test_conv_attention_refuses_convs_without_attention(device):
    b = synth_batch(2, seed=2).to(device)
    x = torch.randn(b.x.size(0), 16, device=device)
    for conv in (layer._NNConv(16, 16, 4), layer._GCNConv(16, 16, 4)):
        with pytest.raises(GlamHipError, match="no attention weights"):
            explain.conv_attention(conv.to(device), x, b.edge_index, b.edge_attr)
    with pytest.raises(GlamHipError, match="no attention weights"):
        explain.readout_attention(layer.GlobalPool5(), x, b.batch)


# ---------------------------------------------------------------------------------------------
# 6. readouts
# ---------------------------------------------------------------------------------------------
def test_readout_attention_lapool(device):
    b = synth_batch(6, seed=9)
    N, B = b.x.size(0), 6
    torch.manual_seed(4)
    ro = layer.GlobalLAPool(60)
    x = torch.randn(N, 60)
    p = {dt: [t.detach().to(dt) for t in (ro.pool.gate_nn.weight, ro.pool.gate_nn.bias, ro.pool.nn.weight, ro.pool.nn.bias)]
         for dt in (torch.float32, torch.float64)}
    w_ref = {dt: O.segment_softmax(torch.nn.functional.linear(x.to(dt), p[dt][0], p[dt][1]), b.batch, B).view(-1) for dt in p}
    o_ref = {dt: O.global_attention(x.to(dt), b.batch, B, *p[dt]) for dt in p}
    ro = ro.to(device)
    xd, bd = x.to(device), b.batch.to(device)
    w = explain.readout_attention(ro, xd, bd, B)
    assert w.shape == (N,)
    err, bound = assert_fp32_parity(w, w_ref[torch.float64], w_ref[torch.float32], "GlobalLAPool weights", k=8)
    print(f"  GlobalLAPool weights: max|d| = {err:.2e} (bound {bound:.2e})")
    assert torch.equal(explain.readout_attention(ro.pool, xd, bd, B), w)
    with torch.no_grad():
        out = ro(xd, bd, B)
    v64 = torch.nn.functional.linear(x.double(), p[torch.float64][2], p[torch.float64][3])
    rebuilt = O.scatter(w.cpu().double().view(-1, 1) * v64, b.batch, B, "sum")
    bound = _twin_bound(o_ref[torch.float64], o_ref[torch.float32])
    err = (out.cpu().double() - rebuilt).abs().max().item()
    print(f"  GlobalLAPool: |readout(x) - scatter(w nn(x))| = {err:.2e} (fp64-twin bound of readout(x): {bound:.2e})")
    assert err <= bound


@pytest.mark.parametrize("C,steps", [(60, 3), (15, 2)])
def test_readout_attention_set2set(device, C, steps):
    b = synth_batch(6, seed=10)
    N, B = b.x.size(0), 6
    torch.manual_seed(5)
    ro = layer.Set2Set(C, steps)
    x = torch.randn(N, C)
    ref = {}
    for dt in (torch.float32, torch.float64):
        lstm = torch.nn.LSTM(2 * C, C).to(dt)
        lstm.load_state_dict({k: v.detach().to(dt) for k, v in ro.lstm.state_dict().items()})
        with torch.no_grad():
            ref[dt] = R.set2set_weights(x.to(dt), b.batch, B, lstm, steps)
            assert torch.equal(ref[dt][1], O.set2set(x.to(dt), b.batch, B, lstm, steps)), "the restatement is the oracle's recurrence"
    ro = ro.to(device)
    xd, bd = x.to(device), b.batch.to(device)
    w = explain.readout_attention(ro, xd, bd, B)
    assert w.shape == (steps, N)
    for s in range(steps):
        err, bound = assert_fp32_parity(w[s], ref[torch.float64][0][s], ref[torch.float32][0][s], f"Set2Set({C}) step {s}", k=8)
        print(f"  Set2Set({C}) step {s}: max|d| = {err:.2e} (bound {bound:.2e})")
        tot = O.scatter(w[s].cpu().double(), b.batch, B, "sum")
        assert (tot - 1).abs().max() <= 1e-5
    with torch.no_grad():
        out = ro(xd, bd, B)
    assert out.shape == (B, 2 * C)
    rebuilt = O.scatter(w[-1].cpu().double().view(-1, 1) * x.double(), b.batch, B, "sum")
    q64, q32 = ref[torch.float64][1][:, C:], ref[torch.float32][1][:, C:]
    bound = _twin_bound(q64, q32)
    err = (out[:, C:].cpu().double() - rebuilt).abs().max().item()
    print(f"  Set2Set({C}): |readout(x)[:, C:] - sum w x| = {err:.2e} (fp64-twin bound of the read: {bound:.2e})")
    assert err <= bound


# ---------------------------------------------------------------------------------------------
# 7. explain()
# ---------------------------------------------------------------------------------------------
PAIRS = [("_TripletMessage", "GlobalLAPool"), ("_TripletMessageLight", "Set2Set"), ("_GATConv", "GlobalPool5"), ("_NNConv", "GlobalPool5")]


@pytest.mark.parametrize("alpha_w", [1, 4])
@pytest.mark.parametrize("block,readout", PAIRS)
def test_explain(device, block, readout, alpha_w):
    B = 6
    b = synth_batch(B, seed=12)
    torch.manual_seed(6)
    m = model.Architecture(mol_block=block, mol_readout=readout, hid_dim_alpha=alpha_w).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(device)
    m.graphed_call = False
    bd = b.to(device)
    N, E, C = b.x.size(0), b.edge_index.size(1), 15 * alpha_w
    with torch.no_grad():
        ref = m(bd)
    ex = explain.explain(m, bd)
    assert torch.equal(ex.out, ref), "out is the eager eval forward, bit for bit"
    assert ex.out.shape == (B, 1) and ex.hidden.shape == (N, C) and not ex.out.requires_grad
    assert len(ex.edge_attention) == len(ex.atom_sent) == m.message_steps == 3
    conv = m.mol_conv.conv.conv
    assert not conv._forward_pre_hooks and not m.mol_readout._forward_pre_hooks and not m._forward_pre_hooks, "the hooks are gone"
    assert torch.equal(ex.weights("hidden_node"), ex.hidden.mean(-1))
    assert torch.equal(ex.ptr.cpu().long(), b.ptr)
    assert [t.size(0) for t in ex.per_molecule(ex.weights("hidden_node"))] == (b.ptr[1:] - b.ptr[:-1]).tolist()

    if block == "_NNConv":
        assert ex.edge_attention == [None] * 3 and ex.atom_sent == [None] * 3
        assert torch.equal(ex.edge_index, bd.edge_index)
        with pytest.raises(ValueError):
            ex.weights("edge_attention")
    else:
        H = 3 if block == "_TripletMessage" else 1
        Ex = E + N if block == "_GATConv" else E
        assert ex.edge_index.shape == (2, Ex)
        if block == "_GATConv":
            assert torch.equal(ex.edge_index[:, :E], bd.edge_index) and torch.equal(ex.edge_index[:, E:].cpu(), torch.arange(N).repeat(2, 1))
        for s, (a, snt) in enumerate(zip(ex.edge_attention, ex.atom_sent)):
            assert a.shape == (Ex, H) and snt.shape == (N, H)
            _rows_sum_to_one(a, ex.edge_index[1], N, f"explain {block} step {s}")
            ref_sent = O.scatter(a.cpu().double(), ex.edge_index[0].cpu(), N, "sum")
            assert (snt.cpu().double() - ref_sent).abs().max() <= 8 * 4 * EPS32 * max(1.0, ref_sent.abs().max().item())
        assert torch.equal(ex.weights("edge_attention"), ex.atom_sent[-1].mean(-1))
        per_edge = ex.per_molecule(ex.edge_attention[-1], per="edge")
        assert len(per_edge) == B and sum(t.size(0) for t in per_edge) == Ex
        # the first message step's weights against the concatenated form on the CPU: its input is the embedding mol_lin0(x) in eval mode
        x0 = {dt: O.linear_block({k: v.to(dt) for k, v in sd.items()}, "mol_lin0.", b.x.to(dt), "RReLU") for dt in (torch.float32, torch.float64)}
        pre = "mol_conv.conv.conv."
        twin = {}
        for dt in x0:
            p = {k[len(pre):]: v.to(dt) for k, v in sd.items() if k.startswith(pre)}
            if block == "_TripletMessage":
                twin[dt] = R.triplet_alpha(x0[dt], b.edge_index, b.edge_attr.to(dt), p["weight_node"], p["weight_edge"], p["weight_triplet_att"], 3)[0]
            elif block == "_TripletMessageLight":
                twin[dt] = R.light_alpha(x0[dt], b.edge_index, b.edge_attr.to(dt), p["weight_node"], p["weight_triplet_att"])[0]
            else:
                twin[dt] = R.gat_alpha(x0[dt], b.edge_index, p["lin_l.weight"], p["att_l"], p["att_r"])[1]
        err, bound = assert_fp32_parity(ex.edge_attention[0], twin[torch.float64], twin[torch.float32], f"explain {block} step 0", k=8)
        print(f"  explain {block} x{alpha_w} step 0: alpha max|d| = {err:.2e} (bound {bound:.2e})")

    if readout == "GlobalLAPool":
        assert ex.readout_attention.shape == (N,) and ex.weights("lapool_attention") is ex.readout_attention
        assert torch.equal(ex.readout_attention, explain.readout_attention(m.mol_readout, ex.hidden, bd.batch, B))
    elif readout == "Set2Set":
        assert ex.readout_attention.shape == (3, N) and torch.equal(ex.weights("set2set_attention"), ex.readout_attention[-1])
    else:
        assert ex.readout_attention is None
        with pytest.raises(ValueError):
            ex.weights("lapool_attention")
    if ex.readout_attention is not None:
        tot = O.scatter(ex.readout_attention.reshape(-1, N)[-1].cpu().double(), b.batch, B, "sum")
        assert (tot - 1).abs().max() <= 1e-5

    # the model is untouched: a training step still runs and gives finite gradients
    m.train()
    out = m(bd)
    out.sum().backward()
    grads = [p.grad for p in m.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    with pytest.raises(GlamHipError, match="training mode"):
        explain.explain(m, bd)
