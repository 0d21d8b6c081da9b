"""GPU (MI355X): DDI pair scoring — the doubly indexed fusion for small x small pairs (``glam_pair_pool_gather_fwd``,
csrc/pairgather.hip: one wave per pair) and ``ArchitectureDDI.encode_drugs`` / ``score_pairs`` on top of it.

The property everything rests on: with every drug held ONCE on both sides and a pair given as two indices, the fusion's max column (and
argmax) is bit for bit that of ``ops.pair_pool`` on physically gathered rows, and the whole ``[max, mean]`` sits within the fp64-twin
bound of the oracle on the gathered batches.  ``score_pairs`` is then checked against the oracle's two-drug model on the expanded
batches and against ``model(mol1, mol2)`` on them."""
import copy

import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, layer, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_molecule
from tests.conftest import assert_twin_parity

pytestmark = pytest.mark.gpu


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


def _ptr(sizes):
    return torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.long)


def _gathered(x, sizes, idx):
    """Rows and batch vector of the segments ``idx`` laid out one copy per pair (what a ``Batch`` of the selected graphs holds)."""
    off = _ptr(sizes)
    rows = torch.cat([x[off[q]:off[q + 1]] for q in idx]) if len(idx) else x[:0]
    return rows, _batch([sizes[q] for q in idx])


def _pair_pool_with_argmax(x1, x2, sp1, sp2):
    """``ops.pair_pool`` and the argmax its node keeps for the backward pass."""
    out = ops.pair_pool(x1.clone().requires_grad_(True), x2.clone().requires_grad_(True), sp1, sp2)
    arg = next(t for t in out.grad_fn.saved_tensors if t.dtype == torch.int32)
    return out.detach(), arg


# Both sides are cut the same way (two towers over one set of drugs).  Second-side segments of 1, 63, 64, 65 and 130 rows: below, at and
# above the 64-row chunk, and three chunks; first-side segments of 1, 2 and 33 rows: a lone row, one row pair, an odd last row.  Drug 2 is
# referenced many times, drug 7 never; (2, 2) and (6, 6) pair a drug with itself; (6, 6) is 130 x 130.
_SIZES = [1, 2, 33, 63, 64, 65, 130, 5]
_IDX1 = [2, 0, 1, 2, 2, 2, 3, 6, 2]
_IDX2 = [2, 4, 3, 5, 6, 0, 6, 6, 1]


@pytest.mark.parametrize("D", [4, 15, 16, 60, 64, 92, 128])
def test_gathered_fusion_equals_pair_pool_on_gathered_rows(device, D):
    """16-byte form (4, 16, 60, 64, 92, 128) and dword form (15).  ``P`` = 1, 4, 5, 9: one wave of a block, a full block, a partial last
    block (three waves without a pair), three blocks.  Both indices, either one (the other side physically gathered: identity there), and
    neither (``Q1 == Q2 == P``)."""
    torch.manual_seed(D)
    Q, b = len(_SIZES), _batch(_SIZES)
    x1, x2 = torch.randn(b.numel(), D), torch.randn(b.numel(), D)
    g1, gb1 = _gathered(x1, _SIZES, _IDX1)
    g2, gb2 = _gathered(x2, _SIZES, _IDX2)
    sp = ops.SegmentPtr(b.to(device), Q)
    d1, d2, dg1, dg2 = x1.to(device), x2.to(device), g1.to(device), g2.to(device)
    # the reference, once: pair_pool on physically gathered rows (a pair's values do not depend on the other pairs of the call)
    ref, ref_arg = _pair_pool_with_argmax(dg1, dg2, ops.SegmentPtr(gb1.to(device), 9), ops.SegmentPtr(gb2.to(device), 9))
    enc_ptr = _ptr(_SIZES)
    shift1 = enc_ptr[_IDX1] - _ptr([_SIZES[q] for q in _IDX1])[:-1]        # gathered row -> row of the encoding
    shift2 = enc_ptr[_IDX2] - _ptr([_SIZES[q] for q in _IDX2])[:-1]
    ref_arg = ref_arg.cpu().long()
    for P in (1, 4, 5, 9):
        i1, i2 = _IDX1[:P], _IDX2[:P]
        n1, n2 = int((gb1 < P).sum()), int((gb2 < P).sum())
        gsp1, gsp2 = ops.SegmentPtr(gb1[:n1].to(device), P), ops.SegmentPtr(gb2[:n2].to(device), P)
        zero = torch.zeros(P, dtype=torch.long)
        with torch.no_grad():
            runs = {"both": (ops.pair_pool_gather(d1, d2, sp, sp, i1, np.asarray(i2), return_argmax=True), shift1[:P], shift2[:P]),
                    "idx1 only": (ops.pair_pool_gather(d1, dg2[:n2], sp, gsp2, torch.tensor(i1), None, return_argmax=True), shift1[:P], zero),
                    "idx2 only": (ops.pair_pool_gather(dg1[:n1], d2, gsp1, sp, None, i2, return_argmax=True), zero, shift2[:P]),
                    "neither": (ops.pair_pool_gather(dg1[:n1], dg2[:n2], gsp1, gsp2, return_argmax=True), zero, zero)}
            again = ops.pair_pool_gather(d1, d2, sp, sp, i1, i2, return_argmax=True)
            plain = layer.dot_and_global_pool2_gather(d1, d2, sp, sp, i1, i2)                 # (argmax = NULL in the kernel)
        out, arg = runs["both"][0]
        assert torch.equal(out, again[0]) and torch.equal(arg, again[1]) and torch.equal(out, plain), f"P={P}: two runs differ"
        for mode, ((o, a), s1, s2) in runs.items():
            what = f"D={D} P={P} {mode}"
            assert o.shape == (P, 2) and a.shape == (P, 2) and a.dtype == torch.int32
            assert torch.equal(o[:, 0], ref[:P, 0]), f"{what}: max column differs from pair_pool on gathered rows"
            assert torch.equal(o, out), f"{what}: differs from the doubly indexed call"
            back = ref_arg[:P].clone()
            back[:, 0] += s1
            back[:, 1] += s2
            assert torch.equal(a.cpu().long(), back), f"{what}: argmax"

    def run(dt):
        return O.dot_and_global_pool(g1.to(dt), g2.to(dt), gb1, gb2, 9, 2), []
    assert_twin_parity(run, out, [], f"pair_pool_gather D={D}")


@pytest.mark.parametrize("D", [8, 15, 45])
def test_gathered_fusion_ties_route_to_the_first_flattened_pair(device, D):
    """Small-integer rows (every dot product exact), exactly duplicated rows on both sides: the maximum occurs several times in each pair
    and ``arg`` is its first flattened occurrence ``r1 * n2 + r2`` — 16-byte form (8) and dword form (15, 45), through swapping indices;
    70 second-side rows put duplicates in different 64-row chunks."""
    s1, s2, i1, i2 = [4, 3, 5], [5, 70], [1, 0, 2], [1, 0, 1]
    b1, b2 = _batch(s1), _batch(s2)
    g = torch.Generator().manual_seed(D)
    x1 = torch.randint(-1, 2, (b1.numel(), D), generator=g).float()
    x2 = torch.randint(-1, 2, (b2.numel(), D), generator=g).float()
    for a, b in [(3, 0), (2, 1), (5, 4), (6, 4), (9, 7), (10, 8), (11, 7)]:      # every first-side row has a twin: every score occurs twice
        x1[a] = x1[b]
    for a, b in [(1, 0), (3, 2), (4, 0), (5 + 69, 5 + 0), (5 + 65, 5 + 3), (5 + 64, 5 + 63)]:
        x2[a] = x2[b]
    sp1, sp2 = ops.SegmentPtr(b1.to(device), 3), ops.SegmentPtr(b2.to(device), 2)
    with torch.no_grad():
        out, arg = ops.pair_pool_gather(x1.to(device), x2.to(device), sp1, sp2, i1, i2, return_argmax=True)
    o1, o2 = _ptr(s1), _ptr(s2)
    for i, (a, b) in enumerate(zip(i1, i2)):
        S = x1[b1 == a].double() @ x2[b2 == b].double().T
        flat = S.reshape(-1)
        first = int(torch.argmax(flat))
        assert flat[first] == flat.max() and (flat == flat.max()).sum() > 1, "the case must hold a tie"
        assert first == int((flat == flat.max()).nonzero()[0]), "argmax must be the first occurrence"
        assert out[i, 0].item() == flat[first].item()
        assert arg[i].tolist() == [int(o1[a]) + first // s2[b], int(o2[b]) + first % s2[b]]
        assert abs(out[i, 1].item() - S.mean().item()) <= 1e-6


def test_gathered_fusion_empty_segments_and_no_pairs(device):
    """An empty segment on either side (or both): ``0, 0`` and ``arg = -1, -1``; ``P = 0`` launches nothing."""
    torch.manual_seed(0)
    s1, s2, i1, i2 = [3, 0, 5], [0, 6], [0, 1, 2, 1, 2], [1, 1, 0, 0, 1]
    b1, b2 = _batch(s1), _batch(s2)
    x1, x2 = torch.randn(b1.numel(), 60, device=device), torch.randn(b2.numel(), 60, device=device)
    sp1, sp2 = ops.SegmentPtr(b1.to(device), 3), ops.SegmentPtr(b2.to(device), 2)
    with torch.no_grad():
        out, arg = ops.pair_pool_gather(x1, x2, sp1, sp2, i1, i2, return_argmax=True)
        plain = ops.pair_pool_gather(x1, x2, sp1, sp2, i1, i2)
    assert torch.equal(out, plain)
    assert out[1:4].abs().max().item() == 0.0 and (arg[1:4] == -1).all()
    for i, rows in ((0, slice(0, 3)), (4, slice(3, 8))):
        S = x1[rows].double() @ x2.double().T
        assert abs(out[i, 0].item() - S.max().item()) <= 1e-4 and abs(out[i, 1].item() - S.mean().item()) <= 1e-4
        assert rows.start <= arg[i, 0].item() < rows.stop and 0 <= arg[i, 1].item() < 6
    with _lib.kernel_timer() as kt, torch.no_grad():
        none, narg = ops.pair_pool_gather(x1, x2, sp1, sp2, [], [], return_argmax=True)
    assert none.shape == (0, 2) and narg.shape == (0, 2) and kt.records() == [], "P = 0 launched something"


def test_gathered_fusion_refusals_come_before_any_launch(device):
    s1, s2 = [3, 4, 2], [5, 6]
    b1, b2 = _batch(s1), _batch(s2)
    x1, x2 = torch.randn(b1.numel(), 60, device=device), torch.randn(b2.numel(), 60, device=device)
    wide1, wide2 = torch.randn(b1.numel(), 132, device=device), torch.randn(b2.numel(), 132, device=device)
    sp1, sp2 = ops.SegmentPtr(b1.to(device), 3), ops.SegmentPtr(b2.to(device), 2)
    ok1, ok2 = [0, 2, 1, 1], [1, 0, 0, 1]
    with _lib.kernel_timer() as kt, torch.no_grad():
        for bad1, bad2 in (([0, 3, 1, 1], ok2), ([0, -1, 1, 1], ok2), (ok1, [1, 2, 0, 1]), (ok1, [1, 0, 0]), (ok1, [1, 0, 0, 1, 1]),
                           (ok1, None), (None, ok2), (None, None)):      # out of range, wrong lengths, identity with Q != P
            with pytest.raises(IndexError):
                ops.pair_pool_gather(x1, x2, sp1, sp2, bad1, bad2)
        with pytest.raises(GlamHipError, match="idx2 lives on a device.*read-back"):
            ops.pair_pool_gather(x1, x2, sp1, sp2, ok1, torch.tensor(ok2, device=device))
        with pytest.raises(GlamHipError, match="idx1 lives on a device.*read-back"):
            ops.pair_pool_gather(x1, x2, sp1, sp2, torch.tensor(ok1, device=device), ok2)
        with torch.enable_grad(), pytest.raises(GlamHipError, match="ops.pair_pool"):
            ops.pair_pool_gather(x1.clone().requires_grad_(True), x2, sp1, sp2, ok1, ok2)
        with torch.enable_grad(), pytest.raises(GlamHipError, match="ops.pair_pool"):
            ops.pair_pool_gather(x1, x2.clone().requires_grad_(True), sp1, sp2, ok1, ok2)
        with pytest.raises(GlamHipError, match="disagree"):                      # a width mismatch
            ops.pair_pool_gather(x1, x2[:, :56], sp1, sp2, ok1, ok2)
        with pytest.raises(GlamHipError, match="disagree"):                      # a row-count mismatch
            ops.pair_pool_gather(x1[:-1], x2, sp1, sp2, ok1, ok2)
        with pytest.raises(GlamHipError, match="132"):                           # D = 132: outside the kernel table
            ops.pair_pool_gather(wide1, wide2, sp1, sp2, ok1, ok2)
    assert kt.records() == [], "a refusal launched something"
    with _lib.kernel_timer() as kt, torch.enable_grad():       # grad mode alone is fine: nothing here requires grad
        assert ops.pair_pool_gather(x1, x2, sp1, sp2, ok1, ok2).shape == (4, 2)
    assert [(n, g) for n, g, _ in kt.records()] == [("k_pair_gather", 1)], "one launch of ceil(P / 4) blocks, nothing else"


# ---------------------------------------------------------------------------------------------
# ArchitectureDDI.encode_drugs / score_pairs
# ---------------------------------------------------------------------------------------------
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU")
_FIRST = [0, 1, 1, 4, 3, 1, 0, 4, 1]          # Q = 6 drugs, P = 9 pairs: drug 1 many times, drug 5 never, (1, 1) and (4, 4) with themselves
_SECOND = [2, 1, 0, 4, 1, 3, 2, 0, 2]


def _drugs(n=6, seed=5):
    rng = np.random.default_rng(seed)
    return [synth_molecule(rng) for _ in range(n)]


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDDI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **_ACTS, **kw).eval()


def _readout(sd, prefix, kind, x, batch, P, dt):
    if kind == "GlobalPool5":
        return O.global_pool5(x, batch, P)
    if kind == "GlobalLAPool":
        q = prefix + "pool."
        return O.global_attention(x, batch, P, sd[q + "gate_nn.weight"], sd[q + "gate_nn.bias"], sd[q + "nn.weight"], sd[q + "nn.bias"])
    C = x.size(1)
    lstm = torch.nn.LSTM(2 * C, C).to(dt)
    lstm.load_state_dict({k[len(prefix) + 5:]: v for k, v in sd.items() if k.startswith(prefix + "lstm.")})
    return O.set2set(x, batch, P, lstm, steps=3)


def _head_block(sd, prefix, x, act, end_norm):
    """``LinearBlock`` of the head: its norm (no ``batch``: statistics over the whole [P, .] matrix) in front of the linear layer."""
    if end_norm == "_LayerNorm":
        x = O.graph_layer_norm(x, sd[prefix + "norm.norm.weight"], sd[prefix + "norm.norm.bias"])
    return O.linear_block(sd, prefix, x, act)


def _oracle_ddi(sd, m1, m2, P, dt, mol_block, graph_norm, readout, end_norm):
    """``O.architecture_ddi`` where it can express the configuration; for the other readouts / a normed head the same assembly, line
    for line, out of the oracle's own pieces."""
    if readout == "GlobalPool5" and end_norm == "_None":
        return O.architecture_ddi(sd, m1, m2, P, message_steps=2, mol_block=mol_block, graph_norm=graph_norm, **_ACTS)
    x1, x2 = O.linear_block(sd, "mol1_lin0.", m1.x, "ReLU"), O.linear_block(sd, "mol2_lin0.", m2.x, "ReLU")
    h1 = h2 = None
    fusion = []
    for _ in range(2):
        x1, h1 = O.message_block(sd, "mol1_conv.", x1, m1.edge_index, m1.edge_attr, h1, m1.batch, P, conv=mol_block, norm=graph_norm, act="ReLU")
        x2, h2 = O.message_block(sd, "mol2_conv.", x2, m2.edge_index, m2.edge_attr, h2, m2.batch, P, conv=mol_block, norm=graph_norm, act="ReLU")
        fusion.append(O.dot_and_global_pool(x1, x2, m1.batch, m2.batch, P, stats=2))
    o1 = O.linear_block(sd, "mol1_flat.", _readout(sd, "mol1_readout.", readout, x1, m1.batch, P, dt), "ReLU")
    o2 = O.linear_block(sd, "mol2_flat.", _readout(sd, "mol2_readout.", readout, x2, m2.batch, P, dt), "ReLU")
    out = torch.cat([o1, o2, torch.cat(fusion, dim=-1)], dim=-1)
    return _head_block(sd, "lin_out1.", _head_block(sd, "lin_out0.", out, "ReLU", end_norm), "_None", end_norm)


@pytest.mark.parametrize("mol_block,readout,graph_norm,alpha,end_norm", [
    ("_NNConv", "GlobalPool5", "_None", 4, "_None"), ("_TripletMessage", "Set2Set", "_None", 4, "_None"),
    ("_NNConv", "GlobalLAPool", "_LayerNorm", 4, "_None"), ("_NNConv", "GlobalPool5", "_None", 1, "_None"),
    ("_NNConv", "GlobalPool5", "_None", 4, "_LayerNorm")])
def test_score_pairs_vs_oracle_on_the_expanded_batches(device, monkeypatch, mol_block, readout, graph_norm, alpha, end_norm):
    """``score_pairs(enc, first, second)`` against the oracle's two-drug model on the batches of the drugs ``first`` / ``second`` collated
    one per pair, and against ``model(mol1, mol2)`` on them: every step's fusion MAX is bit-equal.  hid = 15 takes the dword kernel on
    compacted rows; ``end_norm="_LayerNorm"`` normalises over the 9 pairs of the call in both routes."""
    drugs = _drugs()
    exp1, exp2 = Batch.from_data_list([drugs[q] for q in _FIRST]), Batch.from_data_list([drugs[q] for q in _SECOND])
    net = _net(mol_block=mol_block, mol_readout=readout, graph_norm=graph_norm, hid_dim_alpha=alpha, end_norm=end_norm)
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}

    def run(dt):
        sd = {k: v.to(dt) if v.is_floating_point() else v for k, v in sd0.items()}
        cast = lambda b: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
        with torch.no_grad():
            return _oracle_ddi(sd, cast(exp1), cast(exp2), 9, dt, mol_block, graph_norm, readout, end_norm), []
    net = net.to(device)
    net.graphed_call = False
    seen = {"model": [], "pairs": []}

    def spy(name, key):
        inner = getattr(model, name)

        def f(*a, **k):
            r = inner(*a, **k)
            seen[key].append(r[0].detach().clone())
            return r
        monkeypatch.setattr(model, name, f)
    spy("dot_and_global_pool2", "model")
    spy("dot_and_global_pool2_gather", "pairs")
    with torch.no_grad():
        enc = net.encode_drugs(Batch.from_data_list(drugs).to(device))
        out, contacts = net.score_pairs(enc, _FIRST, _SECOND, return_argmax=True)
        plain = net.score_pairs(enc, np.asarray(_FIRST), torch.tensor(_SECOND))
        full = net(exp1.to(device), exp2.to(device))
    hid = 15 * alpha
    assert enc.num_graphs == 6 and enc.flat1.shape == (6, hid) and enc.flat2.shape == (6, hid)
    assert len(enc.rows1) == len(enc.rows2) == 2 and all(r.is_contiguous() and r.shape == (enc.sp.N, hid) for r in enc.rows1 + enc.rows2)
    assert out.shape == (9, 1) and torch.equal(out, plain)
    assert len(contacts) == 2 and all(c.shape == (9, 2) and c.dtype == torch.int32 for c in contacts)
    what = f"{mol_block}/{readout}/{graph_norm}/alpha={alpha}/end={end_norm}"
    assert_twin_parity(run, out, [], "score_pairs " + what)
    assert_twin_parity(run, full, [], "model on the expanded batches " + what)
    assert len(seen["model"]) == 2 and len(seen["pairs"]) == 4            # (two score_pairs calls)
    for s, (a, b) in enumerate(zip(seen["pairs"][:2], seen["model"])):
        assert torch.equal(a[:, 0], b[:, 0]), f"step {s}: the fusion max differs from model(mol1, mol2)"
    # the contacts are rows of the encoding, inside the pair's own two segments
    seg = enc.sp.ptr.cpu()
    for c in contacts:
        c = c.cpu()
        for i, (a, b) in enumerate(zip(_FIRST, _SECOND)):
            assert seg[a] <= c[i, 0] < seg[a + 1] and seg[b] <= c[i, 1] < seg[b + 1]


def test_score_pairs_refuses_what_would_break_the_contract(device):
    drugs = Batch.from_data_list(_drugs()).to(device)
    net, other = _net().to(device), _net().to(device)
    with torch.no_grad():
        enc = net.encode_drugs(drugs)
        assert net.score_pairs(enc, _FIRST, _SECOND).shape == (9, 1)
        with _lib.kernel_timer() as kt:
            with pytest.raises(GlamHipError, match="another model"):
                other.score_pairs(enc, _FIRST, _SECOND)
            net.train()
            with pytest.raises(GlamHipError, match="training mode"):
                net.score_pairs(enc, _FIRST, _SECOND)
            with pytest.raises(GlamHipError, match="training mode"):
                net.encode_drugs(drugs)
            net.eval()
            with pytest.raises(GlamHipError, match="mol1_flat's norm _LayerNorm"):
                _net(flat_norm="_LayerNorm").to(device).encode_drugs(drugs)
            with pytest.raises(GlamHipError, match="mol1_conv's norm _GraphSizeNorm"):
                _net(graph_norm="_GraphSizeNorm").to(device).encode_drugs(drugs)
            with pytest.raises(IndexError, match=r"second must lie in \[0, 6\)"):
                net.score_pairs(enc, _FIRST, [6] * 9)
        assert kt.records() == [], "a refusal launched something"
    # stale after an optimizer step ...
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    with torch.no_grad():
        with _lib.kernel_timer() as kt, pytest.raises(GlamHipError, match="stale"):
            net.score_pairs(enc, _FIRST, _SECOND)
        assert kt.records() == []
        enc = net.encode_drugs(drugs)                                      # a fresh encoding is accepted again
        assert net.score_pairs(enc, _FIRST, _SECOND).shape == (9, 1)
        # ... and after load_state_dict
        net.load_state_dict(copy.deepcopy(net.state_dict()))
        with _lib.kernel_timer() as kt, pytest.raises(GlamHipError, match="stale"):
            net.score_pairs(enc, _FIRST, _SECOND)
        assert kt.records() == []
    with pytest.raises(GlamHipError, match="no_grad"):
        net.score_pairs(enc, _FIRST, _SECOND)
    with pytest.raises(GlamHipError, match="no_grad"):
        net.encode_drugs(drugs)
