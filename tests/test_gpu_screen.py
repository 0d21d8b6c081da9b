"""GPU (MI355X): screening — the pair-indexed fusion (``glam_pair_pool_indexed_fwd``: csrc/pairpool.hip with ``kIndexed``) and
``ArchitectureDTI.encode_proteins`` / ``screen`` on top of it.

The property everything rests on: with each protein held ONCE and a pair -> protein index, the fusion's max column (and argmax) is bit
for bit that of ``ops.pair_pool`` on physically replicated residue rows, and the whole ``[max, mean]`` sits within the fp64-twin bound
of the oracle on the replicated batch.  ``screen`` is then checked against the oracle's two-tower model on the expanded batch."""
import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, layer, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_batch, synth_protein
from tests.conftest import assert_twin_parity

pytestmark = pytest.mark.gpu


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


def _ptr(sizes):
    return torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.long)


def _replicated(pro, ps, idx):
    """Residue rows and batch vector of the proteins ``idx`` laid out one copy per pair."""
    off = _ptr(ps)
    rows = torch.cat([pro[off[q]:off[q + 1]] for q in idx])
    return rows, _batch([ps[q] for q in idx])


def _pair_pool_with_argmax(mol, pro, msp, psp):
    """``ops.pair_pool`` and the argmax its node keeps for the backward pass."""
    out = ops.pair_pool(mol.clone().requires_grad_(True), pro.clone().requires_grad_(True), msp, psp)
    arg = next(t for t in out.grad_fn.saved_tensors if t.dtype == torch.int32)
    return out.detach(), arg


@pytest.mark.parametrize("D", [60, 64, 16, 15, 92])
def test_indexed_fusion_equals_the_replicated_call(device, D):
    """Split form (D % 4 == 0, D <= 64: ``k_pair_max_partial<true>`` + ``k_pair_finish<true>``; 1 030 residues wrap the 16 x 64 split
    once) and one-block form (15, 92: ``k_pair_pool_fwd<true>``); ligands of 40 and 33 atoms cross the 32-row LDS tile; protein 3 is never
    referenced, protein 2 three times."""
    torch.manual_seed(D)
    ms, ps, idx = [1, 7, 40, 33, 12], [1, 70, 1030, 9], [2, 0, 2, 1, 2]
    P, Q = len(ms), len(ps)
    mb, pb = _batch(ms), _batch(ps)
    mol, pro = torch.randn(mb.numel(), D), torch.randn(pb.numel(), D)
    pro_rep, pb_rep = _replicated(pro, ps, idx)
    msp, psp = ops.SegmentPtr(mb.to(device), P), ops.SegmentPtr(pb.to(device), Q)
    psp_rep = ops.SegmentPtr(pb_rep.to(device), P)
    m, p = mol.to(device), pro.to(device)
    with torch.no_grad():
        out, arg = ops.pair_pool_indexed(m, p, msp, psp, idx, return_argmax=True)
        out2, arg2 = ops.pair_pool_indexed(m, p, msp, psp, np.asarray(idx), return_argmax=True)
        plain = ops.pair_pool_indexed(m, p, msp, psp, torch.tensor(idx))              # (argmax = NULL in the kernel)
    assert torch.equal(out, out2) and torch.equal(arg, arg2) and torch.equal(out, plain), "two runs differ"
    ref, ref_arg = _pair_pool_with_argmax(m, pro_rep.to(device), msp, psp_rep)
    assert torch.equal(out[:, 0], ref[:, 0]), "max column differs from pair_pool on replicated rows"
    back = ref_arg.cpu().long()
    back[:, 1] += _ptr(ps)[idx] - _ptr([ps[q] for q in idx])[:-1]                      # replicated residue row -> row of the encoding
    assert torch.equal(arg.cpu().long(), back)

    def run(dt):
        return O.dot_and_global_pool(mol.to(dt), pro_rep.to(dt), mb, pb_rep, P, 2), []
    assert_twin_parity(run, out, [], f"pair_pool_indexed D={D}")


@pytest.mark.parametrize("D", [60, 45])
def test_indexed_fusion_identity_default(device, D):
    """``pro_of_pair=None`` with Q == P is ``ops.pair_pool``: max column bit-equal, mean within the same bound.  A one-residue protein."""
    torch.manual_seed(D)
    ms, ps = [20, 7, 33, 1], [300, 1, 70, 129]
    mb, pb, P = _batch(ms), _batch(ps), len(ms)
    mol, pro = torch.randn(mb.numel(), D), torch.randn(pb.numel(), D)
    msp, psp = ops.SegmentPtr(mb.to(device), P), ops.SegmentPtr(pb.to(device), P)
    with torch.no_grad():
        out = ops.pair_pool_indexed(mol.to(device), pro.to(device), msp, psp)
        ref = ops.pair_pool(mol.to(device), pro.to(device), msp, psp)
        via_layer = layer.dot_and_global_pool2_indexed(mol.to(device), pro.to(device), mb.to(device), psp, list(range(P)))
    assert torch.equal(out[:, 0], ref[:, 0]) and torch.equal(out, via_layer)
    assert_twin_parity(lambda dt: (O.dot_and_global_pool(mol.to(dt), pro.to(dt), mb, pb, P, 2), []), out, [], f"identity D={D}")


def test_indexed_fusion_empty_segments(device):
    """An empty ligand or an empty (referenced) protein segment: ``0, 0`` and ``arg = -1``, as ``pair_pool``."""
    torch.manual_seed(0)
    ms, ps, idx = [3, 0, 5], [0, 6], [1, 1, 0]
    mb, pb = _batch(ms), _batch(ps)
    mol, pro = torch.randn(mb.numel(), 60, device=device), torch.randn(pb.numel(), 60, device=device)
    msp, psp = ops.SegmentPtr(mb.to(device), 3), ops.SegmentPtr(pb.to(device), 2)
    with torch.no_grad():
        out, arg = ops.pair_pool_indexed(mol, pro, msp, psp, idx, return_argmax=True)
    assert out[1:].abs().max().item() == 0.0 and (arg[1:] == -1).all() and abs(out[0, 0].item() - (mol[:3] @ pro.T).max().item()) <= 1e-4
    assert 0 <= arg[0, 0].item() < 3 and 0 <= arg[0, 1].item() < 6


@pytest.mark.parametrize("D", [8, 12, 45])
def test_indexed_fusion_ties_route_to_the_first_flattened_pair(device, D):
    """Small-integer rows (every dot product exact), every residue row twice and repeated ligand rows: the maximum occurs several times
    in each pair and ``arg`` is its first flattened occurrence ``a * n_res + b`` — split form (8, 12) and one-block form (45), through a
    swapping index."""
    ms, ps, idx = [4, 3], [5, 6], [1, 0]
    mb, pb, P = _batch(ms), _batch(ps), len(ms)
    g = torch.Generator().manual_seed(D)
    mol = torch.randint(-1, 2, (mb.numel(), D), generator=g).float()
    pro = torch.randint(-1, 2, (pb.numel(), D), generator=g).float()
    mol[3], mol[6] = mol[0], mol[4]
    for a, b in [(1, 0), (3, 2), (4, 0), (6, 5), (8, 7), (10, 9)]:
        pro[a] = pro[b]
    msp, psp = ops.SegmentPtr(mb.to(device), P), ops.SegmentPtr(pb.to(device), P)
    with torch.no_grad():
        out, arg = ops.pair_pool_indexed(mol.to(device), pro.to(device), msp, psp, idx, return_argmax=True)
    m_off, p_off = _ptr(ms), _ptr(ps)
    for i, q in enumerate(idx):
        S = mol[mb == i].double() @ pro[pb == q].double().T
        flat = S.reshape(-1)
        first = int(torch.argmax(flat))
        assert flat[first] == flat.max() and (flat == flat.max()).sum() > 1, "the case must hold a tie"
        assert out[i, 0].item() == flat[first].item()
        assert arg[i].tolist() == [int(m_off[i]) + first // ps[q], int(p_off[q]) + first % ps[q]]
        assert abs(out[i, 1].item() - S.mean().item()) <= 1e-6


def test_indexed_fusion_refusals_come_before_any_launch(device):
    ms, ps = [3, 4, 2], [5, 6]
    mb, pb = _batch(ms), _batch(ps)
    mol, pro = torch.randn(mb.numel(), 60, device=device), torch.randn(pb.numel(), 60, device=device)
    msp, psp = ops.SegmentPtr(mb.to(device), 3), ops.SegmentPtr(pb.to(device), 2)
    with _lib.kernel_timer() as kt, torch.no_grad():
        for bad in ([0, 1, 2], [0, -1, 1], [0, 1], [0, 1, 1, 0], None):            # == Q, negative, wrong lengths, identity with Q != P
            with pytest.raises(IndexError):
                ops.pair_pool_indexed(mol, pro, msp, psp, bad)
        with pytest.raises(GlamHipError, match="read-back"):
            ops.pair_pool_indexed(mol, pro, msp, psp, torch.tensor([0, 1, 1], device=device))
        with torch.enable_grad(), pytest.raises(GlamHipError, match="ops.pair_pool"):
            ops.pair_pool_indexed(mol.clone().requires_grad_(True), pro, msp, psp, [0, 1, 1])
        with torch.enable_grad(), pytest.raises(GlamHipError, match="ops.pair_pool"):
            ops.pair_pool_indexed(mol, pro.clone().requires_grad_(True), msp, psp, [0, 1, 1])
    assert kt.records() == [], "a refusal launched something"
    with torch.enable_grad():                                  # grad mode alone is fine: nothing here requires grad
        assert ops.pair_pool_indexed(mol, pro, msp, psp, [0, 1, 1]).shape == (3, 2)


# ---------------------------------------------------------------------------------------------
# ArchitectureDTI.encode_proteins / screen
# ---------------------------------------------------------------------------------------------
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU")
_IDX = [0, 1, 1, 0, 1, 1]


def _proteins(n, seed=4):
    rng = np.random.default_rng(seed)
    return [synth_protein(rng, 40, 130) for _ in range(n)]


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDTI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **_ACTS, **kw).eval()


def _oracle_run(net, mb, expanded, P, **kw):
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}

    def run(dt):
        sd = {k: v.to(dt) for k, v in sd0.items()}
        cast = lambda b: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
        with torch.no_grad():
            return O.architecture_dti(sd, cast(mb), cast(expanded), P, message_steps=2, **_ACTS, **kw), []
    return run


@pytest.mark.parametrize("mol_block,pro_block,norm,alpha", [("_NNConv", "_GCNConv", "_None", 4), ("_TripletMessage", "_TripletMessage", "_PairNorm", 4),
                                                           ("_NNConv", "_GATConv", "_LayerNorm", 4), ("_NNConv", "_GCNConv", "_None", 1)])
def test_screen_vs_oracle_on_the_expanded_batch(device, monkeypatch, mol_block, pro_block, norm, alpha):
    """``screen(ligands, enc, idx)`` against the oracle's two-tower model on the batch of the proteins ``idx`` collated one per pair
    (forward only), the configurations of ``test_two_tower_model_vs_oracle`` plus an odd width (hid = 15: the one-block fusion on rows
    that flow padded).  And against ``model(ligands, expanded)`` itself: every step's fusion MAX is bit-equal."""
    mb, pros = synth_batch(6, seed=3), _proteins(2)
    expanded = Batch.from_data_list([pros[q] for q in _IDX])
    net = _net(mol_block=mol_block, pro_block=pro_block, graph_norm=norm, hid_dim_alpha=alpha)
    run = _oracle_run(net, mb, expanded, 6, mol_block=mol_block, pro_block=pro_block, graph_norm=norm)
    net = net.to(device)
    net.graphed_call = False
    seen = {"model": [], "screen": []}

    def spy(name, key, first):
        inner = getattr(model, name)

        def f(*a, **k):
            r = inner(*a, **k)
            seen[key].append(first(r).detach().clone())
            return r
        monkeypatch.setattr(model, name, f)
    spy("dot_and_global_pool2", "model", lambda r: r[0])
    spy("dot_and_global_pool2_indexed", "screen", lambda r: r[0])
    mol_dev = mb.to(device)
    with torch.no_grad():
        enc = net.encode_proteins(Batch.from_data_list(pros).to(device))
        out, contacts = net.screen(mol_dev, enc, _IDX, return_argmax=True)
        full = net(mol_dev, expanded.to(device))
    assert enc.num_graphs == 2 and enc.flat.shape == (2, 15 * alpha) and len(enc.rows) == 2
    assert out.shape == (6, 1) and len(contacts) == 2 and all(c.shape == (6, 2) and c.dtype == torch.int32 for c in contacts)
    assert_twin_parity(run, out, [], f"screen {mol_block}/{pro_block}/{norm}/alpha={alpha}")
    assert len(seen["model"]) == len(seen["screen"]) == 2
    for s, (a, b) in enumerate(zip(seen["screen"], seen["model"])):
        assert torch.equal(a[:, 0], b[:, 0]), f"step {s}: the fusion max differs from model(ligands, expanded)"
    assert_twin_parity(run, full, [], "model on the expanded batch")
    # the contacts are rows of the ligand batch / of the encoding, inside the pair's own segments
    lig, res = ops.segment_ptr(mol_dev.batch).ptr.cpu(), enc.sp.ptr.cpu()
    for c in contacts:
        c = c.cpu()
        for i, q in enumerate(_IDX):
            assert lig[i] <= c[i, 0] < lig[i + 1] and res[q] <= c[i, 1] < res[q + 1]


def test_screen_one_protein_default_index(device):
    """Q == 1: ``pro_of_pair`` may be omitted — every ligand against the one encoded protein (the LIT-PCBA walk)."""
    mb, pros = synth_batch(6, seed=3), _proteins(1)
    net = _net()
    run = _oracle_run(net, mb, Batch.from_data_list(pros * 6), 6)
    net = net.to(device)
    with torch.no_grad():
        enc = net.encode_proteins(Batch.from_data_list(pros).to(device))
        out = net.screen(mb.to(device), enc)
        again = net.screen(mb.to(device), enc, [0] * 6)
    assert torch.equal(out, again)
    assert_twin_parity(run, out, [], "screen, one protein")
    with torch.no_grad(), pytest.raises(IndexError, match="pass the index"):
        net.screen(mb.to(device), net.encode_proteins(Batch.from_data_list(_proteins(2)).to(device)))


def test_screen_refuses_what_would_break_the_contract(device):
    mb, pros = synth_batch(6, seed=3).to(device), Batch.from_data_list(_proteins(2)).to(device)
    net, other = _net().to(device), _net().to(device)
    with torch.no_grad():
        enc = net.encode_proteins(pros)
        assert net.screen(mb, enc, _IDX).shape == (6, 1)
        with _lib.kernel_timer() as kt:
            with pytest.raises(GlamHipError, match="another model"):
                other.screen(mb, enc, _IDX)
            net.train()
            with pytest.raises(GlamHipError, match="training mode"):
                net.screen(mb, enc, _IDX)
            with pytest.raises(GlamHipError, match="training mode"):
                net.encode_proteins(pros)
            net.eval()
            ln = _net(flat_norm="_LayerNorm").to(device)
            with pytest.raises(GlamHipError, match="pro_flat's norm _LayerNorm"):
                ln.encode_proteins(pros)
        assert kt.records() == [], "a refusal launched something"
        next(net.pro_conv.parameters()).add_(1)
        with _lib.kernel_timer() as kt, pytest.raises(GlamHipError, match="stale"):
            net.screen(mb, enc, _IDX)
        assert kt.records() == []
        assert net.screen(mb, net.encode_proteins(pros), _IDX).shape == (6, 1)     # a fresh encoding is accepted again
    with pytest.raises(GlamHipError, match="no_grad"):
        net.screen(mb, enc, _IDX)
