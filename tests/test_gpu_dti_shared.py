"""GPU (MI355X): training against proteins that are held once — ``glam_pair_pool_shared_fwd`` / ``_bwd`` and ``glam_pair_rows_bwd``
(csrc/pairshared.hip), ``ops.pair_pool_shared`` / ``ops.pair_rows`` and ``ArchitectureDTI.forward_shared`` on top of them.

What everything rests on: with each protein held ONCE and a pair -> protein index, the forward is bit for bit the screening fusion
(``ops.pair_pool_indexed``), the ligand gradient is that of ``ops.pair_pool`` on physically replicated residue rows, and the gradient of
a protein's residue rows is the sum of its copies' gradients in the replicated batch — taken in a fixed order, so two runs agree bit for
bit.  ``forward_shared`` is then checked, output and every parameter gradient, against the oracle's two-tower model on the expanded batch."""
import copy

import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_batch, synth_protein
from tests.conftest import assert_close, assert_twin_parity

pytestmark = pytest.mark.gpu


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


def _ptr(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def _replicated(pro, ps, idx):
    off = _ptr(ps)
    return torch.cat([pro[off[q]:off[q + 1]] for q in idx]), _batch([ps[q] for q in idx])


def _oracle_on_replicated(mol, pro, ms, ps, idx, d_out, extra=None):
    """``run(dtype)`` for ``assert_twin_parity``: the oracle's fusion on the replicated batch under autograd -> out, [d_mol, d_pro] with
    the copies' residue gradients summed per protein.  ``extra(mol, pro) -> scalar``: a second use of the two matrices (held once)."""
    mb = _batch(ms)
    off, rep_off = _ptr(ps), _ptr([ps[q] for q in idx])

    def run(dt):
        m, p = mol.to(dt).requires_grad_(True), pro.to(dt).requires_grad_(True)
        rows, pb_rep = _replicated(p, ps, idx)
        o = O.dot_and_global_pool(m, rows, mb, pb_rep, len(ms), 2)
        loss = (o * d_out.to(dt)).sum()
        if extra is not None:
            loss = loss + extra(m, p)
        gm, gp = torch.autograd.grad(loss, [m, p])
        assert rep_off[-1] == rows.size(0) and off[-1] == p.size(0)
        return o.detach(), [gm, gp]
    return run


def _arg_of(out):
    return next(t for t in out.grad_fn.saved_tensors if t.dtype == torch.int32 and t.dim() == 2)


def _setup(ms, ps, D, device, seed, positive=False):
    torch.manual_seed(seed)
    mb, pb = _batch(ms), _batch(ps)
    mol, pro = torch.randn(mb.numel(), D), torch.randn(pb.numel(), D)
    if positive:
        mol, pro = mol.abs(), pro.abs()
    d_out = torch.randn(len(ms), 2)
    msp, psp = ops.SegmentPtr(mb.to(device), len(ms)), ops.SegmentPtr(pb.to(device), len(ps))
    return mol, pro, d_out, msp, psp


def _shared_grads(mol, pro, d_out, msp, psp, idx, device, runs=2):
    m, p = mol.to(device).requires_grad_(True), pro.to(device).requires_grad_(True)
    out = ops.pair_pool_shared(m, p, msp, psp, idx)
    gs = [torch.autograd.grad(out, [m, p], d_out.to(device), retain_graph=True) for _ in range(runs)]
    return out, gs


@pytest.mark.parametrize("D", [60, 64, 16, 15, 92])
def test_shared_fusion_against_the_replicated_call(device, D):
    """Vector form (60, 64, 16) and general form (15, 92); ligands of 40 and 33 atoms cross the 32-row tile, 1 030 residues wrap the
    32 x 16 residue split twice, protein 2 is referenced three times (pairs 0, 2, 4), protein 3 never."""
    ms, ps, idx = [1, 7, 40, 33, 12], [1, 70, 1030, 9], [2, 0, 2, 1, 2]
    mol, pro, d_out, msp, psp = _setup(ms, ps, D, device, D)
    out, ((dm, dp), (dm2, dp2)) = _shared_grads(mol, pro, d_out, msp, psp, idx, device)
    with torch.no_grad():
        ref, ref_arg = ops.pair_pool_indexed(mol.to(device), pro.to(device), msp, psp, idx, return_argmax=True)
    assert torch.equal(out.detach(), ref), "forward differs from pair_pool_indexed"
    assert torch.equal(_arg_of(out), ref_arg)
    assert torch.equal(dm, dm2) and torch.equal(dp, dp2), "a second backward differs from the first"
    # the ligand gradient: ops.pair_pool on physically replicated residue rows
    rows, pb_rep = _replicated(pro, ps, idx)
    m_r, p_r = mol.to(device).requires_grad_(True), rows.to(device).requires_grad_(True)
    out_r = ops.pair_pool(m_r, p_r, msp, ops.SegmentPtr(pb_rep.to(device), len(ms)))
    dm_r, _ = torch.autograd.grad(out_r, [m_r, p_r], d_out.to(device))
    if D in (60, 64, 16):
        assert torch.equal(dm, dm_r), "d_mol differs from pair_pool on replicated rows"
    off = _ptr(ps)
    assert dp[off[3]:off[4]].abs().max().item() == 0.0, "an unreferenced protein must get zeros"
    assert_twin_parity(_oracle_on_replicated(mol, pro, ms, ps, idx, d_out), out, [dm, dp], f"pair_pool_shared D={D}", names=["mol", "pro"])


@pytest.mark.parametrize("D", [60, 15])
def test_shared_fusion_colliding_maxima(device, D):
    """Non-negative rows and one residue row of the shared protein scaled by 50: all five pairs have their maximum on THAT row, whose
    gradient is five fmaf terms in batch order on top of the common sum."""
    ms, ps, idx = [3, 9, 1, 40, 5], [50, 90], [1, 1, 1, 1, 1]
    mol, pro, d_out, msp, psp = _setup(ms, ps, D, device, 100 + D, positive=True)
    row = 50 + 37
    pro[row] *= 50
    out, ((dm, dp), (dm2, dp2)) = _shared_grads(mol, pro, d_out, msp, psp, idx, device)
    assert _arg_of(out)[:, 1].tolist() == [row] * 5, "the case must put every pair's maximum on one row"
    assert torch.equal(dp, dp2) and torch.equal(dm, dm2)
    run = _oracle_on_replicated(mol, pro, ms, ps, idx, d_out)
    assert_twin_parity(run, out, [dm, dp], f"colliding maxima D={D}", names=["mol", "pro"])
    assert_twin_parity(lambda dt: (run(dt)[0], [run(dt)[1][1][row]]), out, [dp[row]], f"colliding maxima D={D}, the row", names=["pro_row"])
    assert dp[:50].abs().max().item() == 0.0


@pytest.mark.parametrize("D", [60, 92])
def test_shared_fusion_many_pairs_on_one_protein(device, D):
    """70 ligands of 1-3 atoms on one 130-residue protein (``pro_of_pair=None``): the pair list is longer than a staged tile of 64."""
    ms, ps = [1 + (i % 3) for i in range(70)], [130]
    mol, pro, d_out, msp, psp = _setup(ms, ps, D, device, 200 + D)
    out, ((dm, dp), (dm2, dp2)) = _shared_grads(mol, pro, d_out, msp, psp, None, device)
    assert torch.equal(dp, dp2) and torch.equal(dm, dm2)
    assert_twin_parity(_oracle_on_replicated(mol, pro, ms, ps, [0] * 70, d_out), out, [dm, dp], f"many pairs D={D}", names=["mol", "pro"])


@pytest.mark.parametrize("D", [60, 15])
def test_shared_fusion_empty_segments(device, D):
    ms, ps, idx = [3, 0, 5], [0, 6], [1, 1, 0]
    mol, pro, d_out, msp, psp = _setup(ms, ps, D, device, 3)
    out, ((dm, dp), _) = _shared_grads(mol, pro, d_out, msp, psp, idx, device)
    arg = _arg_of(out)
    assert out[1:].abs().max().item() == 0.0 and (arg[1:] == -1).all() and (arg[0] >= 0).all()
    assert torch.isfinite(dm).all() and torch.isfinite(dp).all()
    assert dm[3:].abs().max().item() == 0.0, "the ligand of an empty pair gets a zero gradient"
    assert dm[:3].abs().max().item() > 0 and dp.abs().max().item() > 0


@pytest.mark.parametrize("D", [60, 92])
def test_shared_fusion_with_identity(device, D):
    """The two matrices handed back through the node (60: their later gradient is added inside the backward launch; 92: the plain
    triple, autograd adds): gradients of ``fusion + second use`` equal those of the ``with_identity=False`` graph."""
    ms, ps, idx = [5, 40, 2, 9], [70, 300, 4], [1, 0, 1, 1]
    mol, pro, d_out, msp, psp = _setup(ms, ps, D, device, 300 + D)
    wm, wp = torch.randn_like(mol), torch.randn_like(pro)
    extra = lambda m, p: (m * m * wm.to(m)).sum() + (p * p * wp.to(p)).sum()      # noqa: E731
    got = []
    for with_identity in (True, False):
        m, p = mol.to(device).requires_grad_(True), pro.to(device).requires_grad_(True)
        if with_identity:
            out, m2, p2 = ops.pair_pool_shared(m, p, msp, psp, idx, with_identity=True)
            assert (m2 is not m) == (D == 60), "the fused add applies where glam_pair_pool_add_supported(D)"
        else:
            out, m2, p2 = ops.pair_pool_shared(m, p, msp, psp, idx), m, p
        got.append((out, torch.autograd.grad((out * d_out.to(device)).sum() + extra(m2, p2), [m, p])))
    run = _oracle_on_replicated(mol, pro, ms, ps, idx, d_out, extra)
    for (out, gs), what in zip(got, ("with_identity", "plain")):
        assert_twin_parity(run, out, list(gs), f"{what} D={D}", names=["mol", "pro"])
    assert torch.equal(got[0][0], got[1][0])


def test_pair_rows_backward_is_an_ordered_index_add(device):
    torch.manual_seed(9)
    P, Q, W = 150, 4, 101                       # (101 columns: two column chunks; 150 pairs: three staged tiles; protein 3 unreferenced)
    idx = torch.randint(0, 3, (P,))
    flat, d_rows = torch.randn(Q, W), torch.randn(P, W)
    index = ops.pair_index(idx, P, Q)
    f = flat.to(device).requires_grad_(True)
    rows = ops.pair_rows(f, index)
    assert torch.equal(rows.detach().cpu(), flat[idx])
    g1, = torch.autograd.grad(rows, f, d_rows.to(device), retain_graph=True)
    g2, = torch.autograd.grad(rows, f, d_rows.to(device))
    assert torch.equal(g1, g2) and g1[3].abs().max().item() == 0.0
    run = lambda dt: (flat[idx].to(dt), [torch.zeros(Q, W, dtype=dt).index_add_(0, idx, d_rows.to(dt))])      # noqa: E731
    assert_twin_parity(run, rows, [g1], "pair_rows", names=["flat"])
    with pytest.raises(IndexError):
        ops.pair_rows(torch.randn(3, W, device=device), index)


# ---------------------------------------------------------------------------------------------
# ArchitectureDTI.forward_shared
# ---------------------------------------------------------------------------------------------
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU")
_IDX = [0, 1, 1, 0, 1, 1]


def _proteins(n, seed=4):
    rng = np.random.default_rng(seed)
    return [synth_protein(rng, 40, 130) for _ in range(n)]


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDTI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **_ACTS, **kw).eval()


@pytest.mark.parametrize("mol_block,pro_block,norm,alpha", [("_NNConv", "_GCNConv", "_None", 4), ("_TripletMessage", "_TripletMessage", "_PairNorm", 4),
                                                           ("_NNConv", "_GATConv", "_LayerNorm", 4), ("_NNConv", "_GCNConv", "_None", 1)])
def test_forward_shared_vs_oracle_on_the_expanded_batch(device, monkeypatch, mol_block, pro_block, norm, alpha):
    """Output and every parameter gradient of ``forward_shared(ligands, proteins, idx)`` against the oracle's two-tower model on the batch
    of the proteins ``idx`` collated one per pair (autograd on its state dict), once in ``eval()`` and once in ``train()`` (nothing here is
    stochastic: the two runs are equal); every step's fusion maximum is bit-equal to that of ``model(ligands, expanded)``."""
    mb, pros = synth_batch(6, seed=3), _proteins(2)
    expanded = Batch.from_data_list([pros[q] for q in _IDX])
    net = _net(mol_block=mol_block, pro_block=pro_block, graph_norm=norm, hid_dim_alpha=alpha)
    names = [n for n, _ in net.named_parameters()]
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    torch.manual_seed(1)
    cot = torch.randn(6, 1)

    def run(dt):
        sd = {k: (v.to(dt).requires_grad_(True) if k in names else v.to(dt)) for k, v in sd0.items()}
        cast = lambda b: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
        out = O.architecture_dti(sd, cast(mb), cast(expanded), 6, message_steps=2, mol_block=mol_block, pro_block=pro_block,
                                 graph_norm=norm, **_ACTS)
        return out.detach(), list(torch.autograd.grad(out, [sd[n] for n in names], cot.to(dt), allow_unused=True))

    net = net.to(device)
    net.graphed_call = False
    seen = {"model": [], "shared": []}

    def spy(name, key):
        inner = getattr(model, name)

        def f(*a, **k):
            r = inner(*a, **k)
            seen[key].append(r[0].detach().clone())
            return r
        monkeypatch.setattr(model, name, f)
    spy("dot_and_global_pool2", "model")
    spy("dot_and_global_pool2_shared", "shared")
    mol_dev, pro_dev = mb.to(device), Batch.from_data_list(pros).to(device)
    results = []
    for training in (False, True):
        net.train(training)
        out = net.forward_shared(mol_dev, pro_dev, _IDX)
        results.append((out.detach(), torch.autograd.grad(out, list(net.parameters()), cot.to(device), allow_unused=True)))
    net.eval()
    with torch.no_grad():
        net(mol_dev, expanded.to(device))
    (out, grads), (out_t, grads_t) = results
    assert out.shape == (6, 1) and torch.equal(out, out_t)
    for n, a, b in zip(names, grads, grads_t):
        assert (a is None and b is None) or torch.equal(a, b), f"eval() and train() differ in d_{n}"
    o64, g64 = run(torch.float64)
    for n, a, r in zip(names, grads, g64):
        assert (a is None) == (r is None), f"{n}: a gradient on one side only"
    assert_twin_parity(run, out, list(grads), f"forward_shared {mol_block}/{pro_block}/{norm}/alpha={alpha}", names=names)
    assert len(seen["shared"]) == 4 and len(seen["model"]) == 2
    for s in range(2):
        assert torch.equal(seen["shared"][s][:, 0], seen["model"][s][:, 0]), f"step {s}: the fusion max differs from model(ligands, expanded)"


def test_forward_shared_default_stochastic_configuration_trains(device):
    """The reference's defaults (RReLU, Dropout(0.2)) in ``train()``: noise is drawn once per distinct protein — it runs, every parameter
    gets a finite gradient and the protein tower gets one that is not zero."""
    torch.manual_seed(2)
    net = model.ArchitectureDTI().to(device).train()
    ops.manual_seed(4, device)
    mb, pros = synth_batch(6, seed=3).to(device), Batch.from_data_list(_proteins(1)).to(device)
    out = net.forward_shared(mb, pros)
    assert out.shape == (6, 1)
    out.sum().backward()
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    for mod in ("pro_lin0", "pro_conv", "pro_flat"):
        assert max(p.grad.abs().max().item() for p in getattr(net, mod).parameters()) > 0, f"{mod} got no gradient"


class _SharedStep(torch.nn.Module):
    """What a trainer wraps around ``forward_shared`` for ``GraphedTrainStep`` (which calls ``model(batch)``)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, batch):
        return self.net.forward_shared(batch.mol, batch.pro, batch.index)


class _PairBatch:
    def __init__(self, mol, pro, index):
        self.mol, self.pro, self.index, self.y = mol, pro, index, mol.y


def test_forward_shared_is_captured_by_graphed_train_step(device):
    """One protein, 6 ligands per batch, the default training configuration: four visits of two batches under ``GraphedTrainStep`` (eager,
    captured, replayed, replayed) follow the eager trajectory — with a ``PairIndex`` kept across the steps and with the default index the
    model keeps."""
    from glam_amd.graphs import GraphedTrainStep
    torch.manual_seed(7)
    net0 = model.ArchitectureDTI(e_dim=64, message_steps=2).to(device).train()
    pro = Batch.from_data_list(_proteins(1)).to(device)
    batches = [_PairBatch(synth_batch(6, seed=21).to(device), pro, ops.pair_index([0] * 6, 6, 1)),
               _PairBatch(synth_batch(6, seed=22).to(device), pro, None)]
    loss_fn = lambda out, b: torch.nn.functional.mse_loss(out.view(-1), b.y.view(-1))      # noqa: E731
    results = []
    for graphed in (False, True):
        step = _SharedStep(copy.deepcopy(net0))
        opt = torch.optim.Adam(step.parameters(), lr=1e-3, capturable=True)
        stepper = GraphedTrainStep(step, opt, loss_fn)
        ops.manual_seed(5, device)
        losses = []
        for _visit in range(4):
            for b in batches:
                if graphed:
                    losses.append(float(stepper(b)))
                else:
                    opt.zero_grad(set_to_none=True)
                    loss = loss_fn(step(b), b)
                    loss.backward()
                    opt.step()
                    losses.append(float(loss.detach()))
        if graphed:
            assert stepper.graphs() == 2
        results.append((losses, [p.detach().clone() for p in step.parameters()]))
    (l_e, p_e), (l_g, p_g) = results
    assert np.allclose(l_e, l_g, rtol=1e-5, atol=1e-6), (l_e, l_g)
    for a, r in zip(p_g, p_e):
        assert_close(a, r, 1e-5, "parameter")


def test_forward_shared_refusals_come_before_any_launch(device):
    mb, pros = synth_batch(6, seed=3).to(device), Batch.from_data_list(_proteins(2)).to(device)
    gsn, ln, bn, net = (_net(graph_norm="_GraphSizeNorm").to(device), _net(flat_norm="_LayerNorm").to(device),
                        _net(graph_norm="_BatchNorm").to(device), _net().to(device))
    with _lib.kernel_timer() as kt:
        with pytest.raises(GlamHipError, match="pro_conv's norm _GraphSizeNorm"):
            gsn.forward_shared(mb, pros, _IDX)
        with pytest.raises(GlamHipError, match="pro_flat's norm _LayerNorm"):
            ln.forward_shared(mb, pros, _IDX)
        with pytest.raises(GlamHipError, match="pro_conv's norm _BatchNorm"):
            bn.train().forward_shared(mb, pros, _IDX)
        for bad in ([0, 1, 1], [0, 1, 1, 0, 1, 1, 0], [0, 1, 2, 0, 1, 1], None):      # wrong lengths, out of range, identity with Q != P
            with pytest.raises(IndexError):
                net.forward_shared(mb, pros, bad)
        with pytest.raises(GlamHipError, match="read-back"):
            net.forward_shared(mb, pros, torch.tensor(_IDX, device=device))
    assert kt.records() == [], "a refusal launched something"
    with torch.no_grad():
        assert bn.eval().forward_shared(mb, pros, _IDX).shape == (6, 1)            # running statistics are per row: accepted
        assert net.forward_shared(mb, pros, _IDX).shape == (6, 1)
