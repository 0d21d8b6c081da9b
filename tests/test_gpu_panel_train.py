"""GPU (MI355X): training on a ligand x protein label table — ``glam_pair_pool_panel_bwd`` (csrc/pairpanel_bwd.hip),
``ops.pair_pool_panel_shared`` and ``ArchitectureDTI.forward_panel`` on top of it.

What everything rests on: with every ligand and every protein held ONCE and a selection of proteins, the forward is bit for bit the
screening panel (``ops.pair_pool_panel``), and the gradient of a row — on either side — is the sum of its copies' gradients in the expanded
pair list (ligand ``l`` repeated ``Qs`` times against the proteins ``sel`` tiled ``L`` times), taken in a fixed order by ONE launch, so two
runs agree bit for bit.  ``forward_panel`` is then checked, output and every parameter gradient, against the oracle's two-tower model on
the expanded batch."""
import copy

import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_molecule, synth_protein
from tests import panel_train_restated as R
from tests.conftest import assert_close, assert_twin_parity

pytestmark = pytest.mark.gpu

WIDTHS = [60, 64, 16, 15, 92, 128]          # 16-byte form: 60, 64, 16 (one column chunk), 92, 128 (two); dword form: 15


def _setup(ms, ps, sel, D, device, seed, positive=False):
    torch.manual_seed(seed)
    mol, pro = torch.randn(sum(ms), D), torch.randn(sum(ps), D)
    if positive:
        mol, pro = mol.abs(), pro.abs()
    d_out = torch.randn(len(ms), len(sel), 2)
    psp = ops.SegmentPtr(R.batch_of(ps).to(device), len(ps))
    msp = ops.SegmentPtr(R.batch_of(ms).to(device), len(ms)) if ms else ops.SegmentPtr.from_parts(torch.zeros(1, dtype=torch.int32, device=device), 0, 0)
    return mol, pro, d_out, msp, psp, ops.panel_plan(ps, sel)


def _arg_of(out):
    return next(t for t in out.grad_fn.saved_tensors if t.dtype == torch.int32 and t.dim() == 3)


def _panel(mol, pro, d_out, msp, psp, plan, device):
    """Forward + two backward runs -> ``out``, ``(d_mol, d_pro)``, after what every case checks: the forward is the screening panel's, a
    second backward is the first bit for bit, and a backward is exactly ONE launch of the library."""
    m, p = mol.to(device).requires_grad_(True), pro.to(device).requires_grad_(True)
    out = ops.pair_pool_panel_shared(m, p, msp, psp, plan)
    with torch.no_grad():
        ref, ref_arg = ops.pair_pool_panel(mol.to(device), pro.to(device), msp, psp, plan, return_argmax=True)
    assert torch.equal(out.detach(), ref), "forward differs from pair_pool_panel"
    assert torch.equal(_arg_of(out), ref_arg)
    gs = []
    for _ in range(2):
        with _lib.kernel_timer() as kt:
            gs.append(torch.autograd.grad(out, [m, p], d_out.to(device), retain_graph=True))
        assert [r[0] for r in kt.records()] == ["k_pair_panel_bwd"], "the backward is one launch"
    assert torch.equal(gs[0][0], gs[1][0]) and torch.equal(gs[0][1], gs[1][1]), "a second backward differs from the first"
    return out, gs[0]


def _twin(mol, pro, ms, ps, sel, d_out, extra=None, skip_empty=False):
    return R.twin_on_expanded(O.dot_and_global_pool, mol, pro, ms, ps, sel, d_out, extra, skip_empty)


@pytest.mark.parametrize("D", WIDTHS)
def test_panel_backward_mixed_table(device, D):
    """Ligands of 40 and 33 atoms cross the 32-row sweep of a ligand's two blocks, 1 030 residues wrap the 32 x 16 split of a protein
    twice, protein 2 is named twice (selections 0 and 2), protein 3 never."""
    ms, ps, sel = [1, 7, 40, 33, 12], [1, 70, 1030, 9], [2, 0, 2, 1]
    mol, pro, d_out, msp, psp, plan = _setup(ms, ps, sel, D, device, D)
    out, (dm, dp) = _panel(mol, pro, d_out, msp, psp, plan, device)
    assert dp[sum(ps[:3]):].abs().max().item() == 0.0, "a protein the selection does not name must get exact zeros"
    assert_twin_parity(_twin(mol, pro, ms, ps, sel, d_out), out, [dm, dp], f"pair_pool_panel_shared D={D}", names=["mol", "pro"])


@pytest.mark.parametrize("D", WIDTHS)
def test_panel_backward_colliding_maxima(device, D):
    """Non-negative rows.  One residue row x 50: every ligand's maximum — for both selections of that protein — sits on it, its gradient
    is ten fmaf terms in batch order on top of the common sum.  Separately one ligand row x 50: every column's maximum sits on it."""
    ms, ps, sel = [3, 9, 1, 40, 5], [50, 90], [1, 0, 1]
    mol, pro, d_out, msp, psp, plan = _setup(ms, ps, sel, D, device, 100 + D, positive=True)
    row = 50 + 37
    pro[row] *= 50
    out, (dm, dp) = _panel(mol, pro, d_out, msp, psp, plan, device)
    assert _arg_of(out)[:, 0::2, 1].flatten().tolist() == [row] * 10, "the case must put every maximum of protein 1 on one row"
    run = _twin(mol, pro, ms, ps, sel, d_out)
    assert_twin_parity(run, out, [dm, dp], f"colliding residue row D={D}", names=["mol", "pro"])
    assert_twin_parity(lambda dt: (run(dt)[0], [run(dt)[1][1][row]]), out, [dp[row]], f"colliding residue row D={D}, the row", names=["pro_row"])
    pro[row] /= 50
    a = 3 + 9 + 1 + 21                                    # a row of the 40-atom ligand, in its second 16-row sweep
    mol[a] *= 50
    out, (dm, dp) = _panel(mol, pro, d_out, msp, psp, plan, device)
    assert _arg_of(out)[3, :, 0].tolist() == [a] * 3, "the case must put every column's maximum of ligand 3 on one row"
    run = _twin(mol, pro, ms, ps, sel, d_out)
    assert_twin_parity(run, out, [dm, dp], f"colliding ligand row D={D}", names=["mol", "pro"])
    assert_twin_parity(lambda dt: (run(dt)[0], [run(dt)[1][0][a]]), out, [dm[a]], f"colliding ligand row D={D}, the row", names=["mol_row"])


@pytest.mark.parametrize("D", WIDTHS)
def test_panel_backward_long_lists(device, D):
    """A protein's list of 300 pairs (more than one staged round of addends at every width — 64 pairs a round at D = 128, 256 at 15 and
    16 — and two tiles of hits) and a ligand's list of 70 selections (two rounds at D = 128)."""
    ms, ps, sel = [1 + (i % 3) for i in range(300)], [130], [0]
    mol, pro, d_out, msp, psp, plan = _setup(ms, ps, sel, D, device, 200 + D)
    out, (dm, dp) = _panel(mol, pro, d_out, msp, psp, plan, device)
    assert_twin_parity(_twin(mol, pro, ms, ps, sel, d_out), out, [dm, dp], f"300 ligands on one protein D={D}", names=["mol", "pro"])
    ms, ps, sel = [4, 18, 1, 7, 2], [9, 21, 5], [(5 * j + j // 7) % 3 for j in range(70)]
    mol, pro, d_out, msp, psp, plan = _setup(ms, ps, sel, D, device, 300 + D)
    out, (dm, dp) = _panel(mol, pro, d_out, msp, psp, plan, device)
    assert_twin_parity(_twin(mol, pro, ms, ps, sel, d_out), out, [dm, dp], f"a selection of 70 D={D}", names=["mol", "pro"])


@pytest.mark.parametrize("D", WIDTHS)
def test_panel_backward_empty_segments(device, D):
    """A 0-row ligand and a SELECTED 0-row protein (flag -1: no contribution, the twin runs on the other pairs), then no ligand at all and
    an empty selection (nothing is launched: zeros)."""
    ms, ps, sel = [3, 0, 5], [0, 6, 20], [1, 0, 2, 1]
    mol, pro, d_out, msp, psp, plan = _setup(ms, ps, sel, D, device, 3)
    out, (dm, dp) = _panel(mol, pro, d_out, msp, psp, plan, device)
    arg = _arg_of(out)
    assert out[1].abs().max().item() == 0.0 and out[:, 1].abs().max().item() == 0.0 and (arg[1] == -1).all() and (arg[:, 1] == -1).all()
    assert (arg[0, 0::2] >= 0).all() and torch.isfinite(dm).all() and torch.isfinite(dp).all()
    assert_twin_parity(_twin(mol, pro, ms, ps, sel, d_out, skip_empty=True), out, [dm, dp], f"empty segments D={D}", names=["mol", "pro"])
    for ms, sel in (([], [1, 2]), ([3, 2], [])):
        mol, pro, d_out, msp, psp, plan = _setup(ms, ps, sel, D, device, 4)
        m, p = mol.to(device).requires_grad_(True), pro.to(device).requires_grad_(True)
        out = ops.pair_pool_panel_shared(m, p, msp, psp, plan)
        assert out.shape == (len(ms), len(sel), 2)
        with _lib.kernel_timer() as kt:
            gm, gp = torch.autograd.grad(out, [m, p], d_out.to(device))
        assert kt.records() == [] and gm.shape == m.shape and gp.abs().max().item() == 0.0 and (gm.numel() == 0 or gm.abs().max().item() == 0.0)


@pytest.mark.parametrize("D", WIDTHS)
def test_panel_backward_with_identity(device, D):
    """The two matrices handed back through the node: the gradient of their second use is added INSIDE the one backward launch, for every
    width; gradients of ``fusion + second use`` equal those of the ``with_identity=False`` graph."""
    ms, ps, sel = [5, 40, 2, 9], [70, 300, 4], [1, 0, 1, 1]
    mol, pro, d_out, msp, psp, plan = _setup(ms, ps, sel, D, device, 400 + D)
    wm, wp = torch.randn_like(mol), torch.randn_like(pro)
    extra = lambda m, p: (m * m * wm.to(m)).sum() + (p * p * wp.to(p)).sum()      # noqa: E731
    got = []
    for with_identity in (True, False):
        m, p = mol.to(device).requires_grad_(True), pro.to(device).requires_grad_(True)
        if with_identity:
            out, m2, p2 = ops.pair_pool_panel_shared(m, p, msp, psp, plan, with_identity=True)
            assert m2 is not m and p2 is not p, "both require grad: the add runs inside the launch for every width of the table"
        else:
            out, m2, p2 = ops.pair_pool_panel_shared(m, p, msp, psp, plan), m, p
        loss = (out * d_out.to(device)).sum() + extra(m2, p2)
        for again in (False, True):
            with _lib.kernel_timer() as kt:
                gs2 = torch.autograd.grad(loss, [m, p], retain_graph=True)
            assert [r[0] for r in kt.records()] == ["k_pair_panel_bwd"], "one backward launch per fusion, the add inside it or not"
            assert not again or (torch.equal(gs[0], gs2[0]) and torch.equal(gs[1], gs2[1])), "a second backward differs from the first"
            gs = gs2
        got.append((out, gs))
    with torch.no_grad():
        ref, ref_arg = ops.pair_pool_panel(mol.to(device), pro.to(device), msp, psp, plan, return_argmax=True)
    assert torch.equal(got[0][0].detach(), ref) and torch.equal(_arg_of(got[0][0]), ref_arg), "forward differs from pair_pool_panel"
    run = _twin(mol, pro, ms, ps, sel, d_out, extra)
    for (out, gs), what in zip(got, ("with_identity", "plain")):
        assert_twin_parity(run, out, list(gs), f"{what} D={D}", names=["mol", "pro"])
    assert torch.equal(got[0][0], got[1][0])


# ---------------------------------------------------------------------------------------------
# ArchitectureDTI.forward_panel
# ---------------------------------------------------------------------------------------------
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU")
_SEL = [1, 0, 1]
_L = 6


def _ligands(n, seed=3):
    rng = np.random.default_rng(seed)
    return [synth_molecule(rng) for _ in range(n)]


def _proteins(n, seed=4):
    rng = np.random.default_rng(seed)
    return [synth_protein(rng, 40, 130) for _ in range(n)]


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDTI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **_ACTS, **kw).eval()


@pytest.mark.parametrize("mol_block,pro_block,norm,alpha", [("_NNConv", "_GCNConv", "_None", 4), ("_TripletMessage", "_TripletMessage", "_PairNorm", 4),
                                                           ("_NNConv", "_GATConv", "_LayerNorm", 4), ("_NNConv", "_GCNConv", "_None", 1)])
def test_forward_panel_vs_oracle_on_the_expanded_batch(device, monkeypatch, mol_block, pro_block, norm, alpha):
    """Output and every parameter gradient of ``forward_panel(ligands, proteins, sel)`` against the oracle's two-tower model on the
    expanded batch — ligand ``l`` repeated ``Qs`` times, the proteins ``sel`` tiled ``L`` times (autograd on its state dict) — once in
    ``eval()`` and once in ``train()`` (nothing here is stochastic: the two runs are equal); every step's fusion is bit-equal to the one
    ``screen_panel`` computes from ``encode_proteins``."""
    ligs, pros = _ligands(_L), _proteins(2)
    Qs = len(_SEL)
    big_m = Batch.from_data_list([ligs[l] for l in range(_L) for _ in range(Qs)])
    big_p = Batch.from_data_list([pros[q] for _ in range(_L) for q in _SEL])
    net = _net(mol_block=mol_block, pro_block=pro_block, graph_norm=norm, hid_dim_alpha=alpha)
    names = [n for n, _ in net.named_parameters()]
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    torch.manual_seed(1)
    cot = torch.randn(_L, Qs, 1)

    def run(dt):
        sd = {k: (v.to(dt).requires_grad_(True) if k in names else v.to(dt)) for k, v in sd0.items()}
        cast = lambda b: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
        out = O.architecture_dti(sd, cast(big_m), cast(big_p), _L * Qs, message_steps=2, mol_block=mol_block, pro_block=pro_block,
                                 graph_norm=norm, **_ACTS)
        grads = torch.autograd.grad(out, [sd[n] for n in names], cot.to(dt).view(_L * Qs, 1), allow_unused=True)
        return out.detach().view(_L, Qs, 1), list(grads)

    net = net.to(device)
    net.graphed_call = False
    seen = {"train": [], "screen": []}

    def spy(name, key, pick):
        inner = getattr(model, name)

        def f(*a, **k):
            r = inner(*a, **k)
            seen[key].append(pick(r).detach().clone())
            return r
        monkeypatch.setattr(model, name, f)
    spy("dot_and_global_pool2_panel_shared", "train", lambda r: r[0])
    spy("dot_and_global_pool2_panel", "screen", lambda r: r)
    mol_dev, pro_dev = Batch.from_data_list(ligs).to(device), Batch.from_data_list(pros).to(device)
    results = []
    for training in (False, True):
        net.train(training)
        out = net.forward_panel(mol_dev, pro_dev, _SEL)
        results.append((out.detach(), torch.autograd.grad(out, list(net.parameters()), cot.to(device), allow_unused=True)))
    net.eval()
    with torch.no_grad():
        net.screen_panel(mol_dev, net.encode_proteins(pro_dev), _SEL)
    (out, grads), (out_t, grads_t) = results
    assert out.shape == (_L, Qs, 1) and torch.equal(out, out_t)
    for n, a, b in zip(names, grads, grads_t):
        assert (a is None and b is None) or torch.equal(a, b), f"eval() and train() differ in d_{n}"
    o64, g64 = run(torch.float64)
    for n, a, r in zip(names, grads, g64):
        assert (a is None) == (r is None), f"{n}: a gradient on one side only"
    assert_twin_parity(run, out, list(grads), f"forward_panel {mol_block}/{pro_block}/{norm}/alpha={alpha}", names=names)
    assert len(seen["train"]) == 4 and len(seen["screen"]) == 2
    for s in range(2):
        assert seen["train"][s].shape == (_L, Qs, 2)
        assert torch.equal(seen["train"][s], seen["screen"][s]), f"step {s}: the fusion differs from screen_panel's"
    assert "_glam_panel_plans" in pro_dev.__dict__ and len(pro_dev.__dict__["_glam_panel_plans"]["plans"]) == 1      # read back once, kept


def test_forward_panel_default_stochastic_configuration_trains(device):
    """The reference's defaults (RReLU, Dropout(0.2)) in ``train()``: noise is drawn once per ligand and once per protein — it runs, every
    parameter gets a finite gradient and both towers get one that is not zero."""
    torch.manual_seed(2)
    net = model.ArchitectureDTI().to(device).train()
    ops.manual_seed(4, device)
    mb, pros = Batch.from_data_list(_ligands(_L)).to(device), Batch.from_data_list(_proteins(2)).to(device)
    out = net.forward_panel(mb, pros, _SEL)
    assert out.shape == (_L, 3, 1)
    out.sum().backward()
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    for mod in ("mol_lin0", "mol_conv", "mol_flat", "pro_lin0", "pro_conv", "pro_flat"):
        assert max(p.grad.abs().max().item() for p in getattr(net, mod).parameters()) > 0, f"{mod} got no gradient"


class _PanelStep(torch.nn.Module):
    """What a trainer wraps around ``forward_panel`` for ``GraphedTrainStep`` (which calls ``model(batch)``)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, batch):
        return self.net.forward_panel(batch.mol, batch.pro, batch.proteins, plan=batch.plan)


class _TableBatch:
    def __init__(self, mol, pro, proteins, plan, y):
        self.mol, self.pro, self.proteins, self.plan, self.y = mol, pro, proteins, plan, y


def test_forward_panel_is_captured_by_graphed_train_step(device):
    """Two proteins, 6 ligands per batch, the default training configuration: four visits of two batches under ``GraphedTrainStep`` (eager,
    captured, replayed, replayed) follow the eager trajectory — with a ``PanelPlan`` kept across the steps and with the plan the model
    keeps on the protein batch."""
    from glam_amd.graphs import GraphedTrainStep
    torch.manual_seed(7)
    net0 = model.ArchitectureDTI(e_dim=64, message_steps=2).to(device).train()
    pros = _proteins(2)
    sizes = [int(p.x.size(0)) for p in pros]
    pro = Batch.from_data_list(pros).to(device)
    torch.manual_seed(8)
    batches = [_TableBatch(Batch.from_data_list(_ligands(_L, 21)).to(device), pro, None, ops.panel_plan(sizes, _SEL), torch.randn(_L * 3).to(device)),
               _TableBatch(Batch.from_data_list(_ligands(_L, 22)).to(device), pro, [0, 1], None, torch.randn(_L * 2).to(device))]
    loss_fn = lambda out, b: torch.nn.functional.mse_loss(out.view(-1), b.y.view(-1))      # noqa: E731
    results = []
    for graphed in (False, True):
        step = _PanelStep(copy.deepcopy(net0))
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


def test_forward_panel_refusals_come_before_any_launch(device):
    mb, pros = Batch.from_data_list(_ligands(_L)).to(device), Batch.from_data_list(_proteins(2)).to(device)
    gsn, ln, bn, net = (_net(graph_norm="_GraphSizeNorm").to(device), _net(flat_norm="_LayerNorm").to(device),
                        _net(graph_norm="_BatchNorm").to(device), _net().to(device))
    odd = _net().to(device)
    odd.pro_flat.norm = ln.pro_flat.norm                                          # the protein tower alone
    with _lib.kernel_timer() as kt:
        with pytest.raises(GlamHipError, match="forward_panel: mol_conv's norm _GraphSizeNorm"):
            gsn.forward_panel(mb, pros, _SEL)
        with pytest.raises(GlamHipError, match="forward_panel: mol_flat's norm _LayerNorm"):
            ln.forward_panel(mb, pros, _SEL)
        with pytest.raises(GlamHipError, match="forward_panel: pro_flat's norm _LayerNorm"):
            odd.forward_panel(mb, pros, _SEL)
        with pytest.raises(GlamHipError, match="forward_panel: mol_conv's norm _BatchNorm"):
            bn.train().forward_panel(mb, pros, _SEL)
        with pytest.raises(GlamHipError, match="the plan was made for 3 proteins"):
            net.forward_panel(mb, pros, plan=ops.panel_plan([40, 50, 60]))
        with pytest.raises(GlamHipError, match="the plan was made for 2 proteins of 8 residue rows"):
            net.forward_panel(mb, pros, plan=ops.panel_plan([4, 4]))
        with pytest.raises(GlamHipError, match="not both"):
            net.forward_panel(mb, pros, _SEL, plan=ops.panel_plan([4, 4]))
    assert kt.records() == [], "a refusal must come before the first launch"
    with pytest.raises(IndexError, match=r"proteins must lie in \[0, 2\)"):
        net.forward_panel(mb, pros, [0, 2])
    with pytest.raises(GlamHipError, match="pair_pool_panel is inference only"):
        ops.pair_pool_panel(torch.randn(4, 8, device=device, requires_grad=True), torch.randn(6, 8, device=device),
                            ops.SegmentPtr(R.batch_of([4]).to(device), 1), ops.SegmentPtr(R.batch_of([6]).to(device), 1), ops.panel_plan([6]))
    with torch.no_grad():
        assert bn.eval().forward_panel(mb, pros, _SEL).shape == (_L, 3, 1)        # running statistics are per row
