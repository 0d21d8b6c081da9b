"""GPU (MI355X): refillable pair lists — ``glam_pair_list_load`` (csrc/pairlist.hip) against its numpy restatement, bit for bit, over the
cases of ``tests/pair_list_restated.py`` and through ``ops.PairList`` / ``data.ResidentPairs``; the shared pair ops on a refilled list
against the same list held on the host; and shuffled DTI / DDI training through ONE captured step (``GraphedTrainStep(SharedStep(net))``)
against eager ``forward_shared`` on host indices, within the padded batches' bound: 4 x the eager path's own sensitivity to the order of
the pairs (``d_perm``, measured live per quantity), floor 2^-20."""
import copy
import types

import numpy as np
import pytest
import torch

from glam_amd import _lib, data, graphs, model, ops, optim
from glam_amd.data import Batch, Data, DeviceDataset, synth_molecule, synth_protein
from tests.pair_list_restated import cases, labels_restated, pair_list_restated

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20          # 8 ulp of the largest magnitude (tests/test_gpu_padded.py)
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")
_CASES = cases()
LOAD, COLLATE = "k_pair_list_load", "k_collate_padded"


def _same(got, want, what):
    want = torch.as_tensor(np.ascontiguousarray(want)).to(got.device)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    assert torch.equal(got, want), f"{what}: differs at {int((got != want).reshape(-1).nonzero()[0])}"


def _dev(a, device, dtype=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(device)


def _names(kt):
    return [name for name, _grid, _us in kt.records()]


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel against numpy
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _CASES, ids=[c["name"] for c in _CASES])
def test_kernel_equals_its_restatement_on_every_output(device, case):
    """The entry point itself, with pair ids and padding: one object per case, filled with a marker, then loaded with every id vector of
    the case in turn — every output word is rewritten each time."""
    P, B, Q, pad = case["P"], case["B"], case["Q"], case["pad"]
    lst = ops.PairList(P, Q, device, pad=pad)
    col, y = _dev(case["col"], device), _dev(case["y"], device, torch.float32)
    y_out = torch.full((B, 3), float("nan"), device=device)
    lst._arena.fill_(-7)
    for k, ids in enumerate(case["loads"]):
        with _lib.kernel_timer() as kt:
            ops.pair_list_launch(_dev(ids, device), lst, col, None, None, B, y, y_out)
        assert _names(kt) == [LOAD]
        idx, order, ptr = pair_list_restated(ids, case["col"], B, P, Q, pad)
        _same(lst.idx, idx, f"load {k} idx")
        _same(lst.order, order, f"load {k} order")
        _same(lst.ptr, ptr, f"load {k} ptr")
        _same(y_out, labels_restated(ids, case["y"], B), f"load {k} y_out")
        _same(lst.order, np.argsort(idx, kind="stable").astype(np.int32), f"load {k} order against numpy")
        _same(lst.ptr, np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=Q))]).astype(np.int32), f"load {k} ptr against numpy")
    # ids = NULL: the identity over the column's first B entries, as side b, without labels
    B0 = min(B, case["col"].shape[0])
    ops.pair_list_launch(None, None, None, lst, col, B0)
    idx, order, ptr = pair_list_restated(None, case["col"], B0, P, Q, pad)
    _same(lst.idx, idx, "identity idx"), _same(lst.order, order, "identity order"), _same(lst.ptr, ptr, "identity ptr")


def test_pair_list_load_is_one_launch_and_leaves_no_residue(device):
    P, Q = 130, 700
    lst = ops.PairList(P, Q, device, pad=3)
    _same(lst.idx, np.full(P, 3, dtype=np.int32), "a fresh list points at its padding segment")
    g = np.random.default_rng(2)
    for k, n in enumerate((130, 100, 0, 64, 65)):
        index = g.integers(0, Q, n)
        if k % 2:                                              # the upload alone, then the hook
            with _lib.kernel_timer() as kt:
                lst.load(index, launch=False)
            assert _names(kt) == [], f"load {k}: launch=False"
            with _lib.kernel_timer() as kt:
                lst.glam_reload()
        else:
            with _lib.kernel_timer() as kt:
                lst.load(index)
                lst.glam_reload()                              # outside a capture a launched load is not repeated
        assert _names(kt) == [LOAD], f"load {k}"
        full = np.concatenate([index, np.full(P - n, 3)]).astype(np.int32)
        by = ops.PairsByProtein(full, Q)
        _same(lst.on(device), full, f"load {k} idx")
        order, ptr = lst.by_protein().on(device)
        _same(order, by.order, f"load {k} order"), _same(ptr, by.ptr, f"load {k} ptr")
        assert order.data_ptr() == lst.order.data_ptr() and lst.on(device).data_ptr() == lst.idx.data_ptr()
    with _lib.kernel_timer() as kt:
        for bad in ([0, Q], [-1], [0.5], [0] * (P + 1)):
            with pytest.raises(IndexError):
                lst.load(bad)
        with pytest.raises(_lib.GlamHipError, match="lives on a device"):
            lst.load(torch.zeros(3, dtype=torch.int64, device=device))
    assert _names(kt) == [], "a refused load launches nothing"
    _same(lst.idx, full, "a refused load leaves the list as it was")
    with pytest.raises(_lib.GlamHipError, match="this PairList lives on"):
        lst.on("cpu")


# ------------------------------------------------------------------------------------------------------------------------------------
# the batch objects: tables, launches, labels
# ------------------------------------------------------------------------------------------------------------------------------------
def _drugs(n, seed):
    rng = np.random.default_rng(seed)
    return [synth_molecule(rng) for _ in range(n)]


@pytest.mark.parametrize("r", [1, 3])
def test_ddi_batch_loads_both_sides_and_the_labels_in_one_launch(device, r):
    """Different Q per side; label rows of 4 and of 12 bytes (not 16-byte aligned)."""
    g = np.random.default_rng(7 + r)
    Np, B, Q1, Q2 = 90, 16, 5, 9
    first, second = g.integers(0, Q1, Np), g.integers(0, Q2, Np)
    y = g.standard_normal((Np, r)).astype(np.float32)
    pairs = data.ResidentPairs(first, second, y, device)
    d1, d2 = Batch.from_data_list(_drugs(Q1, 1)).to(device), Batch.from_data_list(_drugs(Q2, 2)).to(device)
    batch = pairs.ddi_batch(d1, d2, batch_size=B)
    assert (batch.first.P, batch.first.Q, batch.second.P, batch.second.Q) == (B, Q1, B, Q2) and batch.num_real_graphs == B
    assert batch.mol1 is d1 and batch.mol2 is d2
    assert data.ResidentPairs(first, first, y, device).ddi_batch(d1, batch_size=B).mol2 is d1            # one Batch serves both towers
    with pytest.raises(IndexError, match="second column names drugs up to 8, but only 5"):
        pairs.ddi_batch(d1, batch_size=B)

    def check(ids, what):
        for lst, col in ((batch.first, first), (batch.second, second)):
            by = ops.PairsByProtein(col[ids].astype(np.int32), lst.Q)
            _same(lst.idx, col[ids].astype(np.int32), f"{what} idx")
            _same(lst.order, by.order, f"{what} order"), _same(lst.ptr, by.ptr, f"{what} ptr")
        _same(batch.y, y[ids], f"{what} y")

    lists = [g.permutation(Np)[:B], g.integers(0, 10, B), g.permutation(Np)[:B]]            # (the second: repeated pair ids)
    for k, ids in enumerate(lists):
        with _lib.kernel_timer() as kt:
            batch.load(ids)
        assert _names(kt) == [LOAD]
        check(ids, f"load {k}")
    assert batch.load_many(lists) == 3
    for k in (2, 0, 1):
        with _lib.kernel_timer() as kt:
            batch.load(step=k)
        assert _names(kt) == [LOAD]
        check(lists[k], f"step {k}")
    with _lib.kernel_timer() as kt:
        batch.load(lists[0], launch=False)
    assert _names(kt) == []
    check(lists[1], "an upload alone changes nothing")
    with _lib.kernel_timer() as kt:
        batch.glam_reload()
    assert _names(kt) == [LOAD]
    check(lists[0], "the reload hook")
    with _lib.kernel_timer() as kt:
        for bad, err in ((lists[0][:-1], ValueError), (np.r_[lists[0][:-1], Np], IndexError), (lists[0].astype(np.float64), IndexError),
                         (torch.as_tensor(lists[0]).to(device), _lib.GlamHipError)):
            with pytest.raises(err):
                batch.load(bad)
        with pytest.raises(IndexError):
            batch.load(step=3)
    assert _names(kt) == [], "a refused load launches nothing"
    check(lists[0], "a refused load leaves the batch as it was")


class _World:
    """40 synthetic ligands without labels, 3 synthetic proteins of 30-70 residues, 120 labelled pairs."""

    def __init__(self, device):
        rng = np.random.default_rng(31)
        self.ligs = [Data(m.x, m.edge_index, m.edge_attr) for m in (synth_molecule(rng) for _ in range(40))]
        self.first, self.second = rng.integers(0, 40, 120), rng.integers(0, 3, 120)
        self.y = rng.standard_normal((120, 1)).astype(np.float32)
        self.dd = DeviceDataset(self.ligs, device)
        self.pro = Batch.from_data_list([synth_protein(rng, 30, 70) for _ in range(3)]).to(device)
        self.pairs = data.ResidentPairs(self.first, self.second, self.y, device)
        self.y_dev = torch.from_numpy(self.y).to(device)
        self.device = device


_WORLD = {}


def _world(device):
    if device not in _WORLD:
        _WORLD[device] = _World(device)
    return _WORLD[device]


@pytest.mark.parametrize("split", [False, True], ids=["one phantom graph", "phantom_rows"])
def test_dti_batch_is_the_padded_collate_then_the_pair_list(device, split):
    w = _world(device)
    B = 8
    batch = w.pairs.dti_batch(w.dd, w.pro, B, phantom_rows=int(w.dd.ns.max()) if split else None)
    K = batch.mol.num_phantom_graphs
    assert batch.num_graphs == B + K == batch.mol.num_graphs == batch.index.P and batch.num_real_graphs == B and batch.index.Q == 3
    assert batch.pro is w.pro and batch.y.shape == (B, 1)
    g = np.random.default_rng(3)
    lists = [g.permutation(120)[:B] for _ in range(3)]

    def check(ids, what):
        lig = w.first[ids]
        ref = w.dd.collate(lig)
        N, E = ref.x.size(0), ref.edge_index.size(1)
        assert torch.equal(batch.mol.x[:N], ref.x) and torch.equal(batch.mol.edge_index[:, :E], ref.edge_index), f"{what}: the ligands"
        assert bool((batch.mol.x[N:] == 0).all())
        idx = np.concatenate([w.second[ids], np.zeros(K, dtype=np.int64)]).astype(np.int32)
        by = ops.PairsByProtein(idx, 3)
        _same(batch.index.idx, idx, f"{what} idx"), _same(batch.index.order, by.order, f"{what} order"), _same(batch.index.ptr, by.ptr, f"{what} ptr")
        _same(batch.y, w.y[ids], f"{what} y")

    for k, ids in enumerate(lists):
        with _lib.kernel_timer() as kt:
            batch.load(ids)
        names = _names(kt)
        assert len(names) == 2 and names[0].startswith(COLLATE) and names[1] == LOAD, names
        check(ids, f"load {k}")
    assert batch.load_many(lists) == 3
    for k in (1, 2, 0):
        batch.load(step=k)
        check(lists[k], f"step {k}")
    with _lib.kernel_timer() as kt:
        for bad, err in ((lists[0][:-1], ValueError), (np.r_[lists[0][:-1], 120], IndexError), (lists[0] + 0.5, IndexError),
                         (torch.as_tensor(lists[0]).to(device), _lib.GlamHipError)):
            with pytest.raises(err):
                batch.load(bad)
    assert _names(kt) == [], "a refused load launches nothing"
    check(lists[0], "a refused load leaves the batch as it was")


# ------------------------------------------------------------------------------------------------------------------------------------
# the pair ops on a refilled list: the bits of the same list held on the host
# ------------------------------------------------------------------------------------------------------------------------------------
def _segments(sizes, D, device, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(int(sum(sizes)), D, generator=g).to(device)
    bvec = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(device)
    return x, ops.segment_ptr(bvec, len(sizes))


@pytest.mark.parametrize("D", [60, 15])
def test_ops_on_a_refilled_list_equal_the_host_index_bit_for_bit(device, D):
    pro_sizes, P = [1, 7, 40, 70, 7, 1], 24
    g = np.random.default_rng(11 + D)
    mol_sizes = g.integers(3, 10, P).tolist()
    mol, msp = _segments(mol_sizes, D, device, 1)
    pro, psp = _segments(pro_sizes, D, device, 2)
    Q = len(pro_sizes)
    flat = torch.randn(Q, 2 * D, generator=torch.Generator().manual_seed(3)).to(device)
    w = torch.randn(P, 2, generator=torch.Generator().manual_seed(4)).to(device)
    wr = torch.randn(P, 2 * D, generator=torch.Generator().manual_seed(5)).to(device)
    spread = g.integers(0, Q - 1, P)                           # protein Q - 1 is named by none
    spread[:Q - 1] = np.arange(Q - 1)
    lists = [spread, np.full(P, 3), g.integers(0, Q, P)]       # ... then one protein named by every pair, then any
    first = [g.integers(0, P, P) for _ in lists]               # the other side of the gathered form: mol segments, repeated
    lst, lst1 = ops.PairList(P, Q, device), ops.PairList(P, P, device, name="idx1", over="segments of x1")

    def shared(index):
        a, b = mol.clone().requires_grad_(), pro.clone().requires_grad_()
        out, a2, b2 = ops.pair_pool_shared(a, b, msp, psp, index, with_identity=True)
        ((out * w).sum() + (a2 * a2).sum() + (b2 * b2).sum()).backward()
        return out.detach(), a.grad, b.grad

    def gathered(i1, i2):
        a, b = mol.clone().requires_grad_(), pro.clone().requires_grad_()
        out, a2, b2 = ops.pair_pool_gather_shared(a, b, msp, psp, i1, i2, with_identity=True)
        ((out * w).sum() + (a2 * a2).sum() + (b2 * b2).sum()).backward()
        return out.detach(), a.grad, b.grad

    def rows(index):
        f = flat.clone().requires_grad_()
        out = ops.pair_rows(f, index)
        (out * wr).sum().backward()
        return out.detach(), f.grad

    for k, (idx, idx1) in enumerate(zip(lists, first)):
        host, host1 = ops.pair_index(idx, P, Q), ops.pair_index(idx1, P, P, name="idx1", over="segments of x1")
        lst.load(idx), lst1.load(idx1)
        for what, got, want in (("pair_pool_shared", shared(lst), shared(host)), ("pair_pool_gather_shared", gathered(lst1, lst), gathered(host1, host)),
                                ("pair_rows", rows(lst), rows(host))):
            for name, a, b in zip(("output", "first gradient", "second gradient"), got, want):
                assert torch.equal(a, b), f"list {k} {what} {name}: max |d| {float((a - b).abs().max()):.3e}"
    with pytest.raises(IndexError, match="validated for 24 pairs over 6"):
        ops.pair_pool_shared(mol, pro, msp, _segments(pro_sizes[:5], D, device, 2)[1], lst)


# ------------------------------------------------------------------------------------------------------------------------------------
# shuffled training through one captured step
# ------------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b, scale):
    return float((a.double() - b.double()).abs().max()) / max(float(scale.double().abs().max()), 1e-300)


def _within(got, ref, permuted, what):
    """|got - ref| <= 4 x max(d_perm, 2^-20), all relative to the quantity's largest magnitude; d_perm = |permuted - ref| (same scale)."""
    d_perm, d = _rel(permuted, ref, ref), _rel(got, ref, ref)
    print(f"[pair list] {what}: d_perm {d_perm:.3e}  d {d:.3e}  bound {4 * max(d_perm, FLOOR):.3e}", flush=True)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    assert d <= 4 * max(d_perm, FLOOR), f"{what}: deviates {d:.3e} > 4 x max(d_perm = {d_perm:.3e}, 2^-20)"


def _mse(out, batch):
    return torch.nn.functional.mse_loss(out.view(-1), batch.y.view(-1))


def _dti_net(device, **kw):
    torch.manual_seed(0)
    return model.ArchitectureDTI(e_dim=64, message_steps=2, mol_block="_TripletMessage", **_ACTS, **kw).to(device).train()


def _dti_eager(net, w, ids):
    """The loss of eager ``forward_shared`` on a fresh ligand Batch and a fresh host index of the pairs ``ids``."""
    mb = Batch.from_data_list([w.ligs[i] for i in w.first[ids]]).to(w.device)
    out = net.forward_shared(mb, w.pro, ops.pair_index(w.second[ids], len(ids), 3))
    return _mse(out, types.SimpleNamespace(y=w.y_dev[torch.as_tensor(ids, device=w.device)]))


def _grads(net, loss):
    return loss.detach(), torch.autograd.grad(loss, list(net.parameters()))


@pytest.mark.parametrize("split", [False, True], ids=["one phantom graph", "phantom_rows"])
def test_dti_replay_follows_every_shuffled_load(device, split):
    """Six steps on different shuffled pairs through ONE batch object and one stepper whose optimizer never moves the parameters: eager,
    capture, replays.  The default pro_block="_GCNConv" is admitted: the protein tower never sees a phantom row."""
    w, B = _world(device), 8
    net = _dti_net(device)
    assert type(net.pro_conv.conv).__name__ == "_GCNConv"
    batch = w.pairs.dti_batch(w.dd, w.pro, B, phantom_rows=int(w.dd.ns.max()) if split else None)
    step = model.SharedStep(net)
    stepper = graphs.GraphedTrainStep(step, optim.Adam(step.parameters(), lr=0.0, capturable=True), graphs.padded_loss(_mse))
    rng = np.random.default_rng(9)
    names = [n for n, _ in net.named_parameters()]
    for k in range(6):
        ids = rng.permutation(120)[:B]
        (l_ref, g_ref), (l_perm, g_perm) = _grads(net, _dti_eager(net, w, ids)), _grads(net, _dti_eager(net, w, ids[rng.permutation(B)]))
        loss = stepper(batch.load(ids, launch=k % 2 == 0))
        _within(loss, l_ref, l_perm, f"step {k + 1} loss")
        for name, p, r, q in zip(names, net.parameters(), g_ref, g_perm):
            _within(p.grad, r, q, f"step {k + 1} grad {name}")
    assert stepper.graphs() == 1


def test_ddi_replay_follows_every_shuffled_load(device):
    rng = np.random.default_rng(17)
    drugs = Batch.from_data_list(_drugs(20, 5)).to(device)
    first, second = rng.integers(0, 20, 90), rng.integers(0, 20, 90)
    y = rng.standard_normal((90, 1)).astype(np.float32)
    y_dev = torch.from_numpy(y).to(device)
    B = 16
    batch = data.ResidentPairs(first, second, y, device).ddi_batch(drugs, batch_size=B)
    torch.manual_seed(0)
    net = model.ArchitectureDDI(e_dim=64, message_steps=2, **_ACTS).to(device).train()
    step = model.SharedStep(net)
    stepper = graphs.GraphedTrainStep(step, optim.Adam(step.parameters(), lr=0.0, capturable=True), graphs.padded_loss(_mse))

    def eager(ids):
        out = net.forward_shared(drugs, drugs, first[ids], second[ids])
        return _grads(net, _mse(out, types.SimpleNamespace(y=y_dev[torch.as_tensor(ids, device=device)])))

    names = [n for n, _ in net.named_parameters()]
    for k in range(6):
        ids = rng.permutation(90)[:B]
        (l_ref, g_ref), (l_perm, g_perm) = eager(ids), eager(ids[rng.permutation(B)])
        loss = stepper(batch.load(ids, launch=k % 2 == 0))
        _within(loss, l_ref, l_perm, f"step {k + 1} loss")
        for name, p, r, q in zip(names, net.parameters(), g_ref, g_perm):
            _within(p.grad, r, q, f"step {k + 1} grad {name}")
    assert stepper.graphs() == 1


def test_parameters_move_as_in_the_eager_loop(device):
    """lr = 1e-3 for six steps: the graphed loop against the eager loop on the same pair ids from the same weights; the permuted twin is
    the eager loop on per-step permuted pairs."""
    w, B = _world(device), 8
    net = _dti_net(device)
    ref, twin = copy.deepcopy(net), copy.deepcopy(net)
    batch = w.pairs.dti_batch(w.dd, w.pro, B)
    step = model.SharedStep(net)
    stepper = graphs.GraphedTrainStep(step, optim.Adam(step.parameters(), lr=1e-3, capturable=True), graphs.padded_loss(_mse))
    opts = [optim.Adam(m.parameters(), lr=1e-3, capturable=True) for m in (ref, twin)]
    rng = np.random.default_rng(21)
    for k in range(6):
        ids = rng.permutation(120)[:B]
        stepper(batch.load(ids, launch=k % 2 == 0))
        for m, opt, use in ((ref, opts[0], ids), (twin, opts[1], ids[rng.permutation(B)])):
            opt.zero_grad(set_to_none=True)
            _dti_eager(m, w, use).backward()
            opt.step()
    assert stepper.graphs() == 1
    moved = 0.0
    for (name, p), r, q, p0 in zip(net.named_parameters(), ref.parameters(), twin.parameters(), _dti_net(device).parameters()):
        _within(p.detach(), r.detach(), q.detach(), f"parameter {name}")
        moved = max(moved, float((p.detach() - p0.detach()).abs().max()))
    assert moved > 1e-4, "the parameters moved"


@pytest.mark.parametrize("kw,named", [(dict(end_norm="_BatchNorm"), "lin_out0.norm"), (dict(flat_norm="_LayerNorm"), "mol_flat.norm")])
def test_admission_refuses_on_the_first_step_with_nothing_captured(device, kw, named):
    w = _world(device)
    net = _dti_net(device, **kw)
    batch = w.pairs.dti_batch(w.dd, w.pro, 8).load(np.arange(8))
    step = model.SharedStep(net)
    stepper = graphs.GraphedTrainStep(step, optim.Adam(step.parameters(), lr=0.0, capturable=True), graphs.padded_loss(_mse))
    with _lib.kernel_timer() as kt:
        with pytest.raises(ValueError, match=named.replace(".", r"\.")):
            stepper(batch)
    assert _names(kt) == [] and stepper.graphs() == 0
    assert all(not m._forward_pre_hooks for m in net.modules())


def test_ddi_admission_does_not_refuse_a_batch_norm_in_the_head(device):
    rng = np.random.default_rng(19)
    drugs = Batch.from_data_list(_drugs(20, 5)).to(device)
    pairs = data.ResidentPairs(rng.integers(0, 20, 90), rng.integers(0, 20, 90), rng.standard_normal((90, 1)).astype(np.float32), device)
    batch = pairs.ddi_batch(drugs, batch_size=16)
    torch.manual_seed(0)
    net = model.ArchitectureDDI(e_dim=64, message_steps=2, end_norm="_BatchNorm", **_ACTS).to(device).eval()
    step = model.SharedStep(net)
    stepper = graphs.GraphedTrainStep(step, optim.Adam(step.parameters(), lr=0.0, capturable=True), graphs.padded_loss(_mse))
    losses = [stepper(batch.load(rng.permutation(90)[:16])) for _ in range(3)]
    assert bool(torch.isfinite(torch.stack(losses)).all()) and stepper.graphs() == 1
