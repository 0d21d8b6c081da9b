"""GPU (MI355X): refillable protein batches (``data.ResidentDTIRefillBatch``).  The order contract after every load —
the real part of ``pro`` is ``proteins.collate(slots)`` field by field, ``index`` the lists ``ops.pair_index(keys, ...)`` builds on the host,
``y`` the pairs' labels, all ``torch.equal``; ``SharedStep(net)(batch)[:B]`` and every parameter gradient against eager ``forward_shared``
on fresh collates within ``_within`` of tests/test_gpu_padded.py (4 x the eager path's own sensitivity to the order of the pairs, floor
2^-20), for ``pro_block`` ``_GCNConv`` (the inline route of csrc/gcn.hip against the cached route) and ``_NNConv``, in ``eval()`` and
``train()``; filler and phantom proteins do not reach the real rows; one captured graph follows three different loads.

12 synthetic proteins of 20 - 70 residues and one of 130, 40 ligands, 200 pairs, B = 8, Qb = 4."""
import numpy as np
import pytest
import torch

from glam_amd import _lib, data, graphs, model, ops, optim
from glam_amd.data import Data, DeviceDataset, synth_molecule, synth_protein
from tests import protein_refill_restated as R
from tests.test_gpu_padded import _within

pytestmark = pytest.mark.gpu

B, QB = 8, 4
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")
_WORLD = {}


class _World:
    def __init__(self, device):
        rng = np.random.default_rng(31)
        strip = lambda d: Data(d.x, d.edge_index, d.edge_attr)      # noqa: E731  (no y: the labels belong to the pairs)
        self.device = device
        pros = [synth_protein(rng, 20, 70) for _ in range(12)] + [synth_protein(rng, 130, 130)]
        self.ligands = DeviceDataset([strip(synth_molecule(rng)) for _ in range(40)], device)
        self.proteins = DeviceDataset([strip(p) for p in pros], device)
        self.first = rng.integers(0, 40, 200)
        self.second = rng.integers(0, 13, 200)
        self.second[:20] = 12                                       # (enough pairs of the largest protein for a load of it alone)
        self.y = rng.standard_normal((200, 1)).astype(np.float32)
        self.y_dev = torch.from_numpy(self.y).to(device)
        self.pairs = data.ResidentPairs(self.first, self.second, self.y, device)
        m = int(self.proteins.ns.max())
        self.kw = dict(phantom_rows=int(self.ligands.ns.max()), protein_slots=QB, protein_phantom_rows=m)
        # three loads: one protein alone, exactly Qb proteins, repeated proteins below Qb
        by = [np.flatnonzero(self.second == q) for q in range(13)]
        self.loads = [by[12][:B],
                      np.concatenate([by[q][:2] for q in (1, 4, 7, 9)]),
                      np.concatenate([by[3][:5], by[10][:3]])[rng.permutation(B)]]
        assert [len(set(self.second[i].tolist())) for i in self.loads] == [1, QB, 2] and all(len(i) == B for i in self.loads)

    def batch(self):
        return self.pairs.dti_batch(self.ligands, self.proteins, B, **self.kw)


def _world(device):
    if device not in _WORLD:
        _WORLD[device] = _World(device)
    return _WORLD[device]


def _same(got, want, what):
    want = torch.as_tensor(np.ascontiguousarray(want)).to(got.device) if not torch.is_tensor(want) else want
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    assert torch.equal(got, want), f"{what}: differs"


def _mark(batch):
    """Every tensor a load must rewrite, filled with a marker — through ``.data``, as a kernel writes: no version counter moves, so the
    index caches and trust marks that hang on these tensor objects stay what they are."""
    for pb in (batch.mol, batch.pro):
        xbuf, arena = pb._keep
        for t, v in ((xbuf, float("nan")), (arena, -7), (pb.edge_index, -7), (pb.batch, -7), (pb.ptr, -7), (pb.edge_attr, float("nan"))):
            t.data.fill_(v)
    batch.index._arena.data.fill_(-7)
    batch.y.data.fill_(float("nan"))


def _check_contract(w, batch, ids, what):
    slots, keys, U = R.slots_and_keys(w.second[ids], w.proteins.ns, QB)
    if batch.slots is not None:                                # (the host copies of the last load(ids))
        assert (batch.slots.tolist(), batch.keys.tolist(), batch.distinct) == (slots, keys, U)
    pro, Kp, K = batch.pro, batch.pro.num_phantom_graphs, batch.mol.num_phantom_graphs
    ref = w.proteins.collate(slots)
    N, E = ref.x.size(0), ref.edge_index.size(1)
    _same(pro.x[:N], ref.x, f"{what} pro.x"), _same(pro.edge_index[:, :E], ref.edge_index, f"{what} pro.edge_index")
    _same(pro.edge_attr[:E], ref.edge_attr, f"{what} pro.edge_attr"), _same(pro.batch[:N], ref.batch, f"{what} pro.batch")
    _same(pro.ptr[:QB + 1], ref.ptr, f"{what} pro.ptr")
    assert bool((pro.x[N:] == 0).all()) and bool((pro.batch[N:] >= QB).all()) and int(pro.ptr[-1]) == pro.capacity[0]
    assert bool((pro.edge_index[0, E:] == pro.edge_index[1, E:]).all()) and bool((pro.edge_index[0, E:] >= N).all())      # phantom self-loops
    gi, gr = ops.graph_index(pro.edge_index, pro.capacity[0]), ops.graph_index(ref.edge_index, N)
    assert gi.rowptr.untyped_storage().data_ptr() == pro._keep[1].untyped_storage().data_ptr()      # the batch's own index, not a rebuilt one
    _same(gi.rowptr[:N + 1], gr.rowptr, f"{what} rowptr"), _same(gi.src[:E], gr.src, f"{what} src")
    _same(gi.transpose()[0][:N + 1], gr.transpose()[0], f"{what} colptr"), _same(gi.transpose()[1][:E], gr.transpose()[1], f"{what} dst")
    lig = w.ligands.collate(w.first[ids])
    _same(batch.mol.x[:lig.x.size(0)], lig.x, f"{what} mol.x")
    full = np.concatenate([keys, np.zeros(K, dtype=np.int64)]).astype(np.int32)
    host = ops.pair_index(full, B + K, QB + Kp).by_protein()
    _same(batch.index.idx, full, f"{what} idx"), _same(batch.index.order, host.order, f"{what} order"), _same(batch.index.ptr, host.ptr, f"{what} ptr")
    _same(batch.y, w.y[ids], f"{what} y")


def test_order_contract_after_every_load(device):
    w = _world(device)
    batch = w.batch()
    K, Kp = batch.mol.num_phantom_graphs, batch.pro.num_phantom_graphs
    assert batch.num_graphs == B + K == batch.index.P and batch.index.Q == QB + Kp == batch.pro.num_graphs and batch.num_real_graphs == B
    assert ops.gcn_inline(batch.pro.edge_index) and not ops.gcn_inline(batch.mol.edge_index) and batch.y.shape == (B, 1)
    _mark(batch)
    for k, ids in enumerate(w.loads):
        with _lib.kernel_timer() as kt:
            if k == 1:                                         # the upload alone, then the hook
                batch.load(ids, launch=False)
                batch.glam_reload()
            else:
                batch.load(ids)
                batch.glam_reload()                            # outside a capture a launched load is not repeated
        names = [n for n, _g, _us in kt.records()]
        assert len(names) == 4 and all(n.startswith("k_collate_padded") for n in names[:2]) and names[2:] == ["k_pair_list_load"] * 2, names
        _check_contract(w, batch, ids, f"load {k}")
    _mark(batch)
    assert batch.load_many(w.loads) == 3
    for k in (2, 0, 1):
        batch.load(step=k)
        batch.slots = None                                     # (the host copies follow load(ids) only)
        _check_contract(w, batch, w.loads[k], f"step {k}")
    many = np.concatenate([np.flatnonzero(w.second == q)[:2] for q in (0, 2, 5, 6)])[:B - 1].tolist() + [int(np.flatnonzero(w.second == 8)[0])]
    with _lib.kernel_timer() as kt:
        with pytest.raises(ValueError, match="5 distinct proteins, the batch holds protein_slots = 4"):
            batch.load(many)
        with pytest.raises(ValueError, match="exactly 8 pairs"):
            batch.load(w.loads[0][:-1])
    assert kt.records() == [], "a refused load launches nothing"
    _check_contract(w, batch, w.loads[1], "a refused load leaves the batch as it was")


def _mse(out, y):
    return torch.nn.functional.mse_loss(out.view(-1), y.view(-1))


def _net(device, alpha, pro_block, train):
    torch.manual_seed(0)
    net = model.ArchitectureDTI(hid_dim_alpha=alpha, e_dim=64, message_steps=2, pro_block=pro_block, **_ACTS).to(device)
    return net.train() if train else net.eval()


def _eager(net, w, ids):
    """``(out, loss, grads)`` of eager ``forward_shared`` on fresh collates of the pairs' ligands and DISTINCT proteins and a host index."""
    u, keys, _U = R.slots_and_keys(w.second[ids], w.proteins.ns, len(set(w.second[ids].tolist())))
    out = net.forward_shared(w.ligands.collate(w.first[ids]), w.proteins.collate(u), ops.pair_index(keys, len(ids), len(u)))
    loss = _mse(out, w.y_dev[torch.as_tensor(ids, device=w.device)])
    return out.detach(), loss.detach(), torch.autograd.grad(loss, list(net.parameters()))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("alpha", [1, 4])
@pytest.mark.parametrize("pro_block", ["_GCNConv", "_NNConv"])
def test_step_on_a_refilled_batch_against_eager_forward_shared(device, pro_block, alpha, train):
    w = _world(device)
    net = _net(device, alpha, pro_block, train)
    batch, step = w.batch(), model.SharedStep(net)
    names = [n for n, _ in net.named_parameters()]
    rng = np.random.default_rng(5)
    with batch.glam_admission(step):
        for k, ids in enumerate(w.loads):
            perm = rng.permutation(B)
            o_ref, l_ref, g_ref = _eager(net, w, ids)
            o_perm, l_perm, g_perm = _eager(net, w, ids[perm])
            out = step(batch.load(ids))[:B]
            loss = _mse(out, batch.y)
            grads = torch.autograd.grad(loss, list(net.parameters()))
            _within(out.detach(), o_ref, o_perm[torch.as_tensor(np.argsort(perm), device=device)], f"load {k} output")
            _within(loss.detach(), l_ref, l_perm, f"load {k} loss")
            for name, g, r, q in zip(names, grads, g_ref, g_perm):
                _within(g, r, q, f"load {k} grad {name}")


@pytest.mark.parametrize("pro_block", ["_GCNConv", "_NNConv"])
def test_filler_and_phantom_proteins_do_not_reach_the_real_rows(device, pro_block):
    w = _world(device)
    net, batch = _net(device, 4, pro_block, False), w.batch()
    step = model.SharedStep(net)
    for ids in w.loads[::2]:                                   # U = 1 and U = 2: two or three fillers
        batch.load(ids)
        n_real = int(w.proteins.ns[batch.slots[:batch.distinct]].sum())
        with torch.no_grad():
            out1 = step(batch)[:B].clone()
            rows = batch.pro.x.data[n_real:]                  # (written as a kernel writes: no version counter moves)
            rows.copy_(torch.randn(rows.shape, device=device, generator=torch.Generator(device).manual_seed(1)) * 50)
            out2 = step(batch)[:B]
        assert torch.equal(out1, out2), f"max |d| {float((out1 - out2).abs().max()):.3e}"


def test_one_graph_follows_three_loads(device):
    w = _world(device)
    net, batch = _net(device, 4, "_GCNConv", True), w.batch()
    step = model.SharedStep(net)
    stepper = graphs.GraphedTrainStep(step, optim.Adam(step.parameters(), lr=0.0, capturable=True),
                                      graphs.padded_loss(lambda out, b: _mse(out, b.y)))
    rng = np.random.default_rng(9)
    losses = []
    for k, ids in enumerate(w.loads):
        _o, l_ref, _g = _eager(net, w, ids)
        _o, l_perm, _g = _eager(net, w, ids[rng.permutation(B)])
        losses.append(stepper(batch.load(ids, launch=k % 2 == 0)))
        _within(losses[-1], l_ref, l_perm, f"step {k + 1} loss")
    assert stepper.graphs() == 1
    again = stepper(batch.load(w.loads[0], launch=False))
    assert stepper.graphs() == 1 and torch.equal(again, losses[0]), f"{float(again)} vs {float(losses[0])}"


def test_admission_refuses_a_protein_side_gat_on_the_first_step(device):
    w = _world(device)
    net = _net(device, 4, "_GATConv", True)
    step = model.SharedStep(net)
    stepper = graphs.GraphedTrainStep(step, optim.Adam(step.parameters(), lr=0.0, capturable=True),
                                      graphs.padded_loss(lambda out, b: _mse(out, b.y)))
    batch = w.batch().load(w.loads[0], launch=False)
    with _lib.kernel_timer() as kt:
        with pytest.raises(ValueError, match=r"pro_conv\.conv \(_GATConv\)"):
            stepper(batch)
    assert kt.records() == [] and stepper.graphs() == 0
