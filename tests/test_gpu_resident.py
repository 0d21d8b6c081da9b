"""GPU: device-resident datasets.  Every oracle is the existing path — ``PackedDataset.collate(ids).to(device)`` for the
batch, ``GraphIndex`` / ``SegmentPtr`` built from clones of the same tensors for the index — so every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

from glam_amd import _lib, model, ops
from glam_amd.data import Data, DataLoader, DeviceDataset, PackedDataset, synth_molecule, synth_protein

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _mols():
    rng = np.random.default_rng(11)
    return tuple(synth_molecule(rng) for _ in range(70))


def _star(n):
    """Node 0 bonded to n - 1 leaves, both directions: the hub has in- and out-degree n - 1."""
    hub, leaves = torch.zeros(n - 1, dtype=torch.long), torch.arange(1, n)
    ei = torch.cat([torch.stack([leaves, hub]), torch.stack([hub, leaves])], 1)
    g = torch.Generator().manual_seed(n)
    return Data(torch.randn(n, 15, generator=g), ei, torch.eye(4)[torch.arange(ei.size(1)) % 4], torch.randn(1, 1, generator=g))


def _hand_made(star_nodes):
    g = torch.Generator().manual_seed(5)
    lone = Data(torch.randn(1, 15, generator=g), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 4), torch.randn(1, 1, generator=g))
    pair = Data(torch.randn(2, 15, generator=g), torch.tensor([[0, 1], [1, 0]]), torch.eye(4)[:2], torch.randn(1, 1, generator=g))
    return [lone, pair, _star(star_nodes)]


def _tiny_graphs(count=48):
    """Paths of 1-3 nodes."""
    g, out = torch.Generator().manual_seed(7), []
    for i in range(count):
        n = 1 + i % 3
        a = torch.arange(n - 1)
        ei = torch.cat([torch.stack([a, a + 1]), torch.stack([a + 1, a])], 1)
        out.append(Data(torch.randn(n, 15, generator=g), ei, torch.eye(4)[torch.arange(ei.size(1)) % 4], torch.randn(1, 1, generator=g)))
    return out


def _case(name):
    """-> (graphs, [id lists], whether both ELL forms exist)"""
    rng = np.random.default_rng(3)
    if name == "a-molecules":
        ids = rng.permutation(64)[:48]
        ids[7], ids[30] = ids[0], ids[19]                   # two graphs twice
        return list(_mols()[:64]), [ids], True
    if name == "b-hand-made":                               # a 1-node 0-edge graph, a 2-node graph, a 5-node star (hub degree 4)
        return _hand_made(5), [[0, 1, 2], [0], [0, 2, 1, 0]], True
    if name == "c-degree-5":                                # the star with a sixth node: no ELL form, the CSR as before
        return _hand_made(6), [[0, 1, 2], [2, 2]], False
    if name == "d-proteins":                                # F = 49, De = 8 continuous, unsorted duplicate edges, degree > 4
        return [synth_protein(rng, 20, 40) for _ in range(4)], [[3, 1, 0, 2, 1]], False
    if name == "e-y-rows":                                  # 1, 2 and 3 rows of y per graph: the y_ptr path
        g = torch.Generator().manual_seed(9)
        graphs = [Data(m.x, m.edge_index, m.edge_attr, torch.randn(1 + i % 3, 2, generator=g)) for i, m in enumerate(_mols()[:9])]
        return graphs, [[4, 8, 0, 5, 5, 1]], True
    if name == "f-global-table":                            # one slot more than a block keeps in LDS
        return _tiny_graphs(), [rng.integers(0, 48, int(_lib.load().glam_collate_lds_slots()) + 1)], True
    raise KeyError(name)


CASES = ["a-molecules", "b-hand-made", "c-degree-5", "d-proteins", "e-y-rows", "f-global-table"]


def _same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, f"{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
    assert torch.equal(a, b), what


def _same_batch(b, ref, what):
    for f in ("x", "edge_index", "edge_attr", "y", "batch", "ptr"):
        _same(getattr(b, f), getattr(ref, f), f"{what} {f}")
    assert b.num_graphs == ref.num_graphs, what
    for f in ("edge_index", "batch"):
        t = getattr(b, f)
        assert t._glam_trusted == t._version and getattr(ref, f)._glam_trusted == getattr(ref, f)._version, f"{what} {f} mark"
    if ref.edge_attr is not None:
        assert b.edge_attr._glam_onehot == (ref.edge_attr._glam_onehot[0], b.edge_attr._version), f"{what} onehot mark"


@pytest.mark.parametrize("name", CASES)
def test_collation_and_index_equal_the_host_path(device, name):
    graphs, id_lists, has_ell = _case(name)
    packed = PackedDataset(graphs)
    dd = DeviceDataset(packed, device)
    assert (dd.ell_ok, dd.ell_t_ok) == (has_ell, has_ell) and len(dd) == len(graphs)
    for ids in id_lists:
        what = f"{name} ids={list(ids)[:8]}"
        b = dd.collate(ids)
        _same_batch(b, packed.collate(ids).to(device), what)
        N, B = b.x.size(0), len(ids)
        # no per-batch build, no read-back: the installed object, resolved, before any model call
        hit = ops._GI_CACHE.get(b.edge_index)
        gi = ops.graph_index(b.edge_index, N)
        assert hit is not None and gi is hit[1], what
        assert gi._ell is not False and gi._ell_t is not False and gi._t is not None, what
        sp = ops.segment_ptr(b.batch, B)
        assert sp is ops._SP_CACHE.get(b.batch) and sp is ops.segment_ptr(b.batch) and (sp.N, sp.B) == (N, B), what
        # the index of the existing path, from clones of the same tensors
        ref = ops.GraphIndex(b.edge_index.clone(), N)
        assert (gi.N, gi.E) == (ref.N, ref.E)
        for got, want, part in zip((gi.rowptr, gi.src, gi.eid) + gi.transpose(), (ref.rowptr, ref.src, ref.eid) + ref.transpose(),
                                   ("rowptr", "src", "eid", "colptr", "dst", "eid_t")):
            _same(got, want, f"{what} {part}")
        for got, want, part in ((gi.ell(), ref.ell(), "ell"), (gi.ell_t(), ref.ell_t(), "ell_t")):
            if has_ell:
                assert got is not None and want is not None, f"{what} {part}"
                _same(got[0], want[0], f"{what} {part} nodes")
                _same(got[1], want[1], f"{what} {part} edges")
                assert got[0].data_ptr() % 16 == 0 and got[1].data_ptr() % 16 == 0, f"{what} {part} alignment"
            else:
                assert got is None and want is None, f"{what} {part}"
        _same(sp.ptr, ops.SegmentPtr(b.batch.clone(), B).ptr, f"{what} segment ptr")


def test_collation_is_one_launch_and_the_index_needs_none(device):
    graphs, (ids,), _ = _case("a-molecules")
    dd = DeviceDataset(graphs, device)
    with _lib.kernel_timer() as kt:
        b = dd.collate(ids)
        gi = ops.graph_index(b.edge_index, b.x.size(0))
        gi.transpose(), gi.ell(), gi.ell_t(), ops.segment_ptr(b.batch, b.num_graphs)
    names = [r[0] for r in kt.records()]
    assert len(names) == 1 and "k_collate" in names[0], names


def test_bad_ids_raise_before_any_launch(device):
    dd = DeviceDataset(_hand_made(5), device)
    with _lib.kernel_timer() as kt:
        for ids in ([3], [0, -1]):
            with pytest.raises(IndexError):
                dd.collate(ids)
    assert kt.records() == []


def test_resident_loader_yields_the_host_loaders_batches(device):
    mols = list(_mols())
    host = DataLoader(mols, batch_size=16, shuffle=True, seed=3, device=device)
    res = DataLoader(mols, batch_size=16, shuffle=True, seed=3, device=device, resident=True)
    for epoch in range(2):                                  # (the order follows seed + epoch in both)
        hb, rb = list(host), list(res)
        assert len(hb) == len(rb) == len(res) == 5 and rb[-1].num_graphs == 6          # the short last batch included
        for k, (h, r) in enumerate(zip(hb, rb)):
            _same_batch(r, h, f"epoch {epoch} batch {k}")
    cached = DataLoader(mols, batch_size=16, device=device, resident=True)             # cache keeps its meaning: fixed order, same objects
    first, again = list(cached), list(cached)
    assert all(a is b for a, b in zip(first, again))
    for h, r in zip(DataLoader(mols, batch_size=16, device=device), first):
        _same_batch(r, h, "cached")


def test_model_forward_and_training_step_are_bit_equal(device):
    mols = list(_mols())
    packed = PackedDataset(mols)
    dd = DeviceDataset(packed, device)
    ids = np.random.default_rng(1).permutation(len(mols))[:32]
    torch.manual_seed(0)
    net = model.Architecture().to(device).eval()
    with torch.no_grad():
        out_res = net(dd.collate(ids))
        out_host = net(packed.collate(ids).to(device))
    assert out_res.shape == (32, 1) and torch.equal(out_res, out_host)
    # a training step of the shuffling loop's model (tools/bench_shuffle_loader.py: _NNConv, PairNorm, ReLU, no dropout)
    net = model.Architecture(mol_block="_NNConv", graph_norm="_PairNorm", graph_do="_None()", end_do="_None()", pre_act="ReLU", graph_act="ReLU",
                             flat_act="ReLU").to(device).train()
    steps = []
    for b in (dd.collate(ids), packed.collate(ids).to(device)):
        net.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(net(b).view(-1), b.y.view(-1))
        loss.backward()
        steps.append((loss.detach().clone(), [p.grad.clone() for p in net.parameters()]))
    (loss_res, g_res), (loss_host, g_host) = steps
    assert torch.equal(loss_res, loss_host)
    assert len(g_res) == len(g_host) > 0
    for (n, _p), a, b in zip(net.named_parameters(), g_res, g_host):
        assert torch.equal(a, b), n
