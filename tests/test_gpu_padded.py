"""GPU: fixed-capacity resident batches and the stepper that replays one captured step for every batch of a shuffling loop (DESIGN.md
§4.16).  Collation is compared exactly — the real part against ``DeviceDataset.collate``, the phantom tail against its numpy restatement
(tests/padded_restated.py), the whole index against the existing builders.  Floating-point results are held to the EXISTING path's own
sensitivity to the order of the graphs (``d_perm``, measured live per quantity): padding moves rows across blocks much as a permutation does.
"""
import functools

import numpy as np
import pytest
import torch

from glam_amd import _lib, graphs, model, ops, optim
from glam_amd.data import Data, DataLoader, DeviceDataset, PaddedBatch, synth_molecule, synth_protein
from tests.padded_restated import phantom_layout

pytestmark = pytest.mark.gpu

B8 = 8
FLOOR = 2.0 ** -20          # 8 ulp of the largest magnitude: the room a changed row count needs on an order-invariant path
PARITY = dict(mol_block="_TripletMessage", graph_do="_None()", end_do="_None()", pre_act="ReLU", graph_act="ReLU", flat_act="ReLU")


@functools.lru_cache(maxsize=None)
def _mols():
    rng = np.random.default_rng(23)
    return tuple(synth_molecule(rng) for _ in range(40))


@functools.lru_cache(maxsize=None)
def _dataset(device):
    return DeviceDataset(list(_mols()), device)


def _star6():
    """Node 0 bonded to 5 leaves, both directions: in- and out-degree 5, so a dataset that holds it has no ELL form."""
    hub, leaves = torch.zeros(5, dtype=torch.long), torch.arange(1, 6)
    ei = torch.cat([torch.stack([leaves, hub]), torch.stack([hub, leaves])], 1)
    g = torch.Generator().manual_seed(6)
    return Data(torch.randn(6, 15, generator=g), ei, torch.eye(4)[torch.arange(10) % 4], torch.randn(1, 1, generator=g))


def _tiny_graphs(count):
    """Paths of 1-2 nodes."""
    g, out = torch.Generator().manual_seed(7), []
    for i in range(count):
        n = 1 + i % 2
        ei = torch.tensor([[0, 1], [1, 0]])[:, :2 * (n - 1)]
        out.append(Data(torch.randn(n, 15, generator=g), ei, torch.eye(4)[torch.arange(ei.size(1)) % 4], torch.randn(1, 1, generator=g)))
    return out


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, f"{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
    assert torch.equal(a, b), what


def _check_load(dd, pb, ids, what, load=True):
    """``pb.load(ids)`` (``load=False``: the caller has loaded them): real part == ``dd.collate(ids)``, tail == the restatement, whole index ==
    the existing builders."""
    dev = dd.device
    ref = dd.collate(ids)
    if load:
        pb.load(ids)
    B, N, E = len(ids), ref.x.size(0), ref.edge_index.size(1)
    N_cap, E_cap = pb.capacity
    lay = phantom_layout(N, E, N_cap, E_cap)
    t = lambda a, dtype: torch.as_tensor(a, dtype=dtype, device=dev)       # noqa: E731
    assert pb.num_graphs == B + 1 and pb.num_real_graphs == B
    assert pb.x.shape == (N_cap,) + ref.x.shape[1:] and pb.edge_index.shape == (2, E_cap) and pb.batch.shape == (N_cap,) and pb.ptr.shape == (B + 2,)
    # fields: real part, phantom tail
    F, Fp = ref.x.size(1), -(-ref.x.size(1) // 4) * 4
    buf = ops.pad_cols(pb.x, Fp)
    assert buf.shape == (N_cap, Fp) and buf.data_ptr() == pb.x.data_ptr(), f"{what}: pad_cols must hand out the batch's own buffer, not a copy"
    _same(pb.x[:N], ref.x, f"{what} x")
    assert not buf[N:].any() and not buf[:, F:].any(), f"{what}: phantom x rows and the pad columns of every row are zero"
    _same(pb.edge_index[:, :E], ref.edge_index, f"{what} edge_index")
    _same(pb.edge_index[:, E:], t(lay["edge_index"], torch.int64), f"{what} phantom edge_index")
    _same(pb.edge_attr[:E], ref.edge_attr, f"{what} edge_attr")
    _same(pb.edge_attr[E:], dd.ea[:1].expand(E_cap - E, *dd.ea.shape[1:]).contiguous(), f"{what} phantom edge_attr = the dataset's edge row 0")
    _same(pb.y, ref.y, f"{what} y")
    _same(pb.batch[:N], ref.batch, f"{what} batch")
    assert bool((pb.batch[N:] == B).all()), f"{what} phantom batch"
    _same(pb.ptr[:B + 1], ref.ptr, f"{what} ptr")
    assert int(pb.ptr[B + 1]) == N_cap
    for f in ("edge_index", "batch"):
        assert getattr(pb, f)._glam_trusted == getattr(pb, f)._version, f"{what} {f} mark"
    assert pb.edge_attr._glam_onehot == (ref.edge_attr._glam_onehot[0], pb.edge_attr._version), f"{what} onehot mark"
    # the installed index, found without a build
    hit = ops._GI_CACHE.get(pb.edge_index)
    gi = ops.graph_index(pb.edge_index, N_cap)
    assert hit is not None and gi is hit[1] and (gi.N, gi.E) == (N_cap, E_cap), what
    sp = ops.segment_ptr(pb.batch, B + 1)
    assert sp is ops._SP_CACHE.get(pb.batch) and (sp.N, sp.B) == (N_cap, B + 1), what
    # ... its real part is glam_collate's, its tail the restatement
    gr = ops.graph_index(ref.edge_index, N)
    for (ptr_p, nbr_p, eid_p), (ptr_r, nbr_r, eid_r), part in (((gi.rowptr, gi.src, gi.eid), (gr.rowptr, gr.src, gr.eid), "by target"),
                                                                (gi.transpose(), gr.transpose(), "by source")):
        _same(ptr_p[:N + 1], ptr_r, f"{what} {part} pointer")
        _same(nbr_p[:E], nbr_r, f"{what} {part} neighbours")
        _same(eid_p[:E], eid_r, f"{what} {part} edge ids")
        _same(ptr_p[N:], t(lay["rowptr"], torch.int32), f"{what} {part} phantom pointer")
        _same(nbr_p[E:], t(lay["src"], torch.int32), f"{what} {part} phantom neighbours")
        _same(eid_p[E:], t(lay["eid"], torch.int32), f"{what} {part} phantom edge ids")
    has_ell = dd.ell_ok and dd.ell_t_ok
    assert has_ell or not (dd.ell_ok or dd.ell_t_ok)
    for got, real, part in ((gi.ell(), gr.ell(), "ell"), (gi.ell_t(), gr.ell_t(), "ell_t")):
        if not has_ell:
            assert got is None, f"{what} {part}"
            continue
        for k, name in ((0, "ell_nodes"), (1, "ell_edges")):
            _same(got[k][:N], real[k], f"{what} {part} {name}")
            _same(got[k][N:], t(lay[name], torch.int32), f"{what} {part} phantom {name}")
            assert got[k].data_ptr() % 16 == 0
    # ... and the whole of it what the existing builders make of the padded edge list
    whole = ops.GraphIndex(pb.edge_index.clone(), N_cap)
    for got, want, part in zip((gi.rowptr, gi.src, gi.eid) + gi.transpose(), (whole.rowptr, whole.src, whole.eid) + whole.transpose(),
                               ("rowptr", "src", "eid", "colptr", "dst", "eid_t")):
        _same(got, want, f"{what} built {part}")
    for got, want, part in ((gi.ell(), whole.ell(), "ell"), (gi.ell_t(), whole.ell_t(), "ell_t")):
        assert (got is None) == (want is None) == (not has_ell), f"{what} built {part}"
        if has_ell:
            _same(got[0], want[0], f"{what} built {part} nodes")
            _same(got[1], want[1], f"{what} built {part} edges")
    _same(sp.ptr, ops.SegmentPtr(pb.batch.clone(), B + 1).ptr, f"{what} segment ptr")
    return ref


def _sizes(dd, ids):
    return int(dd.ns[list(ids)].sum()), int(dd.es[list(ids)].sum())


def test_collate_random_batch_f15_rows_padded_to_16(device):
    dd = _dataset(device)
    pb = dd.padded(B8)
    assert isinstance(pb, PaddedBatch) and pb.capacity == dd.capacity(B8)
    assert ops.padded_base(pb.x).shape == (pb.capacity[0], 16)             # F = 15: rows of 16 floats, the last one zero
    ids = np.random.default_rng(1).permutation(40)[:B8]
    _check_load(dd, pb, ids, "random")


def test_collate_batch_that_attains_e_cap(device):
    dd = _dataset(device)
    pb = dd.padded(B8)
    ids = np.argsort(dd.es, kind="stable")[-B8:]
    assert _sizes(dd, ids)[1] == pb.capacity[1]                            # E_pad = 0: phantom nodes without any edge
    _check_load(dd, pb, ids, "E_pad = 0")


@pytest.mark.parametrize("extra,what", [((1, 4), "one phantom node of degree 4"), ((50, 7), "phantom nodes without edges")])
def test_collate_chosen_capacities(device, extra, what):
    dd = _dataset(device)
    ids = np.random.default_rng(2).permutation(40)[:B8]
    N, E = _sizes(dd, ids)
    pb = dd.padded(B8, capacity=(N + extra[0], E + extra[1]))
    _check_load(dd, pb, ids, what)


def test_collate_dataset_with_a_degree_5_star_has_no_ell_form(device):
    dd = DeviceDataset(list(_mols()[:12]) + [_star6()], device)
    assert not dd.ell_ok and not dd.ell_t_ok
    ids = [3, 12, 0, 7]
    N, E = _sizes(dd, ids)
    pb = dd.padded(4, capacity=(N + 2, E + 11))                            # 11 self-loops on 2 phantom nodes: degrees 6 and 5
    assert dd.capacity(4)[0] == int(np.sort(dd.ns)[-4:].sum()) + 1
    _check_load(dd, pb, ids, "degree-5 star")


def test_collate_protein_records_rows_of_49_padded_to_52(device):
    rng = np.random.default_rng(4)
    dd = DeviceDataset([synth_protein(rng, 20, 40) for _ in range(6)], device)
    pb = dd.padded(3)
    assert ops.padded_base(pb.x).shape == (pb.capacity[0], 52) and pb.edge_attr.size(1) == 8
    _check_load(dd, pb, [4, 0, 2], "proteins")


def test_collate_table_beyond_the_lds_slots(device):
    B = int(_lib.load().glam_collate_lds_slots()) + 1
    dd = DeviceDataset(_tiny_graphs(B + 60), device)
    pb = dd.padded(B)
    _check_load(dd, pb, np.random.default_rng(8).permutation(B + 60)[:B], "global-memory table")


def test_second_smaller_load_leaves_no_residue(device):
    dd = _dataset(device)
    pb = dd.padded(B8)
    big, small = np.argsort(dd.ns, kind="stable")[-B8:], np.argsort(dd.ns, kind="stable")[:B8]
    assert _sizes(dd, small)[0] < _sizes(dd, big)[0] and _sizes(dd, small)[1] < _sizes(dd, big)[1]
    pb.load(big)
    pb.load(small)
    _check_load(dd, pb, small, "second, smaller load", load=False)       # (every field is compared over its whole capacity, pad columns included)
    pb.load_many([big, small, big[::-1]])                     # ... and the same through the uploaded tables of an epoch
    for step, ids in ((0, big), (1, small), (2, big[::-1])):
        pb.load(step=step)
        _check_load(dd, pb, ids, f"load_many step {step}", load=False)


def test_one_launch_per_load_and_none_for_the_index(device):
    dd = _dataset(device)
    pb = dd.padded(B8)
    ids = np.arange(B8)
    with _lib.kernel_timer() as kt:
        pb.load(ids)
        gi = ops.graph_index(pb.edge_index, pb.x.size(0))
        gi.transpose(), gi.ell(), gi.ell_t(), ops.segment_ptr(pb.batch, pb.num_graphs)
    names = [r[0] for r in kt.records()]
    assert len(names) == 1 and "k_collate_padded" in names[0], names
    with _lib.kernel_timer() as kt:
        pb.load(ids, launch=False)                            # the table only: the launch belongs to the stepper's graph
    assert kt.records() == []


def test_refused_loads_launch_nothing(device):
    dd = _dataset(device)
    pb = dd.padded(B8)
    heavy = int(np.argmax(dd.es))
    assert B8 * int(dd.es[heavy]) > pb.capacity[1]
    with _lib.kernel_timer() as kt:
        with pytest.raises(ValueError, match="exactly 8 graphs"):
            pb.load(np.arange(7))
        with pytest.raises(ValueError, match="capacity"):
            pb.load([heavy] * B8)                             # repeated ids overflow what holds any 8 DISTINCT graphs
        with pytest.raises(IndexError):
            pb.load([0, 1, 2, 3, 4, 5, 6, 40])
        with pytest.raises(ValueError, match="exactly 8 graphs"):
            pb.load_many([np.arange(8), np.arange(7)])
        with pytest.raises(IndexError):
            pb.load(step=0)                                   # nothing uploaded
    assert kt.records() == []
    with pytest.raises(ValueError, match="largest graph"):
        dd.padded(B8, capacity=(int(dd.ns.max()), 10 ** 4))
    with pytest.raises(ValueError, match="y rows"):
        g = torch.Generator().manual_seed(1)
        DeviceDataset([Data(m.x, m.edge_index, m.edge_attr, torch.randn(1 + i % 2, 1, generator=g)) for i, m in enumerate(_mols()[:6])], device).padded(2)


def test_padded_loader_reloads_one_batch_in_the_resident_loaders_order(device):
    mols = list(_mols())
    res = DataLoader(mols, batch_size=12, shuffle=True, seed=3, device=device, resident=True)
    pad = DataLoader(mols, batch_size=12, shuffle=True, seed=3, device=device, resident=True, padded=True)
    for epoch in range(2):
        first = None
        for k, (r, p) in enumerate(zip(res, pad)):
            N, E = r.x.size(0), r.edge_index.size(1)
            if k < 3:                                         # full batches: the same object, reloaded
                first = first or p
                assert p is first and isinstance(p, PaddedBatch) and p.num_real_graphs == 12
                _same(p.x[:N], r.x, f"epoch {epoch} batch {k} x")
                _same(p.edge_index[:, :E], r.edge_index, f"epoch {epoch} batch {k} edge_index")
                _same(p.y, r.y, f"epoch {epoch} batch {k} y")
            else:                                             # the short last one: an ordinary batch
                assert not isinstance(p, PaddedBatch) and p.num_graphs == 4
                _same(p.x, r.x, "short batch x")
        assert k == 3


# ------------------------------------------------------------------------------------------------------------------------------------
# floating point: the padded batch against the unpadded one, within 4 x the unpadded path's own sensitivity to the order of the graphs
# ------------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b, scale):
    return float((a.double() - b.double()).abs().max()) / max(float(scale.double().abs().max()), 1e-300)


def _within(got, ref, permuted, what):
    """|got - ref| <= 4 x max(d_perm, 2^-20), all relative to the quantity's largest magnitude; d_perm = |permuted - ref| (same scale)."""
    d_perm, d = _rel(permuted, ref, ref), _rel(got, ref, ref)
    print(f"[padded] {what}: d_perm {d_perm:.3e}  d_padded {d:.3e}  bound {4 * max(d_perm, FLOOR):.3e}", flush=True)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    assert d <= 4 * max(d_perm, FLOOR), f"{what}: padded deviates {d:.3e} > 4 x max(d_perm = {d_perm:.3e}, 2^-20)"


def _mse(out, batch):
    return torch.nn.functional.mse_loss(out.view(-1), batch.y.view(-1))


def _eager_step(net, batch, n=None):
    """(loss, parameter gradients) of one eager step; ``n``: the loss reads ``output[:n]``.  ``p.grad`` is left alone."""
    out = net(batch)
    loss = _mse(out if n is None else out[:n], batch)
    return loss.detach(), torch.autograd.grad(loss, list(net.parameters()))


def test_phantom_graph_does_not_reach_the_real_graphs(device):
    dd = _dataset(device)
    pb = dd.padded(B8)
    rng = np.random.default_rng(5)
    ids = rng.permutation(40)[:B8]
    perm = rng.permutation(B8)
    torch.manual_seed(0)
    net = model.Architecture(**PARITY).to(device).eval()
    with torch.no_grad():
        ref, permuted = net(dd.collate(ids)), net(dd.collate(ids[perm]))
        out = net(pb.load(ids))
    assert out.shape == (B8 + 1, 1) and bool(torch.isfinite(out).all()), "every row is finite, the phantom graph's included"
    inv = torch.as_tensor(np.argsort(perm), device=device)
    _within(out[:B8], ref, permuted[inv], "model output")


def test_gradients_of_one_training_step(device):
    dd = _dataset(device)
    pb = dd.padded(B8)
    rng = np.random.default_rng(6)
    ids = rng.permutation(40)[:B8]
    torch.manual_seed(0)
    net = model.Architecture(**PARITY).to(device).train()
    (l_ref, g_ref), (l_perm, g_perm) = _eager_step(net, dd.collate(ids)), _eager_step(net, dd.collate(ids[rng.permutation(B8)]))
    l_pad, g_pad = _eager_step(net, pb.load(ids), B8)
    _within(l_pad, l_ref, l_perm, "loss")
    for (name, _p), a, r, q in zip(net.named_parameters(), g_pad, g_ref, g_perm):
        _within(a, r, q, f"grad {name}")


def _replay(device, net, steps=6):
    """``steps`` loads of different shuffled ids through ONE PaddedBatch and one stepper whose optimizer never moves the parameters: eager,
    capture, replays — each against an eager step on ``collate`` of that step's ids."""
    dd = _dataset(device)
    pb = dd.padded(B8)
    stepper = graphs.GraphedTrainStep(net, optim.Adam(net.parameters(), lr=0.0, capturable=True), graphs.padded_loss(_mse))
    rng = np.random.default_rng(9)
    names = [n for n, _ in net.named_parameters()]
    for k in range(steps):
        ids = rng.permutation(40)[:B8]
        (l_ref, g_ref), (l_perm, g_perm) = _eager_step(net, dd.collate(ids)), _eager_step(net, dd.collate(ids[rng.permutation(B8)]))
        loss = stepper(pb.load(ids, launch=k % 2 == 0))       # (both ways: launched by load, or left to the step)
        _within(loss, l_ref, l_perm, f"step {k + 1} loss")
        for name, p, r, q in zip(names, net.parameters(), g_ref, g_perm):
            _within(p.grad, r, q, f"step {k + 1} grad {name}")
    assert stepper.graphs() == 1


def test_replay_follows_every_reload(device):
    torch.manual_seed(0)
    _replay(device, model.Architecture(**PARITY).to(device).train())


def test_replay_with_nnconv(device):
    torch.manual_seed(0)
    _replay(device, model.Architecture(**dict(PARITY, mol_block="_NNConv")).to(device).train())


def test_replay_on_the_general_kernels(device, monkeypatch):
    monkeypatch.setattr(ops, "WS_ROUTE", "0")
    torch.manual_seed(0)
    _replay(device, model.Architecture(**PARITY).to(device).train())


def test_training_mode_smoke_with_the_references_defaults(device):
    dd = _dataset(device)
    pb = dd.padded(B8)
    torch.manual_seed(0)
    net = model.Architecture().to(device).train()               # RReLU, Dropout(0.2), _NNConv
    stepper = graphs.GraphedTrainStep(net, optim.Adam(net.parameters(), lr=1e-3, capturable=True), graphs.padded_loss(_mse))
    rng = np.random.default_rng(10)
    losses = torch.stack([stepper(pb.load(rng.permutation(40)[:B8], launch=False)) for _ in range(10)])
    assert bool(torch.isfinite(losses).all()) and stepper.graphs() == 1
    with torch.no_grad():
        out = net.eval()(pb.load(np.arange(B8)))
    assert out.shape == (B8 + 1, 1) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("kw,named", [(dict(graph_norm="_BatchNorm"), "mol_conv.norm"), (dict(mol_block="_GCNConv"), "mol_conv.conv"),
                                      (dict(flat_norm="_LayerNorm"), "mol_flat.norm")])
def test_models_that_mix_graphs_are_refused_on_the_first_padded_step(device, kw, named):
    dd = _dataset(device)
    pb = dd.padded(B8).load(np.arange(B8), launch=False)
    net = model.Architecture(**dict(PARITY, **kw)).to(device).train()
    stepper = graphs.GraphedTrainStep(net, optim.Adam(net.parameters(), lr=0.0, capturable=True), graphs.padded_loss(_mse))
    with pytest.raises(ValueError, match=named.replace(".", r"\.")):
        stepper(pb)
    assert all(not m._forward_pre_hooks for m in net.modules())
    stepper(dd.collate(np.arange(B8)))                          # the same model on an ordinary batch: as before
