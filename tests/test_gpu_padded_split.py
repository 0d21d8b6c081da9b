"""GPU: fixed-capacity resident batches whose surplus nodes are cut into bounded phantom graphs (``phantom_rows``).
Collation is compared exactly — the real part against ``DeviceDataset.collate``, the tails against the numpy restatement
(tests/padded_split_restated.py), the whole index and the segment pointer against the existing builders.  Floating-point results are held
to the yardstick of tests/test_gpu_padded.py: ``4 x max(d_perm, 2^-20)`` with ``d_perm`` measured live per quantity from ``collate(ids)``
against ``collate(permuted ids)``.  The molecules, the model settings and the comparison helpers are that module's."""
import numpy as np
import pytest
import torch

from glam_amd import _lib, graphs, model, ops, optim
from glam_amd.data import DeviceDataset, PaddedBatch, synth_protein
from tests.padded_split_restated import split_layout
from tests.test_gpu_padded import B8, PARITY, _dataset, _eager_step, _mols, _mse, _same, _sizes, _star6, _tiny_graphs, _within

pytestmark = pytest.mark.gpu

M4 = 4
PAIRNORM = dict(PARITY, graph_norm="_PairNorm")         # the per-graph norm: the kernel family that one large phantom graph slows down


def _check_split_load(dd, pb, ids, what, load=True):
    """``pb.load(ids)`` (``load=False``: the caller has loaded them): real part == ``dd.collate(ids)``, tails == the restatement, installed
    index and segment pointer == what the existing builders make of the padded tensors, both found without a build."""
    dev = dd.device
    ref = dd.collate(ids)
    if load:
        pb.load(ids)
    B, N, E = len(ids), ref.x.size(0), ref.edge_index.size(1)
    N_cap, E_cap = pb.capacity
    K, m = pb.num_phantom_graphs, pb.phantom_rows
    P = N_cap - N
    assert K <= P <= K * m, f"{what}: {P} surplus nodes on {K} phantom graphs of 1 .. {m}"
    lay = split_layout(N, E, N_cap, E_cap, B, K)
    t = lambda a, dtype: torch.as_tensor(a, dtype=dtype, device=dev)       # noqa: E731
    assert pb.num_graphs == B + K and pb.num_real_graphs == B
    assert pb.x.shape == (N_cap,) + ref.x.shape[1:] and pb.edge_index.shape == (2, E_cap) and pb.batch.shape == (N_cap,) and pb.ptr.shape == (B + K + 1,)
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
    _same(pb.batch[N:], t(lay["batch"], torch.int64), f"{what} phantom batch")
    _same(pb.ptr[:B + 1], ref.ptr, f"{what} ptr")
    _same(pb.ptr[B:], t(lay["ptr"], torch.int64), f"{what} phantom ptr")
    counts = torch.bincount(pb.batch[N:] - B, minlength=K)
    assert counts.numel() == K and int(counts.min()) >= 1 and int(counts.max()) <= m, f"{what}: every phantom graph has 1 .. {m} nodes"
    for f in ("edge_index", "batch"):
        assert getattr(pb, f)._glam_trusted == getattr(pb, f)._version, f"{what} {f} mark"
    # the installed index and segment pointer: cache hits, not builds
    hit = ops._GI_CACHE.get(pb.edge_index)
    gi = ops.graph_index(pb.edge_index, N_cap)
    assert hit is not None and gi is hit[1] and (gi.N, gi.E) == (N_cap, E_cap), what
    sp = ops.segment_ptr(pb.batch, B + K)
    assert sp is ops._SP_CACHE.get(pb.batch) and (sp.N, sp.B) == (N_cap, B + K), what
    # ... whose tails are the restatement
    for (ptr_p, nbr_p, eid_p), part in (((gi.rowptr, gi.src, gi.eid), "by target"), (gi.transpose(), "by source")):
        _same(ptr_p[N:], t(lay["rowptr"], torch.int32), f"{what} {part} phantom pointer")
        _same(nbr_p[E:], t(lay["src"], torch.int32), f"{what} {part} phantom neighbours")
        _same(eid_p[E:], t(lay["eid"], torch.int32), f"{what} {part} phantom edge ids")
    has_ell = dd.ell_ok and dd.ell_t_ok
    for got, part in ((gi.ell(), "ell"), (gi.ell_t(), "ell_t")):
        if not has_ell:
            assert got is None, f"{what} {part}"
            continue
        _same(got[0][N:], t(lay["ell_nodes"], torch.int32), f"{what} {part} phantom nodes")
        _same(got[1][N:], t(lay["ell_edges"], torch.int32), f"{what} {part} phantom edges")
    # ... and the whole of them what the existing builders make of the padded edge list and batch vector
    whole = ops.GraphIndex(pb.edge_index.clone(), N_cap)
    for got, want, part in zip((gi.rowptr, gi.src, gi.eid) + gi.transpose(), (whole.rowptr, whole.src, whole.eid) + whole.transpose(),
                               ("rowptr", "src", "eid", "colptr", "dst", "eid_t")):
        _same(got, want, f"{what} built {part}")
    for got, want, part in ((gi.ell(), whole.ell(), "ell"), (gi.ell_t(), whole.ell_t(), "ell_t")):
        assert (got is None) == (want is None) == (not has_ell), f"{what} built {part}"
        if has_ell:
            _same(got[0], want[0], f"{what} built {part} nodes")
            _same(got[1], want[1], f"{what} built {part} edges")
    _same(sp.ptr, ops.SegmentPtr(pb.batch.clone(), B + K).ptr, f"{what} segment ptr")
    _same(sp.ptr.to(torch.int64), pb.ptr, f"{what} ptr32 == ptr")
    return ref


def _split(dd, B=B8, m=M4, **kw):
    pb = dd.padded(B, phantom_rows=m, **kw)
    assert isinstance(pb, PaddedBatch) and pb.phantom_rows == m
    return pb


def test_bucket_of_the_molecules(device):
    dd = _dataset(device)
    pb = _split(dd)
    K = pb.num_phantom_graphs
    srt = np.sort(dd.ns)
    assert pb.capacity == dd.capacity(B8, phantom_rows=M4) and 10 <= K < 100 and pb.num_graphs == B8 + K
    assert K * M4 >= pb.capacity[0] - int(srt[:B8].sum()) > (K - 1) * M4 and pb.capacity[0] >= int(srt[-B8:].sum()) + K
    single = dd.padded(B8)                                  # without the keyword: one phantom graph, today's capacity
    assert (single.num_graphs, single.num_phantom_graphs, single.phantom_rows) == (B8 + 1, 1, None) and single.capacity == dd.capacity(B8)
    assert single.capacity[0] == max(int(srt[-B8:].sum()) + 1, -(-(single.capacity[1] + int(np.sort(4 * dd.ns - dd.es)[-B8:].sum())) // 4))


def test_collate_random_batch(device):
    dd = _dataset(device)
    _check_split_load(dd, _split(dd), np.random.default_rng(1).permutation(40)[:B8], "random")


def test_collate_largest_and_smallest_graphs(device):
    dd = _dataset(device)
    pb = _split(dd)
    order = np.argsort(dd.ns, kind="stable")
    big, small = order[-B8:], order[:B8]
    K, N_cap = pb.num_phantom_graphs, pb.capacity[0]
    assert N_cap - _sizes(dd, big)[0] == K, "the B largest graphs leave one node for every phantom graph"
    _check_split_load(dd, pb, big, "P = K")
    assert bool((torch.bincount(pb.batch[_sizes(dd, big)[0]:] - B8) == 1).all())
    assert (K - 1) * M4 < N_cap - _sizes(dd, small)[0] <= K * M4, "the B smallest graphs leave the largest surplus"
    _check_split_load(dd, pb, small, "P at its maximum")


def test_collate_surplus_that_k_does_not_divide(device):
    dd = _dataset(device)
    pb = _split(dd)
    K, N_cap = pb.num_phantom_graphs, pb.capacity[0]
    rng = np.random.default_rng(3)
    ids = next(i for i in (rng.permutation(40)[:B8] for _ in range(100)) if (N_cap - _sizes(dd, i)[0]) % K != 0)
    _check_split_load(dd, pb, ids, "P % K != 0")


def test_second_smaller_load_leaves_no_residue(device):
    dd = _dataset(device)
    pb = _split(dd)
    order = np.argsort(dd.ns, kind="stable")
    big, small = order[-B8:], order[:B8]
    pb.load(big)
    pb.load(small)
    _check_split_load(dd, pb, small, "second, smaller load", load=False)
    pb.load_many([big, small, big[::-1]])                     # ... and the same through the uploaded tables of an epoch
    for step, ids in ((0, big), (1, small), (2, big[::-1])):
        pb.load(step=step)
        _check_split_load(dd, pb, ids, f"load_many step {step}", load=False)


def test_collate_table_beyond_the_lds_slots(device):
    B = int(_lib.load().glam_collate_lds_slots()) + 1
    dd = DeviceDataset(_tiny_graphs(B + 60), device)
    pb = _split(dd, B=B)
    assert pb.num_phantom_graphs > 1
    _check_split_load(dd, pb, np.random.default_rng(8).permutation(B + 60)[:B], "global-memory table")


def test_collate_dataset_with_a_degree_5_star_has_no_ell_form(device):
    dd = DeviceDataset(list(_mols()[:12]) + [_star6()], device)
    assert not dd.ell_ok and not dd.ell_t_ok
    pb = _split(dd, B=4)
    assert pb.capacity[0] == int(np.sort(dd.ns)[-4:].sum()) + pb.num_phantom_graphs
    _check_split_load(dd, pb, [3, 12, 0, 7], "degree-5 star")
    ids = [3, 12, 0, 7]
    N, E = _sizes(dd, ids)
    pb = _split(dd, B=4, capacity=(N + 9, E + 50))            # an explicit capacity: phantom degrees of 5 and 6 on 9 nodes
    _check_split_load(dd, pb, ids, "degree-5 star, chosen capacity")


def test_collate_protein_records_rows_of_49_padded_to_52(device):
    rng = np.random.default_rng(4)
    dd = DeviceDataset([synth_protein(rng, 20, 40) for _ in range(6)], device)
    pb = _split(dd, B=3)
    assert ops.padded_base(pb.x).shape == (pb.capacity[0], 52) and pb.edge_attr.size(1) == 8 and pb.num_phantom_graphs > 1
    _check_split_load(dd, pb, [4, 0, 2], "proteins")


def test_one_launch_per_load_and_none_for_the_index(device):
    dd = _dataset(device)
    pb = _split(dd)
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
    pb = _split(dd)
    small, large = int(np.argmin(dd.ns)), int(np.argmax(dd.ns))
    with _lib.kernel_timer() as kt:
        with pytest.raises(ValueError, match="surplus nodes exceed"):
            pb.load([small] * B8)                             # below any 8 DISTINCT graphs: P > K m
        with pytest.raises(ValueError, match="capacity"):
            pb.load([large] * B8)                             # above them: P < K
        with pytest.raises(ValueError, match="surplus nodes exceed"):
            pb.load_many([np.arange(B8), [small] * B8])
        with pytest.raises(ValueError, match="exactly 8 graphs"):
            pb.load(np.arange(7))
    assert kt.records() == []
    with pytest.raises(ValueError, match="phantom_rows"):
        dd.padded(B8, phantom_rows=0)
    with pytest.raises(ValueError, match="phantom_rows = 1"):
        dd.padded(B8, phantom_rows=1)
    with pytest.raises(ValueError, match="largest graph"):       # B = 1: K = ceil((max + 3 - min) / 4) > 3 phantom nodes beside the largest graph
        dd.padded(1, capacity=(int(dd.ns.max()) + 3, 10 ** 4), phantom_rows=M4)


# ------------------------------------------------------------------------------------------------------------------------------------
# floating point: the split batch against the unpadded one, within 4 x the unpadded path's own sensitivity to the order of the graphs
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [PARITY, PAIRNORM], ids=["no-norm", "_PairNorm"])
def test_phantom_graphs_do_not_reach_the_real_graphs(device, kw):
    dd = _dataset(device)
    pb = _split(dd)
    rng = np.random.default_rng(5)
    ids = rng.permutation(40)[:B8]
    perm = rng.permutation(B8)
    torch.manual_seed(0)
    net = model.Architecture(**kw).to(device).eval()
    with torch.no_grad():
        ref, permuted = net(dd.collate(ids)), net(dd.collate(ids[perm]))
        out = net(pb.load(ids))
    assert out.shape == (B8 + pb.num_phantom_graphs, 1) and bool(torch.isfinite(out).all()), "every row is finite, the phantom graphs' included"
    inv = torch.as_tensor(np.argsort(perm), device=device)
    _within(out[:B8], ref, permuted[inv], "model output")


@pytest.mark.parametrize("kw", [PARITY, PAIRNORM], ids=["no-norm", "_PairNorm"])
def test_gradients_of_one_training_step(device, kw):
    dd = _dataset(device)
    pb = _split(dd)
    rng = np.random.default_rng(6)
    ids = rng.permutation(40)[:B8]
    torch.manual_seed(0)
    net = model.Architecture(**kw).to(device).train()
    (l_ref, g_ref), (l_perm, g_perm) = _eager_step(net, dd.collate(ids)), _eager_step(net, dd.collate(ids[rng.permutation(B8)]))
    l_pad, g_pad = _eager_step(net, pb.load(ids), B8)
    _within(l_pad, l_ref, l_perm, "loss")
    for (name, _p), a, r, q in zip(net.named_parameters(), g_pad, g_ref, g_perm):
        _within(a, r, q, f"grad {name}")


def test_replay_follows_every_reload(device):
    """Six loads of different shuffled ids through ONE split PaddedBatch and one stepper whose optimizer never moves the parameters: eager,
    capture, replays — each against an eager step on ``collate`` of that step's ids."""
    dd = _dataset(device)
    pb = _split(dd)
    torch.manual_seed(0)
    net = model.Architecture(**PAIRNORM).to(device).train()
    stepper = graphs.GraphedTrainStep(net, optim.Adam(net.parameters(), lr=0.0, capturable=True), graphs.padded_loss(_mse))
    rng = np.random.default_rng(9)
    names = [n for n, _ in net.named_parameters()]
    for k in range(6):
        ids = rng.permutation(40)[:B8]
        (l_ref, g_ref), (l_perm, g_perm) = _eager_step(net, dd.collate(ids)), _eager_step(net, dd.collate(ids[rng.permutation(B8)]))
        loss = stepper(pb.load(ids, launch=k % 2 == 0))       # (both ways: launched by load, or left to the step)
        _within(loss, l_ref, l_perm, f"step {k + 1} loss")
        for name, p, r, q in zip(names, net.parameters(), g_ref, g_perm):
            _within(p.grad, r, q, f"step {k + 1} grad {name}")
    assert stepper.graphs() == 1


@pytest.mark.parametrize("kw,named", [(dict(graph_norm="_BatchNorm"), "mol_conv.norm"), (dict(mol_block="_GCNConv"), "mol_conv.conv"),
                                      (dict(flat_norm="_LayerNorm"), "mol_flat.norm")])
def test_models_that_mix_graphs_are_refused_on_the_first_split_step(device, kw, named):
    dd = _dataset(device)
    pb = _split(dd).load(np.arange(B8), launch=False)
    net = model.Architecture(**dict(PARITY, **kw)).to(device).train()
    stepper = graphs.GraphedTrainStep(net, optim.Adam(net.parameters(), lr=0.0, capturable=True), graphs.padded_loss(_mse))
    with pytest.raises(ValueError, match=named.replace(".", r"\.")):
        stepper(pb)
    assert all(not m._forward_pre_hooks for m in net.modules())
    stepper(dd.collate(np.arange(B8)))                          # the same model on an ordinary batch: as before
