"""CPU: the host side of fixed-capacity batches — the capacity rule, the phantom layout's restatement against a brute-force
grouping, the C ABI's argument checks and every refusal that is decided before a device call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from glam_amd import _lib, graphs, model
from glam_amd.data import DataLoader, padded_bucket, padded_capacity, padded_fit, synth_molecule
from tests.conftest import ROOT
from tests.padded_restated import phantom_layout, stable_grouping

FIELDS = 17


def _vectors(name):
    rng = np.random.default_rng(17)
    if name == "molecules":
        ns = rng.integers(12, 29, 300)
        return ns, 2 * (ns - 1 + rng.integers(1, 3, 300))
    if name == "edgeless-giant":                # one graph with many nodes and no edges among small dense ones
        ns = rng.integers(2, 6, 60)
        es = 4 * ns
        ns[7], es[7] = 500, 0
        return ns, es
    if name == "all-equal":
        return np.full(50, 9), np.full(50, 36)
    if name == "dense-and-sparse":              # degree-4 graphs next to paths: 4 n - e ranges from 0 to 4 n
        ns = rng.integers(1, 40, 120)
        return ns, np.where(rng.random(120) < 0.5, 4 * ns, 2 * (ns - 1))
    raise KeyError(name)


@pytest.mark.parametrize("ell", [False, True])
@pytest.mark.parametrize("name", ["molecules", "edgeless-giant", "all-equal", "dense-and-sparse"])
def test_capacity_holds_every_subset_without_repetition(name, ell):
    ns, es = _vectors(name)
    rng = np.random.default_rng(5)
    for B in (1, 8, 32, len(ns)):               # (B = the dataset: one subset, which attains E_cap)
        n_cap, e_cap = padded_capacity(ns, es, B, ell)
        assert e_cap == np.sort(es)[-B:].sum() and n_cap >= np.sort(ns)[-B:].sum() + 1
        for _ in range(200 if B < len(ns) else 1):
            ids = rng.permutation(len(ns))[:B]
            N, E = int(ns[ids].sum()), int(es[ids].sum())
            assert N <= n_cap - 1 and E <= e_cap, (name, B)
            if ell:
                assert 4 * (n_cap - N) >= e_cap - E, (name, B)
            padded_fit(B, B, N, E, n_cap, e_cap, ell)       # ... and load() agrees
        # the worst subsets by each criterion, not left to chance
        for order in (np.argsort(-ns, kind="stable"), np.argsort(-es, kind="stable"), np.argsort(-(4 * ns - es), kind="stable")):
            N, E = int(ns[order[:B]].sum()), int(es[order[:B]].sum())
            assert N <= n_cap - 1 and E <= e_cap and (not ell or 4 * (n_cap - N) >= e_cap - E), (name, B)
    if not ell:
        assert padded_capacity(ns, es, 8, False)[0] == np.sort(ns)[-8:].sum() + 1        # without an ELL form one phantom node suffices
    for B in (0, len(ns) + 1):
        with pytest.raises(ValueError, match="distinct graphs"):
            padded_capacity(ns, es, B, ell)


@pytest.mark.parametrize("N,E,N_cap,E_cap", [(10, 24, 11, 28), (10, 24, 30, 31), (10, 24, 12, 24), (7, 0, 9, 13), (0, 0, 3, 7), (5, 8, 6, 8),
                                              (20, 40, 23, 52), (20, 40, 22, 57)])
def test_phantom_layout_is_the_stable_grouping_of_the_padded_edge_list(N, E, N_cap, E_cap):
    lay = phantom_layout(N, E, N_cap, E_cap)
    P, E_pad = N_cap - N, E_cap - E
    assert lay["lens"].sum() == E_pad and lay["lens"].max() - lay["lens"].min() <= 1 and (np.diff(lay["lens"]) <= 0).all()
    assert np.array_equal(lay["starts"], E + np.concatenate([[0], np.cumsum(lay["lens"])[:-1]]))
    # a real part whose edges all point at real nodes: a ring over the real nodes, E edges (any would do: the tail only needs them in front)
    real = np.stack([np.arange(E) % max(N, 1), (np.arange(E) + 1) % max(N, 1)]).astype(np.int64)
    ei = np.concatenate([real, lay["edge_index"]], 1)
    assert ei.shape == (2, E_cap) and (lay["edge_index"] >= N).all() and (lay["edge_index"] < N_cap).all()
    for keys, other in ((ei[1], ei[0]), (ei[0], ei[1])):                # by target, by source: the tail is the same
        rowptr, srt, eid = stable_grouping(keys, other, N_cap)
        assert np.array_equal(rowptr[N:], lay["rowptr"])
        assert np.array_equal(srt[E:], lay["src"]) and np.array_equal(eid[E:], lay["eid"])
        if lay["ell_nodes"] is not None:
            for p in range(P):
                a, b = rowptr[N + p], rowptr[N + p + 1]
                assert lay["ell_nodes"][p].tolist() == srt[a:b].tolist() + [-1] * (4 - (b - a))
                assert lay["ell_edges"][p].tolist() == eid[a:b].tolist() + [-1] * (4 - (b - a))
    assert (lay["ell_nodes"] is None) == (E_pad > 4 * P)


def test_bucket_and_load_refusals_decided_on_the_host():
    ns, es, ones = np.array([3, 5, 2, 4]), np.array([4, 8, 2, 6]), np.ones(4, dtype=np.int64)
    assert padded_bucket(ns, es, ones, 2, None, True) == (*padded_capacity(ns, es, 2, True), 1)
    assert padded_bucket(ns, es, 2 * ones, 2, (12, 20), False) == (12, 20, 2)
    for y_rows in (np.array([1, 2, 1, 1]), np.zeros(4, dtype=np.int64), np.zeros(0)):       # y rows differ / no y at all
        with pytest.raises(ValueError, match="y rows"):
            padded_bucket(ns, es, y_rows, 2, None, True)
    for capacity in ((5, 20), (12, 7)):                     # the largest graph (5 nodes + the phantom node, 8 edges) does not fit
        with pytest.raises(ValueError, match="largest graph"):
            padded_bucket(ns, es, ones, 2, capacity, False)
    n_cap, e_cap = padded_capacity(ns, es, 2, True)         # (10, 14)
    padded_fit(2, 2, 9, 14, n_cap, e_cap, True)
    with pytest.raises(ValueError, match="exactly 2 graphs"):
        padded_fit(2, 3, 9, 12, n_cap, e_cap, True)
    with pytest.raises(ValueError, match="exceed the capacity"):      # graph 1 twice: 10 nodes leave no phantom node
        padded_fit(2, 2, 10, 16, n_cap, e_cap, True)
    with pytest.raises(ValueError, match="exceed the capacity"):
        padded_fit(2, 2, 4, e_cap + 1, n_cap, e_cap, False)
    with pytest.raises(ValueError, match="degree 4"):                 # one phantom node would carry 6 self-loops
        padded_fit(2, 2, n_cap - 1, e_cap - 6, n_cap, e_cap, True)
    padded_fit(2, 2, n_cap - 1, e_cap - 6, n_cap, e_cap, False)       # ... which only the ELL form minds


def test_loader_keywords():
    rng = np.random.default_rng(0)
    mols = [synth_molecule(rng) for _ in range(4)]
    with pytest.raises(ValueError, match="resident=True"):
        DataLoader(mols, batch_size=2, padded=True)
    with pytest.raises(ValueError, match="nothing to cache"):
        DataLoader(mols, batch_size=2, device="cuda", resident=True, padded=True, cache=True)
    assert DataLoader(mols, batch_size=2, device="cuda", resident=True, padded=True).cache is False
    assert DataLoader(mols, batch_size=2).padded is False


def test_padded_loss_slices_only_padded_batches():
    seen = []
    loss = graphs.padded_loss(lambda out, batch: seen.append(out) or out.sum())
    out = torch.arange(6.0).view(3, 2)

    class _B:
        pass
    plain, padded = _B(), _B()
    padded.num_real_graphs = 2
    assert float(loss(out, plain)) == 15.0 and seen[-1] is out
    assert float(loss(out, padded)) == 6.0 and seen[-1].shape == (2, 2)


@pytest.mark.parametrize("kw,named", [(dict(graph_norm="_BatchNorm"), "mol_conv.norm"), (dict(pre_norm="_BatchNorm"), "mol_lin0.norm"),
                                      (dict(mol_block="_GCNConv"), "mol_conv.conv"), (dict(mol_block="_GATConv"), "mol_conv.conv"),
                                      (dict(graph_norm="_GraphSizeNorm"), "mol_conv.norm")])
def test_admission_refuses_by_the_module_tree(kw, named):
    with pytest.raises(ValueError, match=named.replace(".", r"\.")):
        graphs.padded_admission(model.Architecture(**kw))


def test_admission_refuses_a_norm_called_without_its_batch_vector():
    x, batch = torch.randn(6, 60), torch.tensor([0, 0, 0, 1, 1, 1])
    for kw, named in ((dict(flat_norm="_LayerNorm"), "mol_flat.norm"), (dict(end_norm="_PairNorm"), "lin_out1.norm")):
        net = model.Architecture(**kw)
        norm = net.get_submodule(named)
        with graphs.padded_admission(net):
            with pytest.raises(ValueError, match=named.replace(".", r"\.")):
                norm(torch.randn(6, norm.norm.in_channels if hasattr(norm.norm, "in_channels") else 8))
        assert not norm._forward_pre_hooks                  # the check leaves nothing behind
    # the per-graph call of the same classes is admitted, as are the reference's defaults
    net = model.Architecture(graph_norm="_PairNorm", pre_norm="_LayerNorm")
    with graphs.padded_admission(net) as adm:
        assert len(adm._norms) == 2
        for _name, m in adm._norms:
            (hook,) = m._forward_pre_hooks.values()
            assert hook(m, (x, batch), {}) is None and hook(m, (x,), {"batch": batch}) is None
    graphs.padded_admission(model.Architecture())


def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    lib = _lib.load()
    assert "glam_collate_padded(" in header and "glam_collate_padded" in _lib.SIGNATURES and hasattr(lib, "glam_collate_padded")
    assert _lib.ABI_VERSION == lib.glam_abi_version() == 4          # a new entry point: no exported signature changed
    assert _lib.api().glam_collate_padded.errcheck is not None and "glam_collate_padded" not in _lib.VALUE_RETURNS


def test_abi_rejects_bad_arguments_before_any_device_work():
    """Every call fails a check that runs BEFORE the launch (made-up addresses that nothing dereferences)."""
    raw = _lib.load()
    good = [0x10000 * (i + 1) for i in range(FIELDS)]
    ptrs = lambda v: (ctypes.c_void_p * FIELDS)(*v)         # noqa: E731
    ds, out, table = ptrs(good), ptrs(good), ctypes.c_void_p(0x900000)
    sizes = (4, 12, 24, 1, 30, 60, 64, 16, 4)               # B, N_cap, E_cap, y rows per graph, Ed, row bytes x / x stride / edge_attr / y

    def call(ds=ds, out=out, table=table, sizes=sizes):
        return raw.glam_collate_padded(ds, out, table, *sizes, None)

    def with_(i, v):
        return sizes[:i] + (v,) + sizes[i + 1:]

    for kw in (dict(ds=None), dict(out=None), dict(table=None)):
        assert call(**kw) == _lib.GLAM_E_INVALID and b"null pointer" in raw.glam_last_error()
    for i, v in ((0, 0), (0, -1), (0, 2 ** 31), (1, 0), (1, 2 ** 31), (2, -1), (2, 2 ** 31)):        # B, N_cap, E_cap out of range
        assert call(sizes=with_(i, v)) == _lib.GLAM_E_INVALID and b"out of range" in raw.glam_last_error(), (i, v)
    for r in (0, -2):                                       # y given, rows per graph not positive
        assert call(sizes=with_(3, r)) == _lib.GLAM_E_INVALID and b"positive integer" in raw.glam_last_error()
    for stride in (56, 60, 72):                             # below the row, or no multiple of 16
        assert call(sizes=with_(6, stride)) == _lib.GLAM_E_INVALID and b"multiple of 16" in raw.glam_last_error()
    assert call(sizes=with_(4, 0)) == _lib.GLAM_E_INVALID and b"edge row 0" in raw.glam_last_error()    # phantom edges need a row to copy
    assert call(sizes=with_(5, 62)) == _lib.GLAM_E_INVALID and b"multiples of 4" in raw.glam_last_error()
    for field in (4, 5, 6, 7, 10, 0, 1, 8, 12, 2):
        vals = list(good)
        vals[field] = None
        assert call(out=ptrs(vals)) == _lib.GLAM_E_INVALID and b"null pointer" in raw.glam_last_error(), field
    vals = list(good)
    vals[0] += 4                                            # the padded x rows start on 16 bytes
    assert call(out=ptrs(vals)) == _lib.GLAM_E_INVALID
    vals = list(good)
    vals[16] = None
    assert call(out=ptrs(vals)) == _lib.GLAM_E_INVALID and b"ELL pair" in raw.glam_last_error()
    assert call(sizes=with_(1, 2 ** 30)) == _lib.GLAM_E_UNSUPPORTED and b"2^31" in raw.glam_last_error()
    with pytest.raises(_lib.GlamHipError, match=r"^glam_collate_padded failed \(code -1\): "):
        _lib.api().glam_collate_padded(None, None, None, *sizes, None)
