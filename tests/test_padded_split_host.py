"""CPU: the host side of fixed-capacity batches whose surplus is cut into bounded phantom graphs — the capacity rule
against every subset, the restated layout against a brute-force grouping, the C ABI's argument checks and every refusal that is decided
before a device call."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from glam_amd import _lib
from glam_amd.data import DataLoader, padded_bucket, padded_capacity, padded_fit, phantom_graphs, synth_molecule
from tests.conftest import ROOT
from tests.padded_restated import phantom_layout, stable_grouping
from tests.padded_split_restated import split_layout

FIELDS = 17


def _vectors(name):
    """Small (ns, es) with degrees <= 4 (es <= 4 ns), so that both the ELL and the plain rule apply."""
    if name == "mixed":
        return np.array([3, 5, 2, 4, 7, 3, 6, 1]), np.array([4, 8, 2, 6, 12, 12, 10, 0])
    if name == "dense-small-sparse-large":      # the ELL term decides N_cap: the graphs with many edges are not the ones with many nodes
        return np.array([2, 2, 3, 9, 8, 2, 3]), np.array([8, 8, 12, 0, 2, 8, 12])
    if name == "all-equal":
        return np.full(6, 4), np.array([6, 8, 6, 16, 0, 8])
    raise KeyError(name)


def _top(v, B):
    return int(np.sort(v)[-B:].sum())


def _bottom(v, B):
    return int(np.sort(v)[:B].sum())


@pytest.mark.parametrize("ell", [False, True])
@pytest.mark.parametrize("name", ["mixed", "dense-small-sparse-large", "all-equal"])
def test_capacity_holds_every_subset_with_k_bounded_phantom_graphs(name, ell):
    ns, es = _vectors(name)
    for B in (1, 2, 3, len(ns)):
        for m in (1, 2, 3, 4, int(ns.max()), 50):
            if m == 1 and _top(ns, B) != _bottom(ns, B):
                with pytest.raises(ValueError, match="phantom_rows = 1"):
                    padded_capacity(ns, es, B, ell, m)
                continue
            n_cap, e_cap = padded_capacity(ns, es, B, ell, m)
            K = phantom_graphs(ns, B, n_cap, m)
            n_ell = -(-(e_cap + _top(4 * ns - es, B)) // 4) if ell else 0
            assert e_cap == _top(es, B) and n_cap == max(_top(ns, B) + K, n_ell), (name, B, m)
            for ids in itertools.combinations(range(len(ns)), B):
                N, E = int(ns[list(ids)].sum()), int(es[list(ids)].sum())
                P = n_cap - N
                assert K <= P <= K * m and E <= e_cap, (name, B, m, ids)
                if ell:
                    assert 4 * P >= e_cap - E, (name, B, m, ids)
                padded_fit(B, B, N, E, n_cap, e_cap, ell, K, m)        # ... and load() agrees
            if K > 1:       # K is the smallest: with K - 1 phantom graphs the B smallest graphs leave more than (K - 1) m surplus nodes
                assert max(_top(ns, B) + K - 1, n_ell) - _bottom(ns, B) > (K - 1) * m, (name, B, m)
    # one phantom graph may hold everything: the single-phantom capacity, K = 1
    assert padded_capacity(ns, es, 2, ell, 10 ** 6) == padded_capacity(ns, es, 2, ell)
    assert phantom_graphs(ns, 2, padded_capacity(ns, es, 2, ell)[0], 10 ** 6) == 1


def test_none_keeps_the_single_phantom_layout():
    ns, es = _vectors("mixed")
    for B in (1, 3, len(ns)):
        for ell in (False, True):
            n_cap, e_cap = padded_capacity(ns, es, B, ell, None)
            assert (n_cap, e_cap) == padded_capacity(ns, es, B, ell)
            assert n_cap == max(_top(ns, B) + 1, -(-(e_cap + _top(4 * ns - es, B)) // 4) if ell else 0) and e_cap == _top(es, B)
            assert phantom_graphs(ns, B, n_cap, None) == 1          # num_graphs = B + 1
    ones = np.ones(len(ns), dtype=np.int64)
    assert padded_bucket(ns, es, ones, 3, None, True, None) == padded_bucket(ns, es, ones, 3, None, True)
    # ... and K = 1 of the split layout is that layout: every phantom node in graph B, ptr = [N, N_cap]
    lay = split_layout(10, 24, 17, 31, 4, 1)
    assert lay["batch"].tolist() == [4] * 7 and lay["ptr"].tolist() == [10, 17] and lay["counts"].tolist() == [7]
    single = phantom_layout(10, 24, 17, 31)
    assert all(np.array_equal(lay[k], single[k]) for k in single)


@pytest.mark.parametrize("N,E,N_cap,E_cap,B,K", [(10, 24, 17, 31, 4, 3), (10, 24, 17, 31, 4, 7), (10, 24, 17, 52, 4, 2), (0, 0, 5, 7, 1, 2),
                                                (20, 40, 31, 40, 8, 4), (7, 0, 40, 13, 2, 9), (5, 8, 6, 8, 3, 1)])
def test_split_layout_is_non_decreasing_with_the_stated_counts(N, E, N_cap, E_cap, B, K):
    lay = split_layout(N, E, N_cap, E_cap, B, K)
    P = N_cap - N
    s, r = divmod(P, K)
    batch, ptr, counts = lay["batch"], lay["ptr"], lay["counts"]
    assert batch.shape == (P,) and (np.diff(batch) >= 0).all() and batch[0] == B and batch[-1] == B + K - 1
    assert np.array_equal(np.bincount(batch - B, minlength=K), counts) and counts.sum() == P
    assert counts.min() >= 1 and counts.max() - counts.min() <= 1 and (np.diff(counts) <= 0).all() and counts.max() == s + (r > 0)
    assert np.array_equal(ptr, N + np.concatenate([[0], np.cumsum(counts)])) and ptr[0] == N and ptr[K] == N_cap
    # the closed form the kernel evaluates: the divmod idiom of the edge runs, restated over nodes
    p = np.arange(P)
    head = r * (s + 1)
    assert np.array_equal(batch, B + np.where(p < head, p // (s + 1), r + (p - head) // max(s, 1)))
    # the cut moves no edge: the index is the brute-force stable grouping of the padded edge list, as for one phantom graph
    real = np.stack([np.arange(E) % max(N, 1), (np.arange(E) + 1) % max(N, 1)]).astype(np.int64)
    ei = np.concatenate([real, lay["edge_index"]], 1)
    for keys, other in ((ei[1], ei[0]), (ei[0], ei[1])):
        rowptr, srt, eid = stable_grouping(keys, other, N_cap)
        assert np.array_equal(rowptr[N:], lay["rowptr"]) and np.array_equal(srt[E:], lay["src"]) and np.array_equal(eid[E:], lay["eid"])
        if lay["ell_nodes"] is not None:
            for q in range(P):
                a, b = rowptr[N + q], rowptr[N + q + 1]
                assert lay["ell_nodes"][q].tolist() == srt[a:b].tolist() + [-1] * (4 - (b - a))
                assert lay["ell_edges"][q].tolist() == eid[a:b].tolist() + [-1] * (4 - (b - a))
    # every phantom edge stays inside its owner's phantom graph
    assert np.array_equal(batch[lay["edge_index"][0] - N], batch[lay["edge_index"][1] - N])


def test_refusals_decided_on_the_host():
    ns, es, ones = np.array([3, 5, 2, 4]), np.array([4, 8, 2, 6]), np.ones(4, dtype=np.int64)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="phantom_rows"):
            padded_capacity(ns, es, 2, True, bad)
        with pytest.raises(ValueError, match="phantom_rows"):
            padded_bucket(ns, es, ones, 2, None, True, bad)
    with pytest.raises(ValueError, match="phantom_rows = 1"):           # unequal sizes: no fixed K gives every surplus node its own graph
        padded_capacity(ns, es, 2, False, 1)
    assert padded_capacity(np.full(4, 3), es, 2, False, 1) == (7, 14)   # equal sizes: K = 1 node, P = 1 always
    # an explicit capacity: K = ceil((N_cap - botB) / m), one node each beside the largest graph
    assert padded_bucket(ns, es, ones, 2, (12, 20), False, 4) == (12, 20, 1) and phantom_graphs(ns, 2, 12, 4) == 2        # (12 - 5) / 4
    with pytest.raises(ValueError, match="largest graph"):              # B = 1, botB = 2: K = 6 phantom nodes + 5 > 8
        padded_bucket(ns, es, ones, 1, (8, 20), False, 1)
    with pytest.raises(ValueError, match="largest graph"):
        padded_bucket(ns, es, ones, 2, (12, 7), False, 4)
    with pytest.raises(ValueError, match="distinct graphs"):
        padded_bucket(ns, es, ones, 5, (40, 40), False, 4)
    # repeated ids against the bucket of any 2 DISTINCT graphs with m = 2
    n_cap, e_cap = padded_capacity(ns, es, 2, False, 2)
    K = phantom_graphs(ns, 2, n_cap, 2)
    assert (n_cap, K) == (9 + K, 4) and K * 2 >= n_cap - 5 > (K - 1) * 2
    padded_fit(2, 2, 9, 14, n_cap, e_cap, False, K, 2)                  # the two largest: P = K
    padded_fit(2, 2, 5, 6, n_cap, e_cap, False, K, 2)                   # the two smallest: P = K m
    with pytest.raises(ValueError, match="exceed the capacity"):        # graph 1 twice: 10 nodes leave 3 phantom nodes for 4 phantom graphs
        padded_fit(2, 2, 10, 16, n_cap, e_cap, False, K, 2)
    with pytest.raises(ValueError, match="surplus nodes exceed"):       # graph 2 twice: 9 surplus nodes on 4 phantom graphs of 2
        padded_fit(2, 2, 4, 4, n_cap, e_cap, False, K, 2)
    padded_fit(2, 2, 4, 4, n_cap, e_cap, False)                         # ... which only the bounded mode minds
    with pytest.raises(ValueError, match="exactly 2 graphs"):
        padded_fit(2, 3, 9, 12, n_cap, e_cap, False, K, 2)


def test_loader_keyword():
    rng = np.random.default_rng(0)
    mols = [synth_molecule(rng) for _ in range(4)]
    with pytest.raises(ValueError, match="padded=True"):
        DataLoader(mols, batch_size=2, device="cuda", resident=True, phantom_rows=8)
    with pytest.raises(ValueError, match="phantom_rows"):
        DataLoader(mols, batch_size=2, device="cuda", resident=True, padded=True, phantom_rows=0)
    assert DataLoader(mols, batch_size=2, device="cuda", resident=True, padded=True, phantom_rows=8).phantom_rows == 8
    assert DataLoader(mols, batch_size=2, device="cuda", resident=True, padded=True).phantom_rows is None


def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    lib = _lib.load()
    assert "glam_collate_padded_split(" in header and "glam_collate_padded_split" in _lib.SIGNATURES and hasattr(lib, "glam_collate_padded_split")
    assert _lib.ABI_VERSION == lib.glam_abi_version() == 4          # a new entry point: no exported signature changed
    split, single = _lib.SIGNATURES["glam_collate_padded_split"], _lib.SIGNATURES["glam_collate_padded"]
    assert split[0] == single[0] and split[1][:4] + split[1][5:] == single[1] and split[1][4] == ctypes.c_int64      # the same, plus K
    assert _lib.api().glam_collate_padded_split.errcheck is not None and "glam_collate_padded_split" not in _lib.VALUE_RETURNS


def test_abi_rejects_bad_arguments_before_any_device_work():
    """Every call fails a check that runs BEFORE the launch (made-up addresses that nothing dereferences)."""
    raw = _lib.load()
    good = [0x10000 * (i + 1) for i in range(FIELDS)]
    ptrs = lambda v: (ctypes.c_void_p * FIELDS)(*v)         # noqa: E731
    ds, out, table = ptrs(good), ptrs(good), ctypes.c_void_p(0x900000)
    sizes = (4, 3, 12, 24, 1, 30, 60, 64, 16, 4)            # B, K, N_cap, E_cap, y rows per graph, Ed, row bytes x / x stride / edge_attr / y

    def call(ds=ds, out=out, table=table, sizes=sizes):
        return raw.glam_collate_padded_split(ds, out, table, *sizes, None)

    def with_(i, v):
        return sizes[:i] + (v,) + sizes[i + 1:]

    for K in (0, -1, 13, 2 ** 31):                          # K < 1, N_cap < K, B + K beyond int32
        assert call(sizes=with_(1, K)) == _lib.GLAM_E_INVALID and b"K out of range" in raw.glam_last_error(), K
    assert call(sizes=with_(2, 2)) == _lib.GLAM_E_INVALID and b"K out of range" in raw.glam_last_error()        # N_cap = 2 < K = 3
    # ... plus every check of glam_collate_padded
    for kw in (dict(ds=None), dict(out=None), dict(table=None)):
        assert call(**kw) == _lib.GLAM_E_INVALID and b"null pointer" in raw.glam_last_error()
    for i, v in ((0, 0), (0, -1), (0, 2 ** 31), (2, 0), (2, 2 ** 31), (3, -1), (3, 2 ** 31)):          # B, N_cap, E_cap out of range
        assert call(sizes=with_(i, v)) == _lib.GLAM_E_INVALID and b"out of range" in raw.glam_last_error(), (i, v)
    for r in (0, -2):
        assert call(sizes=with_(4, r)) == _lib.GLAM_E_INVALID and b"positive integer" in raw.glam_last_error()
    for stride in (56, 60, 72):
        assert call(sizes=with_(7, stride)) == _lib.GLAM_E_INVALID and b"multiple of 16" in raw.glam_last_error()
    assert call(sizes=with_(5, 0)) == _lib.GLAM_E_INVALID and b"edge row 0" in raw.glam_last_error()
    assert call(sizes=with_(6, 62)) == _lib.GLAM_E_INVALID and b"multiples of 4" in raw.glam_last_error()
    for field in (4, 5, 6, 7, 10, 0, 1, 8, 12, 2):
        vals = list(good)
        vals[field] = None
        assert call(out=ptrs(vals)) == _lib.GLAM_E_INVALID and b"null pointer" in raw.glam_last_error(), field
    vals = list(good)
    vals[16] = None
    assert call(out=ptrs(vals)) == _lib.GLAM_E_INVALID and b"ELL pair" in raw.glam_last_error()
    assert call(sizes=with_(2, 2 ** 30)) == _lib.GLAM_E_UNSUPPORTED and b"2^31" in raw.glam_last_error()
    with pytest.raises(_lib.GlamHipError, match=r"^glam_collate_padded_split failed \(code -1\): "):
        _lib.api().glam_collate_padded_split(None, None, None, *sizes, None)
    # the K = 1 entry point rejects what it rejected before: N_cap = 0 leaves no phantom node
    assert raw.glam_collate_padded(ds, out, table, 4, 0, 24, 1, 30, 60, 64, 16, 4, None) == _lib.GLAM_E_INVALID
