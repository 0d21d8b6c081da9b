"""The index kernels against their numpy restatements, exactly: ``glam_csr_build`` and ``glam_batch_ptr`` (csrc/csr.hip) through
``ops.GraphIndex`` / ``ops.SegmentPtr``, ``glam_ell_build`` (csrc/triplet_pipe.hip) through ``GraphIndex.ell()`` / ``ell_t()`` and raw,
``glam_batch_fingerprint`` (csrc/core.hip) through the C ABI.  Every float kernel of the library reads its neighbours through these
tables, and a wrong bit in them is no rounding error downstream: every comparison here is ``torch.equal``.

tests/index_cases.py holds the cases and restatements; tests/test_index_cases_host.py shows on the CPU that the restatements are the
plain loops, that each case reaches the code path it is named for (scan blocks 1 / 2 / 256 / 257, one and two trips of the capped
grids, segment lengths 32 / 33, both directions, both ELL outcomes) and that eleven wrong builders fail on a named case.  Launches
are asserted from ``_lib.kernel_timer()`` (kernel name and grid of every launch of the library)."""
import ctypes
import functools
import gc

import numpy as np
import pytest
import torch

from glam_amd import _lib, ops
from tests import index_cases as I

pytestmark = pytest.mark.gpu


def _equal(dev, ref):
    """A device tensor against a numpy array: same dtype, same shape, same bits."""
    got = dev.cpu()
    want = torch.from_numpy(np.ascontiguousarray(ref))
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


@functools.lru_cache(maxsize=None)
def _built(name):
    """``(edge_index on the device, GraphIndex, its transpose, launches of both builds)`` of a graph case, built once."""
    g = I.graph_case(name)
    ei = g.edge_index.cuda()
    with _lib.kernel_timer() as kt:
        gi = ops.GraphIndex(ei, g.N)
        t = gi.transpose()
    return ei, gi, t, [(n, grid) for n, grid, _ in kt.records()]


def _assert_index(tables, ref, what):
    """``(ptr, nbr, eid)`` device tensors against the restatement: ``ptr`` whole, the first ``ptr[N]`` entries of the other two."""
    ptr, nbr, eid = ref
    V = int(ptr[-1])
    assert _equal(tables[0], ptr), f"{what}: ptr"
    assert _equal(tables[1][:V], nbr), f"{what}: nbr"
    assert _equal(tables[2][:V], eid), f"{what}: eid"


# ---------------------------------------------------------------------------------------------
# CSR
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.GRAPH_CASES)
def test_csr_is_the_stable_sort(device, name):
    g = I.graph_case(name)
    ei, gi, t, launches = _built(name)
    assert (gi.N, gi.E) == (g.N, g.E) and gi.rowptr.dtype == gi.src.dtype == gi.eid.dtype == torch.int32
    assert gi.src.numel() == g.E == t[1].numel()
    _assert_index((gi.rowptr, gi.src, gi.eid), I.csr_ref(g.edge_index, g.N, 0), f"{name} by target")
    _assert_index(t, I.csr_ref(g.edge_index, g.N, 1), f"{name} by source")
    # a second build from a clone: the atomics of count and fill leave no trace
    again = ops.GraphIndex(ei.clone(), g.N)
    for a, b in zip((gi.rowptr, gi.src, gi.eid) + tuple(t), (again.rowptr, again.src, again.eid) + tuple(again.transpose())):
        assert torch.equal(a, b), f"{name}: two builds differ"
    # the launches of the two builds (by target, by source), with their grids
    scan = [("k_scan_block_sums", I.scan_blocks(g.N)), ("k_scan_top", 1), ("k_scan_apply", I.scan_blocks(g.N))]
    if g.E == 0:
        assert launches == scan * 2, f"{name}: an empty edge list launches the scan alone, got {launches}"
    else:
        edges, nodes = I.grid_for(g.E), I.grid_for(g.N)
        assert launches == ([("k_csr_count", edges)] + scan + [("k_csr_fill", edges), ("k_csr_sort_segments", nodes)]) * 2, launches


def test_the_capped_grids_were_capped(device):
    """The second trips are real: 2 048 blocks for 524 291 edges and for 524 289 nodes, 257 scan blocks behind one ``k_scan_top``."""
    grids = dict(_built("many_edges")[3])
    assert grids["k_csr_count"] == grids["k_csr_fill"] == I.MAX_BLOCKS and I.graph_case("many_edges").E > I.MAX_BLOCKS * I.BLOCK
    grids = dict(_built("second_chunk[524289]")[3])
    assert grids["k_csr_sort_segments"] == I.MAX_BLOCKS and grids["k_scan_apply"] == 257 and grids["k_scan_top"] == 1
    assert dict(_built("second_chunk[524287]")[3])["k_scan_apply"] == 256


@pytest.mark.parametrize("name", ["segment_ladder[shuffled]", "segment_ladder[descending,flip]", "scan_edges[2049]"])
def test_transpose_after_edge_index_was_dropped(device, name):
    """``transpose()`` rebuilds ``edge_index`` from the by-target CSR when the caller's tensor is gone: the same by-source tables."""
    g = I.graph_case(name)
    want = _built(name)[2]
    ei = g.edge_index.to(device)
    gi = ops.GraphIndex(ei, g.N)
    assert gi._ei_ref() is ei
    del ei
    gc.collect()
    assert gi._ei_ref() is None, "the index must not keep edge_index alive"
    got = gi.transpose()
    for a, b, what in zip(got, want, ("colptr", "dst", "eid_t")):
        assert torch.equal(a, b), f"{name}: {what} differs from the transpose taken with the tensor alive"
    _assert_index(got, I.csr_ref(g.edge_index, g.N, 1), f"{name} by source, rebuilt")
    assert gi.transpose() is got


@pytest.mark.parametrize("name", I.BAD_ID_CASES)
def test_bad_ids_raise_or_are_dropped(device, monkeypatch, name):
    g = I.bad_ids()[name]
    monkeypatch.setattr(ops, "VALIDATE", "sync")
    with pytest.raises(IndexError, match="node ids outside"):
        ops.GraphIndex(g.edge_index.to(device), g.N)
    monkeypatch.setattr(ops, "VALIDATE", "off")
    ei = g.edge_index.to(device)
    gi = ops.GraphIndex(ei, g.N)                                      # no exception: the bad edges are skipped by count and fill alike
    _assert_index((gi.rowptr, gi.src, gi.eid), I.csr_ref(g.edge_index, g.N, 0), f"bad_ids[{name}] by target")
    _assert_index(gi.transpose(), I.csr_ref(g.edge_index, g.N, 1), f"bad_ids[{name}] by source")
    assert gi._ei_ref() is ei and int(gi.rowptr[-1]) == g.E - len(g.bad) == int(gi.transpose()[0][-1])
    ops.check_pending()


@pytest.mark.parametrize("name", ["value_row_only", "last_edge", "several"])
def test_transpose_after_a_bad_edge_index_was_dropped(device, monkeypatch, name):
    """An index that outlived a bad ``edge_index`` (``VALIDATE = "off"``, or ``"deferred"`` before the flag is back) holds fewer than ``E``
    entries; the rebuild in ``transpose()`` takes those alone — the entries behind ``rowptr[N]`` were never written and are set to
    edge 0 / node 0 here, which would overwrite a valid edge if they were used — and gives the tables of the valid subset, as with the tensor alive."""
    g = I.bad_ids()[name]
    monkeypatch.setattr(ops, "VALIDATE", "off")
    gi = ops.GraphIndex(g.edge_index.to(device), g.N)                 # (the tensor is a temporary: gone after this line)
    gc.collect()
    assert gi._ei_ref() is None
    V = g.E - len(g.bad)
    assert int(gi.rowptr[-1]) == V
    gi.src[V:] = 0
    gi.eid[V:] = 0
    _assert_index(gi.transpose(), I.csr_ref(g.edge_index, g.N, 1), f"bad_ids[{name}] by source, rebuilt")


# ---------------------------------------------------------------------------------------------
# ELL
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.GRAPH_CASES)
def test_ell_records(device, name):
    """``ell()`` / ``ell_t()``: the restated ``[N, 4]`` records where every degree of that side is at most 4, ``None`` otherwise (and for
    the graph without nodes, which has nothing to build)."""
    g = I.graph_case(name)
    _, gi, t, _ = _built(name)
    for by, got in ((0, gi.ell()), (1, gi.ell_t())):
        nbr, eid, overflow = I.ell_ref(*I.csr_ref(g.edge_index, g.N, by), g.N)
        if overflow or g.N == 0:
            assert got is None, f"{name}: side {by} has a degree above 4"
        else:
            assert got is not None, f"{name}: side {by} has the ELL form"
            assert _equal(got[0], nbr) and _equal(got[1], eid), f"{name}: ELL records of side {by}"
    assert gi.ell() is gi._ell and gi.ell_t() is gi._ell_t            # answered once


@pytest.mark.parametrize("N", I.SECOND_CHUNK_N)
def test_ell_overflow_twin(device, N):
    """One edge more into the last node: no ELL form by target, the by-source form untouched but for that edge; the raw
    ``glam_ell_build`` still writes the first four entries of the overflowing node and raises the flag."""
    name = f"second_chunk[{N},twin]"
    g = I.graph_case(name)
    _, gi, _, _ = _built(name)
    _, plain, _, _ = _built(f"second_chunk[{N}]")
    assert gi.ell() is None and gi.ell_t() is not None and plain.ell() is not None and plain.ell_t() is not None
    changed = (gi.ell_t()[0] != plain.ell_t()[0]).nonzero()
    assert changed[:, 0].tolist() == [g.extra_src]
    lib = _lib.load()
    i32 = dict(dtype=torch.int32, device=device)
    es, ee, ovf = torch.full((N, 4), -7, **i32), torch.full((N, 4), -7, **i32), torch.zeros(1, **i32)
    with _lib.kernel_timer() as kt:
        rc = lib.glam_ell_build(_lib.ptr(gi.rowptr), _lib.ptr(gi.src), _lib.ptr(gi.eid), N, _lib.ptr(es), _lib.ptr(ee), _lib.ptr(ovf), _lib.stream())
    assert rc == 0, lib.glam_last_error()
    assert [(n, grid) for n, grid, _ in kt.records()] == [("k_ell_build", I.grid_for(N))]
    nbr, eid, overflow = I.ell_ref(*I.csr_ref(g.edge_index, N, 0), N)
    assert overflow and int(ovf.item()) == 1
    assert _equal(es, nbr) and _equal(ee, eid)
    assert (es[-1] >= 0).all() and es[-1].tolist() == gi.src[-5:-1].tolist()       # the first four of the five


# ---------------------------------------------------------------------------------------------
# segment pointers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in I.BATCH_CASES.items() if c[2]])
def test_segment_ptr_is_the_restatement(device, name):
    batch, B, _ = I.BATCH_CASES[name]
    ref = I.batch_ptr_ref(batch, B)
    with _lib.kernel_timer() as kt:
        sp = ops.SegmentPtr(torch.from_numpy(batch).to(device), B)
    assert (sp.N, sp.B) == (batch.size, ref.size - 1)
    assert _equal(sp.ptr, ref), name
    assert [(n, grid) for n, grid, _ in kt.records()] == [("k_batch_ptr", I.grid_for(batch.size + 1))]


@pytest.mark.parametrize("name", [n for n, c in I.BATCH_CASES.items() if not c[2]])
def test_segment_ptr_refuses(device, monkeypatch, name):
    batch, B, _ = I.BATCH_CASES[name]
    monkeypatch.setattr(ops, "VALIDATE", "sync")
    with pytest.raises(IndexError, match="non-decreasing"):
        ops.SegmentPtr(torch.from_numpy(batch).to(device), B)


def test_segment_ptr_cache(device):
    batch_np, B, _ = I.BATCH_CASES["N257_empties"]
    batch = torch.from_numpy(batch_np).to(device)
    sp = ops.segment_ptr(batch)
    assert sp.B == int(batch_np[-1]) + 1 and ops.segment_ptr(batch) is sp and ops.segment_ptr(batch, sp.B) is sp
    more = ops.segment_ptr(batch, B)
    assert more is not sp and more.B == B and _equal(more.ptr, I.batch_ptr_ref(batch_np, B))
    assert ops.segment_ptr(batch, B) is more and ops.segment_ptr(batch) is more           # (no count asked: the cached object serves)
    assert _equal(sp.ptr, I.batch_ptr_ref(batch_np, None))
    assert ops.segment_ptr(batch.clone()) is not more


# ---------------------------------------------------------------------------------------------
# fingerprint
# ---------------------------------------------------------------------------------------------
_GARBAGE = 0x5555555555555555


def _fingerprint(tensors, out=None, nbytes=None, n=None):
    """``glam_batch_fingerprint`` through the raw binding: ``(return code, value read back as unsigned, launches)``."""
    lib = _lib.load()
    if out is None:
        out = torch.full((1,), _GARBAGE, dtype=torch.int64, device="cuda")      # the call itself must clear it
    k = len(tensors)
    bufs = (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() for t in tensors])
    sizes = (ctypes.c_int64 * max(k, 1))(*(nbytes if nbytes is not None else [t.numel() * t.element_size() for t in tensors]))
    with _lib.kernel_timer() as kt:
        rc = lib.glam_batch_fingerprint(k if n is None else n, bufs, sizes, ctypes.c_void_p(out.data_ptr()), _lib.stream())
    return rc, int(out.item()) & I.U64, [(name, grid) for name, grid, _ in kt.records()]


def _dev(bufs):
    return [torch.from_numpy(b.view(np.int32)).cuda() for b in bufs]


@pytest.mark.parametrize("name", list(I.FP_CASES))
def test_fingerprint_is_the_restatement(device, name):
    bufs = I.FP_CASES[name]
    total = sum(b.size for b in bufs)
    rc, got, launches = _fingerprint(_dev(bufs))
    assert rc == 0, _lib.load().glam_last_error()
    assert got == I.fingerprint_ref(bufs), f"{name}: {got:#018x} vs {I.fingerprint_ref(bufs):#018x}"
    assert launches == [("k_fingerprint", I.grid_for(total, 4 * I.BLOCK, 256))]


def test_fingerprint_is_position_sensitive(device):
    bufs = I.FP_CASES["total_257_in_4"]
    ref = I.fingerprint_ref(bufs)
    assert bufs[1][3] != bufs[1][40]
    swapped = [b.copy() for b in bufs]
    swapped[1][[3, 40]] = swapped[1][[40, 3]]
    moved = [bufs[0][:-1], np.concatenate([bufs[0][-1:], bufs[1]])] + bufs[2:]   # the boundary one word to the left: the same word stream
    for other in (swapped, moved):
        rc, got, _ = _fingerprint(_dev(other))
        assert rc == 0 and got == I.fingerprint_ref(other) and got != ref
    big = I.FP_CASES["total_262145_in_1"][0]                                     # two words that the SAME thread reads, trips apart
    stride = 256 * I.BLOCK
    assert big.size == 4 * stride + 1 and big[0] != big[4 * stride]           # thread 0 of block 0: its first and fifth trip
    far = big.copy()
    far[[0, 4 * stride]] = far[[4 * stride, 0]]
    rc, got, _ = _fingerprint(_dev([far]))
    assert rc == 0 and got == I.fingerprint_ref([far]) != I.fingerprint_ref([big])


def test_fingerprint_empty_buffer_shifts_the_salts(device):
    values = set()
    for pos in range(4):
        bufs = I.FP_CASES[f"empty_at_{pos}"]
        rc, got, _ = _fingerprint(_dev(bufs))
        assert rc == 0 and got == I.fingerprint_ref(bufs)
        values.add(got)
    assert len(values) == 4
    rc, got, launches = _fingerprint(_dev([np.zeros(0, np.uint32)] * 2))        # nothing to hash: the memset alone
    assert rc == 0 and got == 0 and launches == []


def test_fingerprint_clears_its_output(device):
    bufs = _dev(I.FP_CASES["total_1025_in_3"])
    out = torch.full((1,), _GARBAGE, dtype=torch.int64, device=device)
    rc, first, _ = _fingerprint(bufs, out)
    rc2, second, _ = _fingerprint(bufs, out)                                     # into the same tensor, which now holds `first`
    assert rc == 0 and rc2 == 0 and first == second == I.fingerprint_ref(I.FP_CASES["total_1025_in_3"])


def test_fingerprint_refuses_with_an_error_code(device):
    lib = _lib.load()
    bufs = _dev(I.FP_CASES["total_257_in_4"])
    for kw in (dict(nbytes=[188, 350, 144, 344]), dict(nbytes=[188, 352, 144, 343]), dict(nbytes=[-4, 352, 144, 344]), dict(n=0), dict(n=5)):
        rc, got, launches = _fingerprint(bufs, **kw)
        assert rc != 0 and launches == [], kw
        assert got == _GARBAGE, "a refused call touches nothing"
        assert b"glam_batch_fingerprint" in lib.glam_last_error()
    rc, got, _ = _fingerprint(bufs)                                               # and the next call is fine
    assert rc == 0 and got == I.fingerprint_ref(I.FP_CASES["total_257_in_4"])
