"""CPU: the host side of device-resident datasets — the C ABI of ``glam_collate``, the slot table, id checks, the loader's
``resident`` keyword, and installing an index that already exists (``from_parts``)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from glam_amd import _lib, ops
from glam_amd.data import Data, DataLoader, resident_table, synth_molecule
from tests.conftest import ROOT

FIELDS = 17


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    lib = _lib.load()
    for name in ("glam_collate", "glam_collate_lds_slots"):
        assert name + "(" in header and name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert f"#define GLAM_COLLATE_FIELDS {FIELDS}" in header
    assert "collate.hip" in open(os.path.join(ROOT, "glam_amd", "csrc", "Makefile")).read()
    assert _lib.ABI_VERSION == lib.glam_abi_version() == 4          # new entry points only: no exported signature changed
    assert lib.glam_collate_lds_slots() >= 1024                     # (a B = 1024 batch keeps its table in LDS)
    # a status like every other: the checked view raises by itself
    assert _lib.api().glam_collate.errcheck is not None and "glam_collate" not in _lib.VALUE_RETURNS


def test_slot_table_of_a_hand_written_id_list():
    ns, es, y_rows = np.array([3, 1, 5, 2]), np.array([4, 0, 8, 2]), np.array([1, 2, 1, 3])
    # graph 2 twice, the 0-edge graph 1 in the middle and last
    table, N, E, Y = resident_table([2, 1, 0, 2, 1], ns, es, y_rows)
    assert table.dtype == np.int32 and table.shape == (4, 6)
    assert table[0].tolist() == [2, 1, 0, 2, 1, 0]                  # ids, one entry of padding
    assert table[1].tolist() == [0, 5, 6, 9, 14, 15]                # exclusive node offsets, closed by N
    assert table[2].tolist() == [0, 8, 8, 12, 20, 20]               # the 0-edge graph's slot is empty: it shares its offset
    assert table[3].tolist() == [0, 1, 3, 4, 5, 7]
    assert (N, E, Y) == (15, 20, 7)
    for ids in (torch.tensor([2, 1, 0, 2, 1]), np.array([2, 1, 0, 2, 1], dtype=np.int32), (2, 1, 0, 2, 1)):   # any host sequence
        assert np.array_equal(resident_table(ids, ns, es, y_rows)[0], table)
    table, N, E, Y = resident_table([], ns, es, y_rows)
    assert table.shape == (4, 1) and not table.any() and (N, E, Y) == (0, 0, 0)


@pytest.mark.parametrize("ids", [[4], [0, -1], [1, 2, 99], [0.5], [True]])
def test_bad_ids_raise_index_error(ids):
    ns = np.array([3, 1, 5, 2])
    with pytest.raises(IndexError):
        resident_table(ids, ns, ns, ns)


def test_batches_beyond_int32_are_refused():
    ns = np.array([2 ** 30, 1])
    with pytest.raises(_lib.GlamHipError, match="int32"):
        resident_table([0, 0], ns, np.array([0, 0]), np.array([1, 1]))


def test_resident_loader_needs_a_device_and_one_record_layout():
    rng = np.random.default_rng(0)
    mols = [synth_molecule(rng) for _ in range(4)]
    with pytest.raises(ValueError, match="device"):
        DataLoader(mols, batch_size=2, resident=True)
    odd = mols + [Data(x=torch.zeros(2, 15), edge_index=torch.zeros(2, 0, dtype=torch.long))]      # no edge_attr, no y
    with pytest.raises(ValueError, match="one layout"):
        DataLoader(odd, batch_size=2, device="cuda", resident=True)
    assert DataLoader(odd, batch_size=2).resident is False          # the default is the host loader, heterogeneous records included
    assert len(list(DataLoader(odd, batch_size=2))) == 3


def _pointers(values):
    return (ctypes.c_void_p * FIELDS)(*values)


def test_abi_rejects_bad_arguments_before_any_device_work():
    """Every call below fails a check that runs BEFORE the launch (the pointers are made-up addresses that nothing dereferences)."""
    raw = _lib.load()
    good = [0x10000 * (i + 1) for i in range(FIELDS)]
    ds, out, table = _pointers(good), _pointers(good), ctypes.c_void_p(0x900000)
    sizes = (4, 9, 20, 4, 30, 60, 16, 4)                            # B, N, E, Y, Ed, row bytes of x / edge_attr / y

    def call(ds=ds, out=out, table=table, sizes=sizes):
        return raw.glam_collate(ds, out, table, *sizes, None)

    assert call(ds=None) == _lib.GLAM_E_INVALID and b"null pointer" in raw.glam_last_error()
    assert call(out=None) == _lib.GLAM_E_INVALID
    assert call(table=None) == _lib.GLAM_E_INVALID
    assert call(sizes=(-1,) + sizes[1:]) == _lib.GLAM_E_INVALID
    assert call(sizes=(4, 9, 20, 4, 30, 60, 18, 4)) == _lib.GLAM_E_INVALID and b"multiples of 4" in raw.glam_last_error()
    assert call(sizes=(4, 0, 20, 4, 30, 60, 16, 4)) == _lib.GLAM_E_INVALID                       # edges without nodes
    for field in (5, 6, 7, 10, 4, 1, 8, 12, 0, 2, 3):               # an output the batch needs is missing
        vals = list(good)
        vals[field] = None
        assert call(out=_pointers(vals)) == _lib.GLAM_E_INVALID and b"null pointer" in raw.glam_last_error(), field
    for field in (4, 7, 9, 11, 1, 2):                               # ... or a tensor of the dataset
        vals = list(good)
        vals[field] = None
        assert call(ds=_pointers(vals)) == _lib.GLAM_E_INVALID and b"null pointer" in raw.glam_last_error(), field
    vals = list(good)
    vals[8] += 2                                                    # int32 tensors on 4 bytes
    assert call(out=_pointers(vals)) == _lib.GLAM_E_INVALID and b"misaligned pointer (field 8)" in raw.glam_last_error()
    vals = list(good)
    vals[1] += 4                                                    # int64 tensors on 8
    assert call(out=_pointers(vals)) == _lib.GLAM_E_INVALID and b"misaligned pointer (field 1)" in raw.glam_last_error()
    for side in ("ds", "out"):                                      # ELL records on 16
        vals = list(good)
        vals[14] += 8
        assert call(**{side: _pointers(vals)}) == _lib.GLAM_E_INVALID and b"misaligned ELL" in raw.glam_last_error()
    vals = list(good)
    vals[16] = None                                                 # half a pair
    assert call(out=_pointers(vals)) == _lib.GLAM_E_INVALID and b"ELL pair" in raw.glam_last_error()
    vals = list(good)
    vals[13] = vals[14] = None                                      # an ELL output the dataset has no records for
    assert call(ds=_pointers(vals)) == _lib.GLAM_E_INVALID and b"without the dataset" in raw.glam_last_error()
    assert call(sizes=(4, 2 ** 30, 20, 4, 30, 60, 16, 4)) == _lib.GLAM_E_UNSUPPORTED and b"2^31" in raw.glam_last_error()
    with pytest.raises(_lib.GlamHipError, match=r"^glam_collate failed \(code -1\): "):
        _lib.api().glam_collate(None, None, None, *sizes, None)


def test_an_index_made_from_parts_is_resolved_and_found_by_the_caches():
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    t = (i32(0, 1, 2, 3), i32(1, 2, 0), i32(0, 1, 2))
    pair = (torch.full((3, 4), -1, dtype=torch.int32), torch.full((3, 4), -1, dtype=torch.int32))
    gi = ops.GraphIndex.from_parts(ei, 3, i32(0, 1, 2, 3), i32(2, 0, 1), i32(2, 0, 1), t, pair, None)
    assert (gi.N, gi.E) == (3, 3) and gi.transpose() is gi._t and gi._t == t
    assert gi.ell() is gi._ell and gi._ell[0] is pair[0] and gi.ell_t() is None          # resolved: neither is False, nothing to build
    ops._GI_CACHE.put(ei, (3, gi))
    assert ops.graph_index(ei, 3) is gi                                                  # (a miss would raise: ei is a CPU tensor)
    batch = torch.tensor([0, 0, 1])
    sp = ops.SegmentPtr.from_parts(i32(0, 2, 3), 3, 2)
    assert (sp.N, sp.B) == (3, 2)
    ops._SP_CACHE.put(batch, sp)
    assert ops.segment_ptr(batch) is sp and ops.segment_ptr(batch, 2) is sp
