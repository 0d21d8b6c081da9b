"""CPU: the host side of screening (``ArchitectureDTI.encode_proteins`` / ``screen``) — the C prototype of the indexed fusion against its
ctypes row, and the pair -> protein index rules (``ops.pair_index``), which run before anything is launched and need no device."""
import ctypes

import numpy as np
import pytest
import torch

from glam_amd import _lib, model, ops
from glam_amd._lib import GlamHipError
from tests.test_host_logic import _header_prototypes, _table_type

NAME = "glam_pair_pool_indexed_fwd"


def test_indexed_fusion_prototype_matches_its_signature_row():
    """Header and ``SIGNATURES`` type for type; the entry point returns a STATUS (checked by ``api()``), and the ABI version stays 4:
    the addition is additive."""
    proto = _header_prototypes()[NAME]
    res, args = _lib.SIGNATURES[NAME]
    assert (_table_type(res), [_table_type(a) for a in args]) == proto
    p, i64, i32, sz = "pointer", ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    assert proto == (i32, [p, p, p, p, p, i64, i64, i32, p, p, p, sz, p])
    assert NAME not in _lib.VALUE_RETURNS and _lib.ABI_VERSION == 4
    assert _lib.api().glam_pair_pool_indexed_fwd.errcheck is not None and _lib.load().glam_pair_pool_indexed_fwd.errcheck is None


def test_indexed_fusion_rejects_bad_arguments_without_a_gpu():
    raw = _lib.load()
    none = [None] * 5
    assert raw.glam_pair_pool_indexed_fwd(*none, 0, 0, 60, None, None, None, 0, None) == 0                       # no pairs: nothing to do
    assert raw.glam_pair_pool_indexed_fwd(*none, 4, 2, 257, None, None, None, 0, None) == _lib.GLAM_E_UNSUPPORTED  # D > 256
    assert raw.glam_pair_pool_indexed_fwd(*none, 4, 2, 0, None, None, None, 0, None) == _lib.GLAM_E_UNSUPPORTED
    assert raw.glam_pair_pool_indexed_fwd(*none, 4, 0, 60, None, None, None, 0, None) == _lib.GLAM_E_INVALID       # pairs, no protein
    assert raw.glam_pair_pool_indexed_fwd(*none, 4, 2, 60, None, None, None, 0, None) == _lib.GLAM_E_INVALID       # null pointers
    assert raw.glam_pair_pool_indexed_fwd(*none, -1, 2, 60, None, None, None, 0, None) == _lib.GLAM_E_INVALID
    with pytest.raises(GlamHipError, match="glam_pair_pool_indexed_fwd"):
        _lib.api().glam_pair_pool_indexed_fwd(*none, 4, 2, 60, None, None, None, 0, None)


@pytest.mark.parametrize("make", [list, np.asarray, torch.tensor, lambda v: np.asarray(v, dtype=np.uint8), lambda v: torch.tensor(v, dtype=torch.int32)])
def test_pair_index_accepts_host_integers(make):
    ix = ops.pair_index(make([2, 0, 2, 1, 2]), 5, 4)
    assert ix.host.dtype == np.int32 and ix.host.tolist() == [2, 0, 2, 1, 2] and (ix.P, ix.Q) == (5, 4)
    assert ops.pair_index(ix, 5, 4) is ix                       # validated once, reused by every step of a screen() call


def test_pair_index_refuses_what_the_kernel_would_trust():
    with pytest.raises(IndexError, match=r"\[0, 4\)"):
        ops.pair_index([2, 0, 4, 1, 2], 5, 4)                   # an index equal to Q
    with pytest.raises(IndexError, match=r"\[0, 4\)"):
        ops.pair_index([2, 0, -1, 1, 2], 5, 4)
    with pytest.raises(IndexError, match="one entry per pair"):
        ops.pair_index([2, 0, 1, 2], 5, 4)                      # a wrong length
    with pytest.raises(IndexError, match="one entry per pair"):
        ops.pair_index([[2, 0, 1, 2, 0]], 5, 4)
    with pytest.raises(IndexError, match="integers"):
        ops.pair_index([2.0, 0.0, 1.0, 2.0, 0.0], 5, 4)
    with pytest.raises(IndexError):
        ops.pair_index([], 5, 4)
    with pytest.raises(IndexError, match="validated for"):
        ops.pair_index(ops.pair_index([0, 1], 2, 2), 2, 3)
    with pytest.raises(GlamHipError, match="read-back"):       # a device tensor: no hidden synchronisation to validate it
        ops.pair_index(torch.zeros(5, dtype=torch.int64, device="meta"), 5, 4)
    assert ops.pair_index([], 0, 0).host.shape == (0,)


def test_pair_index_defaults():
    """``None``: the op pairs ligand i with protein i (needs Q == P); ``screen`` pairs every ligand with the ONE encoded protein."""
    assert ops.pair_index(None, 3, 3).host.tolist() == [0, 1, 2]
    with pytest.raises(IndexError, match="3 ligands but 2 proteins"):
        ops.pair_index(None, 3, 2)
    assert ops.pair_index(None, 3, 1, default="single").host.tolist() == [0, 0, 0]
    with pytest.raises(IndexError, match="pass the index"):
        ops.pair_index(None, 3, 3, default="single")


def test_screening_contract_is_refused_before_any_device_work():
    """Training mode, grad mode and a norm that looks across the batch are refused by host-side checks (CPU model, no device behind it)."""
    kw = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")
    net = model.ArchitectureDTI(**kw)
    with torch.no_grad():
        with pytest.raises(GlamHipError, match="training mode"):
            net.encode_proteins(None)
        for slot, norm in (("flat_norm", "_LayerNorm"), ("flat_norm", "_PairNorm"), ("flat_norm", "_GraphSizeNorm"),
                           ("graph_norm", "_GraphSizeNorm"), ("pre_norm", "_GraphSizeNorm")):
            with pytest.raises(GlamHipError, match="depends on how often each protein"):
                model.ArchitectureDTI(**kw, **{slot: norm}).eval().encode_proteins(None)
    with pytest.raises(GlamHipError, match="no_grad"):
        net.eval().screen(None, None)
    with torch.no_grad(), pytest.raises(GlamHipError, match="another model"):
        net.eval().screen(None, object())
    s0 = net._protein_stamp()
    with torch.no_grad():
        next(net.mol_conv.parameters()).add_(1)                 # the ligand side is not part of the stamp
        assert net._protein_stamp() == s0
        next(net.pro_conv.parameters()).add_(1)
        assert net._protein_stamp() != s0
