"""CPU: the host side of DDI pair scoring (``ArchitectureDDI.encode_drugs`` / ``score_pairs``) — the C prototype of the gathered fusion
against its ctypes row, the entry point's argument checks by status code, the index rules (``ops.pair_index`` under other names) and the
refusals of ``score_pairs``, all of which run before anything is launched and need no device."""
import ctypes

import numpy as np
import pytest
import torch

from glam_amd import _lib, model, ops
from glam_amd._lib import GlamHipError
from tests.test_host_logic import _header_prototypes, _table_type

NAME = "glam_pair_pool_gather_fwd"
_KW = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")


def test_gathered_fusion_prototype_matches_its_signature_row():
    """Header and ``SIGNATURES`` type for type; a STATUS return that ``api()`` checks; the ABI version stays 4 (additive)."""
    protos = _header_prototypes()
    res, args = _lib.SIGNATURES[NAME]
    assert (_table_type(res), [_table_type(a) for a in args]) == protos[NAME]
    p, i64, i32 = "pointer", ctypes.c_int64, ctypes.c_int
    assert protos[NAME] == (i32, [p, p, p, p, p, p, i64, i64, i64, i32, p, p, p])
    assert protos["glam_pair_pool_gather_load_bytes"] == (ctypes.c_size_t, [p, p, i32])
    assert NAME not in _lib.VALUE_RETURNS and _lib.ABI_VERSION == 4
    assert getattr(_lib.api(), NAME).errcheck is not None and getattr(_lib.load(), NAME).errcheck is None


def test_gathered_fusion_rejects_bad_arguments_without_a_gpu():
    f = _lib.load().glam_pair_pool_gather_fwd
    none = [None] * 6
    tail = (None, None, None)
    assert f(*none, 0, 0, 0, 60, *tail) == 0                                  # no pairs: nothing to do, nothing dereferenced
    assert f(*none, 0, 3, 3, 128, *tail) == 0
    assert f(*none, 4, 2, 2, 129, *tail) == _lib.GLAM_E_UNSUPPORTED           # D out of range, before anything else
    assert f(*none, 4, 2, 2, 132, *tail) == _lib.GLAM_E_UNSUPPORTED
    assert f(*none, 4, 2, 2, 0, *tail) == _lib.GLAM_E_UNSUPPORTED
    assert f(*none, -1, 2, 2, 60, *tail) == _lib.GLAM_E_INVALID               # P < 0
    assert f(*none, 4, -1, 2, 60, *tail) == _lib.GLAM_E_INVALID
    assert f(*none, 4, 0, 2, 60, *tail) == _lib.GLAM_E_INVALID                # pairs, but no segment on one side
    assert f(*none, 4, 4, 4, 60, *tail) == _lib.GLAM_E_INVALID                # null pointers
    fake = ctypes.c_void_p(4096)                                              # (never dereferenced: each call fails a check first)
    assert f(fake, fake, fake, fake, None, fake, 4, 2, 2, 60, fake, None, None) == _lib.GLAM_E_INVALID       # idx1 = NULL needs Q1 == P
    assert f(fake, fake, fake, fake, fake, None, 4, 2, 2, 60, fake, None, None) == _lib.GLAM_E_INVALID
    assert f(fake, fake, fake, fake, fake, fake, 4, 2, 2, 60, None, None, None) == _lib.GLAM_E_INVALID       # out = NULL
    assert f(ctypes.c_void_p(4098), fake, fake, fake, fake, fake, 4, 2, 2, 60, fake, None, None) == _lib.GLAM_E_INVALID   # not even a dword boundary
    with pytest.raises(GlamHipError, match=NAME):
        _lib.api().glam_pair_pool_gather_fwd(*none, 4, 4, 4, 60, *tail)


def test_gathered_fusion_picks_its_loads_by_width_and_alignment():
    """16-byte loads need D % 4 == 0 AND both matrices on a 16-byte boundary; misaligned rows with D % 4 == 0 are served by the dword
    kernel, not refused; a width outside 1..128 has no kernel."""
    q = _lib.load().glam_pair_pool_gather_load_bytes
    a, off4, off8 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4104)
    assert [q(a, a, D) for D in (4, 60, 64, 92, 128)] == [16] * 5
    assert [q(a, a, D) for D in (1, 15, 45, 90, 127)] == [4] * 5
    assert q(off4, a, 60) == 4 and q(a, off8, 60) == 4 and q(off4, off4, 64) == 4
    assert [q(a, a, D) for D in (0, -4, 129, 132, 256)] == [0] * 5


def test_pair_index_names_the_index_it_refuses():
    """``name`` / ``over`` only change what the messages say; the defaults leave the screening messages as they were."""
    ix = ops.pair_index(np.asarray([2, 0, 2]), 3, 4, name="first", over="drugs")
    assert ix.host.tolist() == [2, 0, 2] and (ix.P, ix.Q) == (3, 4) and ops.pair_index(ix, 3, 4, name="first", over="drugs") is ix
    with pytest.raises(IndexError, match=r"first must lie in \[0, 4\)"):
        ops.pair_index([2, 0, 4], 3, 4, name="first", over="drugs")
    with pytest.raises(IndexError, match="second must have one entry per pair"):
        ops.pair_index([2, 0], 3, 4, name="second", over="drugs")
    with pytest.raises(IndexError, match="first must hold integers"):
        ops.pair_index([2.0, 0.0, 1.0], 3, 4, name="first", over="drugs")
    with pytest.raises(IndexError, match="first was validated for 3 pairs over 4 drugs, not 3 over 5"):
        ops.pair_index(ix, 3, 5, name="first", over="drugs")
    with pytest.raises(IndexError, match="idx1=None takes segment i for pair i: 3 pairs but 2 segments of x1"):
        ops.pair_index(None, 3, 2, name="idx1", over="segments of x1")
    with pytest.raises(GlamHipError, match="second lives on a device.*read-back"):
        ops.pair_index(torch.zeros(3, dtype=torch.int64, device="meta"), 3, 4, name="second", over="drugs")
    # today's messages
    with pytest.raises(IndexError, match=r"pro_of_pair must lie in \[0, 4\)"):
        ops.pair_index([2, 0, 4], 3, 4)
    with pytest.raises(IndexError, match="pro_of_pair=None pairs ligand i with protein i: 3 ligands but 2 proteins"):
        ops.pair_index(None, 3, 2)
    with pytest.raises(IndexError, match="pro_of_pair was validated for 3 pairs over 4 proteins, not 3 over 5"):
        ops.pair_index(ix, 3, 5)
    with pytest.raises(GlamHipError, match="pro_of_pair lives on a device"):
        ops.pair_index(torch.zeros(3, dtype=torch.int64, device="meta"), 3, 4)


def test_pair_scoring_contract_is_refused_before_any_device_work():
    """Training mode, grad mode, a norm that looks across the batch (in EITHER tower) and a foreign encoding are refused by host-side
    checks (CPU model, no device behind it)."""
    net = model.ArchitectureDDI(**_KW)
    with torch.no_grad():
        with pytest.raises(GlamHipError, match="training mode"):
            net.encode_drugs(None)
        with pytest.raises(GlamHipError, match="training mode"):
            net.score_pairs(None, [0], [0])
        for slot, norm, where in (("flat_norm", "_LayerNorm", "mol1_flat"), ("flat_norm", "_PairNorm", "mol1_flat"),
                                  ("flat_norm", "_GraphSizeNorm", "mol1_flat"), ("graph_norm", "_GraphSizeNorm", "mol1_conv"),
                                  ("pre_norm", "_GraphSizeNorm", "mol1_lin0")):
            with pytest.raises(GlamHipError, match=f"{where}'s norm {norm}.*depends on how often each drug"):
                model.ArchitectureDDI(**_KW, **{slot: norm}).eval().encode_drugs(None)
        odd = model.ArchitectureDDI(**_KW).eval()
        odd.mol2_flat.norm = model.ArchitectureDDI(**_KW, flat_norm="_LayerNorm").mol2_flat.norm       # the SECOND tower alone
        with pytest.raises(GlamHipError, match="mol2_flat's norm _LayerNorm"):
            odd.encode_drugs(None)
        for slot in ("pre_norm", "graph_norm"):                  # per graph / per row: admitted (the guard passes, the call then needs data)
            for norm in ("_BatchNorm", "_LayerNorm", "_PairNorm"):
                model.ArchitectureDDI(**_KW, **{slot: norm}).eval()._pairs_guard("encode_drugs")
        model.ArchitectureDDI(**_KW, flat_norm="_BatchNorm", end_norm="_LayerNorm").eval()._pairs_guard("score_pairs")   # the head is free
    with pytest.raises(GlamHipError, match="no_grad"):
        net.eval().score_pairs(None, [0], [0])
    with pytest.raises(GlamHipError, match="no_grad"):
        net.eval().encode_drugs(None)
    with torch.no_grad(), pytest.raises(GlamHipError, match="another model"):
        net.eval().score_pairs(object(), [0], [0])


def test_drug_stamp_follows_both_towers_and_not_the_head():
    net = model.ArchitectureDDI(**_KW).eval()
    s0 = net._drug_stamp()
    with torch.no_grad():
        next(net.lin_out0.parameters()).add_(1)                  # the head is not part of the stamp
        next(net.lin_out1.parameters()).add_(1)
        assert net._drug_stamp() == s0
        for tower in ("mol1_lin0", "mol2_conv", "mol1_flat", "mol2_flat"):
            before = net._drug_stamp()
            next(getattr(net, tower).parameters()).add_(1)
            assert net._drug_stamp() != before, tower
    before = net._drug_stamp()
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    assert net._drug_stamp() != before
    before = net._drug_stamp()
    ops.PARAM_EPOCH += 1                                         # what the raw-pointer optimizers announce
    try:
        assert net._drug_stamp() != before
    finally:
        ops.PARAM_EPOCH -= 1


def test_a_stale_or_foreign_encoding_is_refused_on_the_host():
    """``score_pairs`` looks at the encoding's model and stamp before its rows: a ``DrugEncoding`` without tensors is enough here."""
    net, other = model.ArchitectureDDI(**_KW).eval(), model.ArchitectureDDI(**_KW).eval()

    class _Sp:
        B = 3
    enc = model.DrugEncoding(net, [None, None], [None, None], _Sp(), None, None, net._drug_stamp())
    assert enc.num_graphs == 3 and enc.model() is net
    with torch.no_grad():
        with pytest.raises(GlamHipError, match="another model"):
            other.score_pairs(enc, [0], [0])
        for bad in ([0, 3], [-1, 0]):
            with pytest.raises(IndexError, match=r"first must lie in \[0, 3\)"):
                net.score_pairs(enc, bad, [0, 0])
            with pytest.raises(IndexError, match=r"second must lie in \[0, 3\)"):
                net.score_pairs(enc, [0, 0], bad)
        with pytest.raises(IndexError, match="second must have one entry per pair"):
            net.score_pairs(enc, [0, 1], [0])
        with pytest.raises(GlamHipError, match="second lives on a device"):
            net.score_pairs(enc, [0, 1], torch.zeros(2, dtype=torch.int64, device="meta"))
        next(net.mol2_conv.parameters()).add_(1)
        with pytest.raises(GlamHipError, match="stale"):
            net.score_pairs(enc, [0], [0])
