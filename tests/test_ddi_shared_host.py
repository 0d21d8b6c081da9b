"""CPU: the host side of DDI training on drugs held once (csrc/pairgather_bwd.hip, ``ops.pair_pool_gather_shared``,
``ArchitectureDDI.forward_shared``) — the C prototypes against their ctypes rows, the entry points' argument checks by status code, the
by-drug pair lists of both sides, and the refusals that come before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

from glam_amd import _lib, layer, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import synth_batch
from tests.test_host_logic import _header_prototypes, _table_type

FWD, BWD = "glam_pair_pool_gather_train_fwd", "glam_pair_pool_gather_bwd"
_KW = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")


def test_prototypes_match_the_signature_table():
    """Header and ``SIGNATURES`` type for type; STATUS returns that ``api()`` checks; the ABI version stays 4 (additive), and the inference
    entry point keeps its signature."""
    protos = _header_prototypes()
    p, i64, i32 = "pointer", ctypes.c_int64, ctypes.c_int
    for name in (FWD, BWD):
        res, args = _lib.SIGNATURES[name]
        assert (_table_type(res), [_table_type(a) for a in args]) == protos[name], name
        assert name not in _lib.VALUE_RETURNS
        assert getattr(_lib.api(), name).errcheck is not None and getattr(_lib.load(), name).errcheck is None
    assert protos[FWD] == (i32, [p] * 6 + [i64, i64, i64, i32, p, p, p, p])
    assert protos[BWD] == (i32, [p] * 13 + [i64, i64, i64, i32, p, p, p, p, p])
    assert protos["glam_pair_pool_gather_fwd"] == (i32, [p] * 6 + [i64, i64, i64, i32, p, p, p])
    assert _lib.load().glam_abi_version() == _lib.ABI_VERSION == 4


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    one = ctypes.c_void_p(4096)          # a non-null, aligned address nothing dereferences: the checks come first
    fwd = lambda P, Q1, Q2, D, p=one, i1=one, i2=one: lib.glam_pair_pool_gather_train_fwd(p, p, p, p, i1, i2, P, Q1, Q2, D, p, p, p, None)   # noqa: E731
    bwd = lambda P, Q1, Q2, D, p=one, i1=one, i2=one: lib.glam_pair_pool_gather_bwd(p, p, p, p, i1, i2, *([p] * 7), P, Q1, Q2, D, None, None,  # noqa: E731
                                                                                    p, p, None)
    for f, name in ((fwd, FWD), (bwd, BWD)):
        assert f(0, 0, 0, 60) == 0 and f(0, 3, 2, 128, None, None, None) == 0          # P == 0: before any pointer check
        for D in (0, 129, 132, -4):
            assert f(4, 2, 2, D) == _lib.GLAM_E_UNSUPPORTED, D
        assert f(4, 2, 2, 129) == _lib.GLAM_E_UNSUPPORTED and b"129" in lib.glam_last_error() and name.encode() in lib.glam_last_error()
        assert f(4, 2, 2, 60, None) == _lib.GLAM_E_INVALID and b"null" in lib.glam_last_error()
        assert f(4, 0, 2, 60) == _lib.GLAM_E_INVALID and b"no segment" in lib.glam_last_error()
        assert f(4, 2, 0, 60) == _lib.GLAM_E_INVALID
        assert f(-1, 2, 2, 60) == _lib.GLAM_E_INVALID and f(4, -1, 2, 60) == _lib.GLAM_E_INVALID and f(4, 2, -1, 60) == _lib.GLAM_E_INVALID
        assert f(4, 2, 4, 60, one, None, one) == _lib.GLAM_E_INVALID and b"idx1 = NULL" in lib.glam_last_error()     # identity needs Q1 == P
        assert f(4, 4, 2, 60, one, one, None) == _lib.GLAM_E_INVALID and b"idx2 = NULL" in lib.glam_last_error()
        assert f(4, 2, 2, 60, ctypes.c_void_p(4098)) == _lib.GLAM_E_INVALID and b"aligned" in lib.glam_last_error()
    # the training forward needs what the inference call may leave out
    assert lib.glam_pair_pool_gather_train_fwd(one, one, one, one, one, one, 4, 2, 2, 60, one, None, one, None) == _lib.GLAM_E_INVALID
    assert lib.glam_pair_pool_gather_train_fwd(one, one, one, one, one, one, 4, 2, 2, 60, one, one, None, None) == _lib.GLAM_E_INVALID
    # ... and the backward each of its lists and outputs
    for hole in list(range(4)) + list(range(6, 13)) + [19, 20]:
        args = [one] * 13 + [4, 2, 2, 60, None, None, one, one, None]
        args[hole] = None
        assert lib.glam_pair_pool_gather_bwd(*args) == _lib.GLAM_E_INVALID, hole
    with pytest.raises(GlamHipError, match=f"{FWD} failed"):
        _lib.api().glam_pair_pool_gather_train_fwd(*[None] * 6, 4, 4, 4, 60, *[None] * 4)
    with pytest.raises(GlamHipError, match=f"{BWD} failed"):
        _lib.api().glam_pair_pool_gather_bwd(*[None] * 13, 4, 4, 4, 60, *[None] * 5)


def test_by_drug_lists_of_both_sides():
    """What the backward walks: each side's pairs stably sorted by drug (``PairIndex.by_protein`` — the class is generic), an unreferenced
    drug with an empty run."""
    first, second = [2, 0, 2, 1, 2, 0], [1, 1, 3, 0, 1, 3]
    i1 = ops.pair_index(first, 6, 4, name="first", over="drugs")          # drug 3 never first
    i2 = ops.pair_index(second, 6, 5, name="second", over="drugs")        # drugs 2 and 4 never second
    l1, l2 = i1.by_protein(), i2.by_protein()
    assert isinstance(l1, ops.PairsByProtein) and l1 is i1.by_protein()
    assert l1.order.tolist() == [1, 5, 3, 0, 2, 4] and l1.ptr.tolist() == [0, 2, 3, 6, 6]
    assert l2.order.tolist() == [3, 0, 1, 4, 2, 5] and l2.ptr.tolist() == [0, 1, 4, 4, 6, 6]
    for ix, host, Q in ((l1, first, 4), (l2, second, 5)):
        assert ix.order.dtype == np.int32 and ix.ptr.dtype == np.int32
        for q in range(Q):
            assert np.array_equal(ix.order[ix.ptr[q]:ix.ptr[q + 1]], np.flatnonzero(np.asarray(host) == q))
    ident = ops.pair_index(None, 3, 3, name="idx1", over="segments of x1").by_protein()
    assert ident.order.tolist() == [0, 1, 2] and ident.ptr.tolist() == [0, 1, 2, 3]


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDDI(**_KW, **kw).eval()


def test_forward_shared_refuses_on_the_host():
    d1, d2 = synth_batch(3, seed=3), synth_batch(2, seed=5)
    first, second = [0, 1, 2, 2, 0, 1], [0, 1, 1, 0, 1, 1]
    for slot, norm, where in (("graph_norm", "_GraphSizeNorm", "mol1_conv"), ("pre_norm", "_GraphSizeNorm", "mol1_lin0"),
                              ("flat_norm", "_LayerNorm", "mol1_flat"), ("flat_norm", "_PairNorm", "mol1_flat")):
        with pytest.raises(GlamHipError, match=f"forward_shared: {where}'s norm {norm}.*depends on how often each drug"):
            _net(**{slot: norm}).forward_shared(d1, d2, first, second)
    odd = _net()
    odd.mol2_conv.norm = _net(graph_norm="_GraphSizeNorm").mol2_conv.norm            # the SECOND tower alone
    with pytest.raises(GlamHipError, match="mol2_conv's norm _GraphSizeNorm"):
        odd.forward_shared(d1, d2, first, second)
    for slot, where in (("pre_norm", "mol1_lin0"), ("graph_norm", "mol1_conv"), ("flat_norm", "mol1_flat")):
        with pytest.raises(GlamHipError, match=f"{where}'s norm _BatchNorm .* how often it is repeated"):
            _net(**{slot: "_BatchNorm"}).train().forward_shared(d1, d2, first, second)
    odd = _net().train()
    odd.mol2_flat.norm = _net(flat_norm="_BatchNorm").mol2_flat.norm
    with pytest.raises(GlamHipError, match="mol2_flat's norm _BatchNorm"):
        odd.forward_shared(d1, d2, first, second)
    net = _net()
    with pytest.raises(IndexError, match="second must have one entry per pair"):
        net.forward_shared(d1, d2, first, [0, 1, 1])
    with pytest.raises(IndexError, match="second must have one entry per pair"):
        net.forward_shared(d1, d2, ops.pair_index(first, 6, 3, name="first", over="drugs"), second[:4])      # (P is that of the PairIndex)
    with pytest.raises(IndexError, match="first must have one entry per pair"):
        net.forward_shared(d1, d2, np.zeros((2, 3), dtype=np.int64), [0, 1])
    with pytest.raises(IndexError, match="second was validated for 6 pairs over 2 drugs, not 3 over 2"):
        net.forward_shared(d1, d2, [0, 1, 2], ops.pair_index(second, 6, 2, name="second", over="drugs"))
    with pytest.raises(IndexError, match=r"first must lie in \[0, 3\)"):
        net.forward_shared(d1, d2, [0, 1, 3, 2, 0, 1], second)
    with pytest.raises(IndexError, match=r"second must lie in \[0, 2\)"):
        net.forward_shared(d1, d2, first, [0, 1, 2, 0, 1, 1])
    with pytest.raises(IndexError, match="first must hold integers"):
        net.forward_shared(d1, d2, [0.5] * 6, second)
    with pytest.raises(IndexError, match="second=None takes segment i for pair i: 6 pairs but 2 drugs"):
        net.forward_shared(d1, d2, first, None)
    with pytest.raises(IndexError, match="first=None takes segment i for pair i: 6 pairs but 3 drugs"):
        net.forward_shared(d1, d2, None, second)
    with pytest.raises(IndexError, match="second=None takes segment i for pair i: 3 pairs but 2 drugs"):
        net.forward_shared(d1, d2)
    with pytest.raises(GlamHipError, match="second lives on a device.*read-back"):
        net.forward_shared(d1, d2, first, torch.zeros(6, dtype=torch.int64, device="meta"))
    # what passes the guards goes on to the device — and a CPU batch fails there, loudly (no CPU fallback); the head's norms are free
    for ok in (_net(pre_norm="_BatchNorm"), _net(graph_norm="_PairNorm").train(), _net(end_norm="_LayerNorm").train(), _net()):
        with pytest.raises(GlamHipError, match="HIP device only"):
            ok.forward_shared(d1, d2, first, second)
    with pytest.raises(GlamHipError, match="HIP device only"):
        net.forward_shared(d1, d1)                                                     # the same Batch on both sides, identity indices


def test_the_default_indices_are_kept_per_shape():
    net = _net()
    a = net._shared_index(None, 4, 4, "cpu", "first")
    assert a is net._shared_index(None, 4, 4, "cpu", "second") and a is not net._shared_index(None, 5, 5, "cpu", "first")
    assert a.host.tolist() == [0, 1, 2, 3]


def test_op_refuses_on_the_host_and_pair_pool_gather_still_refuses_grad():
    class _SP:
        def __init__(self, B, N):
            self.B, self.N = B, N
    x1, x2 = torch.randn(4, 8, requires_grad=True), torch.randn(6, 8)
    with pytest.raises(GlamHipError, match="inference only"):
        ops.pair_pool_gather(x1, x2, _SP(2, 4), _SP(3, 6), [0, 1], [2, 2])
    with pytest.raises(IndexError, match=r"idx2 must lie in \[0, 3\)"):
        ops.pair_pool_gather_shared(x1, x2, _SP(2, 4), _SP(3, 6), [0, 1], [2, 3])
    with pytest.raises(IndexError, match="idx1=None takes segment i for pair i: 3 pairs but 2 segments of x1"):
        ops.pair_pool_gather_shared(x1, x2, _SP(2, 4), _SP(3, 6), None, [2, 1, 0])
    with pytest.raises(GlamHipError, match="idx1 lives on a device"):
        ops.pair_pool_gather_shared(x1, x2, _SP(2, 4), _SP(3, 6), torch.zeros(2, dtype=torch.int64, device="meta"), [2, 1])
    with pytest.raises(GlamHipError, match="HIP device only"):
        ops.pair_pool_gather_shared(x1, x2, _SP(2, 4), _SP(3, 6), [0, 1], [2, 2])
    assert "pair_pool_gather_shared" in ops.__dict__ and hasattr(layer, "dot_and_global_pool2_gather_shared")
