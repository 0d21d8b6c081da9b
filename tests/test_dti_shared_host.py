"""CPU: the host side of training against proteins held once (csrc/pairshared.hip, ``ops.pair_pool_shared``, ``forward_shared``) — the
C ABI's prototypes and argument checks, the pair list by protein, and the refusals that come before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from glam_amd import _lib, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_batch, synth_protein
from tests.conftest import ROOT

_NEW = ("glam_pair_pool_shared_fwd", "glam_pair_pool_shared_bwd", "glam_pair_rows_bwd")
_C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}


def test_prototypes_match_the_signature_table():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glam_hip.h")).read(), flags=re.S)
    for name in _NEW:
        ret, params = re.search(r"([\w \t*]+?)\b" + name + r"\s*\(([^()]*)\)\s*;", src).groups()
        types = ["pointer" if "*" in q else _C_SCALARS[" ".join(w for w in q.split()[:-1] if w != "const")] for q in params.split(",")]
        res, args = _lib.SIGNATURES[name]
        assert ret.strip() == "int" and res is ctypes.c_int
        assert [("pointer" if a is ctypes.c_void_p else a) for a in args] == types, name
        assert getattr(_lib.api(), name).errcheck is not None, f"{name} returns a status: the checked view must check it"
    assert _lib.load().glam_abi_version() == _lib.ABI_VERSION == 4       # additive: the version stays


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    one = ctypes.c_void_p(16)            # a non-null, aligned address nothing dereferences: the checks come first
    fwd = lambda P, Q, D, p=one: lib.glam_pair_pool_shared_fwd(p, p, p, p, p, P, Q, D, p, p, p, p, 1 << 30, None)      # noqa: E731
    bwd = lambda P, Q, D, p=one: lib.glam_pair_pool_shared_bwd(*([p] * 10), P, Q, D, None, None, p, p, None)          # noqa: E731
    rows = lambda P, Q, W, p=one: lib.glam_pair_rows_bwd(p, p, p, P, Q, W, p, None)                                  # noqa: E731
    for f in (fwd, bwd):
        assert f(0, 0, 60) == 0 and f(0, 3, 60, None) == 0           # P == 0: nothing to do
        assert f(4, 2, 257) == _lib.GLAM_E_UNSUPPORTED and b"257" in lib.glam_last_error()
        assert f(4, 2, 0) == _lib.GLAM_E_UNSUPPORTED
        assert f(4, 2, 60, None) == _lib.GLAM_E_INVALID and b"null" in lib.glam_last_error()
        assert f(4, 0, 60) == _lib.GLAM_E_INVALID and b"no protein" in lib.glam_last_error()
        assert f(-1, 2, 60) == _lib.GLAM_E_INVALID and f(4, -1, 60) == _lib.GLAM_E_INVALID
    assert rows(0, 0, 60) == 0 and rows(0, 3, 60, None) == 0
    assert rows(4, 2, 60, None) == _lib.GLAM_E_INVALID and b"null" in lib.glam_last_error()
    assert rows(4, 0, 60) == _lib.GLAM_E_INVALID
    assert rows(-1, 2, 60) == _lib.GLAM_E_INVALID and rows(4, -1, 60) == _lib.GLAM_E_INVALID and rows(4, 2, 0) == _lib.GLAM_E_INVALID
    with pytest.raises(GlamHipError, match="glam_pair_pool_shared_bwd failed"):
        _lib.api().glam_pair_pool_shared_bwd(*([None] * 10), 4, 2, 60, None, None, None, None, None)


@pytest.mark.parametrize("idx,Q", [([2, 0, 2, 1, 2], 4), ([0, 0, 0], 1), ([], 3), ([], 0), ([3, 3, 1, 3, 1, 0, 3], 5)])
def test_by_protein_is_the_stable_argsort(idx, Q):
    index = ops.pair_index(idx, len(idx), Q)
    bp = index.by_protein()
    assert bp is index.by_protein(), "built once"
    host = np.asarray(idx, dtype=np.int64)
    assert bp.order.dtype == np.int32 and bp.ptr.dtype == np.int32 and bp.order.shape == (len(idx),) and bp.ptr.shape == (Q + 1,)
    assert np.array_equal(bp.order, np.argsort(host, kind="stable"))
    assert bp.ptr[0] == 0 and bp.ptr[-1] == len(idx)
    for q in range(Q):
        run = bp.order[bp.ptr[q]:bp.ptr[q + 1]]
        assert np.array_equal(run, np.flatnonzero(host == q)), "a protein's pairs in batch order (empty for an unreferenced one)"


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDTI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", pre_act="ReLU", graph_act="ReLU",
                                 flat_act="ReLU", end_act="ReLU", **kw).eval()


def test_forward_shared_refuses_on_the_host():
    rng = np.random.default_rng(4)
    mb, pros = synth_batch(6, seed=3), Batch.from_data_list([synth_protein(rng, 40, 60) for _ in range(2)])
    idx = [0, 1, 1, 0, 1, 1]
    with pytest.raises(GlamHipError, match="pro_conv's norm _GraphSizeNorm"):
        _net(graph_norm="_GraphSizeNorm").forward_shared(mb, pros, idx)
    with pytest.raises(GlamHipError, match="pro_flat's norm _LayerNorm"):
        _net(flat_norm="_LayerNorm").forward_shared(mb, pros, idx)
    with pytest.raises(GlamHipError, match="pro_lin0's norm _BatchNorm .* how often it is repeated"):
        _net(pre_norm="_BatchNorm").train().forward_shared(mb, pros, idx)
    for bad in ([0, 1, 1], [0, 1, 2, 0, 1, 1], [0.5] * 6, None):
        with pytest.raises(IndexError):
            _net().forward_shared(mb, pros, bad)
    # what passes the guards goes on to the device — and a CPU batch fails there, loudly (no CPU fallback)
    for net in (_net(pre_norm="_BatchNorm"), _net(graph_norm="_PairNorm").train(), _net()):
        with pytest.raises(GlamHipError, match="HIP device only"):
            net.forward_shared(mb, pros, idx)


def test_pair_pool_indexed_still_refuses_grad_mode():
    """The screening call stays inference only; the training route is a call of its own."""
    class _SP:
        B, N = 2, 4
    mol, pro = torch.randn(4, 8, requires_grad=True), torch.randn(4, 8)
    with pytest.raises(GlamHipError, match="inference only"):
        ops.pair_pool_indexed(mol, pro, _SP(), _SP(), [0, 1])
    assert "pair_pool_shared" in ops.__dict__ and "pair_rows" in ops.__dict__
