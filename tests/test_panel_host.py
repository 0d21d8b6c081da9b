"""CPU: the host side of panel screening (``ArchitectureDTI.screen_panel`` / ``ops.pair_pool_panel``) — the C prototypes of the panel
fusion against their ctypes rows, the entry point's argument checks by status code, the work table of ``ops.panel_plan`` and its
refusals, the refusals of ``screen_panel`` and its choice between the one-pass and the per-column head: everything that runs before
anything is launched and needs no device."""
import ctypes

import numpy as np
import pytest
import torch

from glam_amd import _lib, model, ops
from glam_amd._lib import GlamHipError
from tests.test_host_logic import _header_prototypes, _table_type

NAME = "glam_pair_pool_panel_fwd"
_KW = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")
_SIZES = [1, 70, 1030, 9, 0, 64, 65]


def test_panel_prototypes_match_their_signature_rows():
    """Header and ``SIGNATURES`` type for type; STATUS returns that ``api()`` checks; the ABI version stays 4."""
    protos = _header_prototypes()
    for name in (NAME, "glam_pair_pool_panel_workspace_bytes", "glam_pair_pool_panel_supported"):
        res, args = _lib.SIGNATURES[name]
        assert (_table_type(res), [_table_type(a) for a in args]) == protos[name], name
    p, i64, i32, sz = "pointer", ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    assert protos[NAME] == (i32, [p, p, p, p, p, i64, p, i64, i64, i64, i32, p, p, i32, p, p, p, sz, p])
    assert protos["glam_pair_pool_panel_workspace_bytes"] == (sz, [i64, i64])
    assert protos["glam_pair_pool_panel_supported"] == (i32, [i32])
    assert _lib.ABI_VERSION == 4
    for name in (NAME, "glam_pair_pool_panel_supported"):                      # both return a STATUS
        assert name not in _lib.VALUE_RETURNS
        assert getattr(_lib.api(), name).errcheck is not None and getattr(_lib.load(), name).errcheck is None


def test_panel_queries():
    lib = _lib.load()
    assert [lib.glam_pair_pool_panel_supported(D) for D in (1, 15, 16, 30, 45, 60, 64, 90, 92, 127, 128)] == [0] * 11       # GLAM_OK
    assert [lib.glam_pair_pool_panel_supported(D) for D in (0, -4, 129, 132, 256)] == [_lib.GLAM_E_UNSUPPORTED] * 5
    with pytest.raises(GlamHipError, match="D=132 not in 1..128"):
        _lib.api().glam_pair_pool_panel_supported(132)
    ws = lib.glam_pair_pool_panel_workspace_bytes
    assert ws(24, 7) == 24 * 7 * 8 and ws(0, 7) == 0 and ws(24, 0) == 0 and ws(-1, 7) == 0
    assert ws(1 << 20, 1 << 20) == 8 << 40                                     # (a size_t product, not an int one)


def test_panel_entry_point_rejects_bad_arguments_without_a_gpu():
    f = _lib.load().glam_pair_pool_panel_fwd
    fake = ctypes.c_void_p(4096)                                                # (never dereferenced: each call fails a check first)

    def call(mol=fake, pro=fake, mptr=fake, pptr=fake, work=fake, T=3, sel=fake, Qs=2, L=4, Q=2, D=60, ms=fake, ps=fake, slab=0, out=fake,
             arg=None, ws=fake, wsb=1 << 20):
        return f(mol, pro, mptr, pptr, work, T, sel, Qs, L, Q, D, ms, ps, slab, out, arg, ws, wsb, None)
    nothing = dict(mol=None, pro=None, mptr=None, pptr=None, work=None, sel=None, ms=None, ps=None, out=None, ws=None, wsb=0)
    assert call(L=0, **nothing) == 0 and call(Qs=0, **nothing) == 0             # nothing to do, nothing dereferenced
    assert call(L=0, Qs=0, Q=0, T=0, D=128, **nothing) == 0
    for D in (0, -1, 129, 132):
        assert call(D=D) == _lib.GLAM_E_UNSUPPORTED
        assert call(D=D, **nothing) == _lib.GLAM_E_UNSUPPORTED                  # ... before the pointers are looked at
    for bad in (dict(L=-1), dict(Qs=-1), dict(Q=-1), dict(T=-1), dict(slab=-1), dict(L=2 ** 31), dict(Q=0),
                dict(L=1 << 20, Qs=1 << 20)):
        assert call(**bad) == _lib.GLAM_E_INVALID, bad
    for name in ("mol", "pro", "mptr", "pptr", "work", "sel", "ms", "ps", "out", "ws"):
        assert call(**{name: None}) == _lib.GLAM_E_INVALID, name
    assert call(mol=ctypes.c_void_p(4098)) == _lib.GLAM_E_INVALID               # not even a dword boundary
    assert call(wsb=3 * 4 * 8 - 1) == _lib.GLAM_E_INVALID                       # one byte short of [3 chunks][4 ligands] partials
    assert call(ws=ctypes.c_void_p(4100), wsb=1 << 20) == _lib.GLAM_E_INVALID   # the 8-byte partials on a 4-byte boundary
    with pytest.raises(GlamHipError, match=NAME):
        _lib.api().glam_pair_pool_panel_fwd(None, None, None, None, None, 3, None, 2, 4, 2, 60, None, None, 0, None, None, None, 0, None)


def _expect(sizes, sel):
    """The table the long way round: chunk by chunk."""
    first = np.concatenate([[0], np.cumsum(sizes)])
    rows, ptr = [], [0]
    for j, q in enumerate(sel):
        for c in range(0, sizes[q], 64):
            rows.append([j, first[q] + c, min(64, sizes[q] - c), len(rows)])
        ptr.append(len(rows))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4), np.asarray(ptr)


def test_panel_plan_all_proteins():
    plan = ops.panel_plan(_SIZES, None)
    assert plan.sel.dtype == np.int32 and plan.sel.tolist() == list(range(7)) and (plan.Qs, plan.Q, plan.N) == (7, 7, sum(_SIZES))
    assert np.diff(plan.chunk_ptr).tolist() == [1, 2, 17, 1, 0, 1, 2] and plan.total_chunks == 24
    assert plan.work.dtype == np.int32 and plan.work.shape == (4 * 24 + 8,)
    rows, ptr = _expect(_SIZES, range(7))
    assert np.array_equal(plan.chunks, rows) and np.array_equal(plan.chunk_ptr, ptr)
    assert plan.chunks[0].tolist() == [0, 0, 1, 0]
    assert plan.chunks[1:3].tolist() == [[1, 1, 64, 1], [1, 65, 6, 2]]                       # 70 rows: one chunk and six rows over
    assert plan.chunks[3].tolist() == [2, 71, 64, 3] and plan.chunks[19].tolist() == [2, 71 + 16 * 64, 6, 19]      # 1 030 = 16 * 64 + 6
    assert plan.chunks[20].tolist() == [3, 1101, 9, 20]
    assert plan.chunks[21].tolist() == [5, 1110, 64, 21]                                     # (protein 4 is empty: no chunk) exactly one chunk
    assert plan.chunks[22:].tolist() == [[6, 1174, 64, 22], [6, 1238, 1, 23]]                # one row over
    assert np.array_equal(plan.chunks[:, 3], np.arange(24)), "a chunk's partials sit at its own number"


@pytest.mark.parametrize("as_type", [list, np.asarray, torch.tensor, lambda s: np.asarray(s, dtype=np.uint8)])
def test_panel_plan_permuted_and_duplicated_selection(as_type):
    sel = [2, 0, 5, 2]
    plan = ops.panel_plan(np.asarray(_SIZES), as_type(sel))
    assert plan.sel.tolist() == sel and plan.sel.dtype == np.int32 and (plan.Qs, plan.Q) == (4, 7)
    assert np.diff(plan.chunk_ptr).tolist() == [17, 1, 1, 17] and plan.total_chunks == 36
    rows, ptr = _expect(_SIZES, sel)
    assert np.array_equal(plan.chunks, rows) and np.array_equal(plan.chunk_ptr, ptr)
    assert plan.chunks[0].tolist() == [0, 71, 64, 0] and plan.chunks[17].tolist() == [1, 0, 1, 17]
    assert plan.chunks[18].tolist() == [2, 1110, 64, 18] and plan.chunks[19].tolist() == [3, 71, 64, 19]       # the duplicate: its own chunks
    assert plan.chunks[-1].tolist() == [3, 71 + 1024, 6, 35]


def test_panel_plan_edges_and_refusals():
    empty = ops.panel_plan(_SIZES, [])
    assert (empty.Qs, empty.total_chunks) == (0, 0) and empty.work.tolist() == [0]
    only_empty = ops.panel_plan(_SIZES, [4, 4])
    assert (only_empty.Qs, only_empty.total_chunks) == (2, 0) and only_empty.work.tolist() == [0, 0, 0]
    assert ops.panel_plan([], None).Qs == 0
    assert ops.panel_plan(torch.tensor(_SIZES), None).total_chunks == 24
    for bad in ([0, 7], [-1, 0], np.asarray([7])):
        with pytest.raises(IndexError, match=r"proteins must lie in \[0, 7\)"):
            ops.panel_plan(_SIZES, bad)
    with pytest.raises(IndexError, match="proteins must hold integers"):
        ops.panel_plan(_SIZES, [2.0, 0.0])
    with pytest.raises(IndexError, match="proteins must hold integers"):
        ops.panel_plan(_SIZES, torch.tensor([True, False]))
    with pytest.raises(IndexError, match="vector"):
        ops.panel_plan(_SIZES, [[2, 0]])
    with pytest.raises(GlamHipError, match="proteins lives on a device.*read-back"):
        ops.panel_plan(_SIZES, torch.zeros(2, dtype=torch.int64, device="meta"))
    with pytest.raises(GlamHipError, match="sizes live on a device"):
        ops.panel_plan(torch.zeros(2, dtype=torch.int64, device="meta"), None)
    with pytest.raises(IndexError, match="non-negative integers"):
        ops.panel_plan([3, -1], None)
    with pytest.raises(IndexError, match="non-negative integers"):
        ops.panel_plan([3.0, 1.0], None)
    with pytest.raises(IndexError, match="2\\^31"):
        ops.panel_plan([2 ** 30, 2 ** 30], None)


class _Sp:
    B = 3
    N = 10
    ptr = None


def _fake_encoding(net):
    """``screen_panel`` looks at the encoding's model and stamp, then at the selection, before any tensor of it."""
    return model.ProteinEncoding(net, [None, None], _Sp(), None, net._protein_stamp())


def test_screen_panel_contract_is_refused_before_any_device_work():
    net, other = model.ArchitectureDTI(**_KW), model.ArchitectureDTI(**_KW).eval()
    enc = _fake_encoding(net)
    assert enc.sizes_host is None and enc.prosum is None and enc.plans == {}
    with torch.no_grad(), pytest.raises(GlamHipError, match="screen_panel: the model is in training mode"):
        net.screen_panel(None, enc)
    net.eval()
    with pytest.raises(GlamHipError, match="screen_panel is inference only.*no_grad"):
        net.screen_panel(None, enc)
    with torch.no_grad():
        with pytest.raises(GlamHipError, match="pro_flat's norm _LayerNorm"):
            model.ArchitectureDTI(**_KW, flat_norm="_LayerNorm").eval().screen_panel(None, enc)
        with pytest.raises(GlamHipError, match="screen_panel: .*another model"):
            other.screen_panel(None, enc)
        with pytest.raises(GlamHipError, match="screen_panel: .*another model"):
            net.screen_panel(None, object())
        for bad in ([0, 3], [-1], np.asarray([3])):                       # the selection: on the host, before the sizes are read back
            with pytest.raises(IndexError, match=r"proteins must lie in \[0, 3\)"):
                net.screen_panel(None, enc, bad)
        with pytest.raises(IndexError, match="proteins must hold integers"):
            net.screen_panel(None, enc, [1.0])
        with pytest.raises(GlamHipError, match="proteins lives on a device"):
            net.screen_panel(None, enc, torch.zeros(2, dtype=torch.int64, device="meta"))
        assert enc.sizes_host is None and enc.plans == {}
        next(net.pro_conv.parameters()).add_(1)
        with pytest.raises(GlamHipError, match="screen_panel: the encoding is stale"):
            net.screen_panel(None, enc)
        with pytest.raises(GlamHipError, match="stale"):                  # ... and a head-side write leaves a fresh one valid
            net.screen_panel(None, enc, [0])
        enc = _fake_encoding(net)
        next(net.lin_out0.parameters()).add_(1)
        with pytest.raises(IndexError):
            net.screen_panel(None, enc, [5])


@pytest.mark.parametrize("end_norm,one_pass", [("_None", True), ("_BatchNorm", True), ("_LayerNorm", False), ("_PairNorm", False),
                                               ("_GraphSizeNorm", False)])
def test_screen_panel_head_route(end_norm, one_pass):
    """Per-row norms (``_None``; ``_BatchNorm`` on running statistics) let the head run once over the ``L * Qs`` rows; a batch-less norm
    that looks across its whole input must see one protein column at a time.  ONE such norm in either block is enough."""
    net = model.ArchitectureDTI(**_KW, end_norm=end_norm).eval()
    assert net._panel_head_in_one_pass() is one_pass
    mixed = model.ArchitectureDTI(**_KW).eval()
    assert mixed._panel_head_in_one_pass()
    mixed.lin_out1.norm = net.lin_out1.norm
    assert mixed._panel_head_in_one_pass() is one_pass
    # the other slots do not matter to the head
    assert model.ArchitectureDTI(**_KW, graph_norm="_LayerNorm", pre_norm="_PairNorm", flat_norm="_BatchNorm").eval()._panel_head_in_one_pass()
