"""CPU: the host side of the DDI interaction matrix (``ArchitectureDDI.score_matrix`` / ``ops.pair_pool_grid``, csrc/pairgrid.hip) — the C
prototypes of the grid fusion against their ctypes rows, the entry point's argument checks by status code, the packed lane table of
``ops.grid_plan`` and its refusals, a numpy restatement of the two kernels off that table against a brute-force maximum (with three wrong
restatements that must fail), and the refusals of ``score_matrix``: everything that runs before anything is launched and needs no device."""
import ctypes

import numpy as np
import pytest
import torch

from glam_amd import _lib, model, ops, ops_pair
from glam_amd._lib import GlamHipError
from tests.grid_restated import WRONG, brute_force, grid_restated
from tests.test_host_logic import _header_prototypes, _table_type

NAME = "glam_pair_pool_grid_fwd"
_ALL = (NAME, "glam_pair_pool_grid_workspace_bytes", "glam_pair_pool_grid_supported")
_KW = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")
_COLS = [20, 20, 20, 20, 63, 1, 64, 65, 130, 0, 5]          # the packing case: column-side sizes
_ROWS = [1, 2, 33, 0, 7]                                      # row-side sizes


def test_grid_prototypes_match_their_signature_rows_and_are_exported():
    """Header and ``SIGNATURES`` type for type; STATUS returns that ``api()`` checks; the ABI version stays 4; the library has them."""
    protos = _header_prototypes()
    for name in _ALL:
        res, args = _lib.SIGNATURES[name]
        assert (_table_type(res), [_table_type(a) for a in args]) == protos[name], name
        assert hasattr(_lib.load(), name), f"{name} is not exported"
    p, i64, i32, sz = "pointer", ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    assert protos[NAME] == (i32, [p, p, p, p, p, i64, p, i64, p, i64, i64, i64, i64, i32, p, p, i32, p, p, p, sz, p])
    assert protos["glam_pair_pool_grid_workspace_bytes"] == (sz, [i64, i64])
    assert protos["glam_pair_pool_grid_supported"] == (i32, [i32])
    assert _lib.ABI_VERSION == 4
    for name in (NAME, "glam_pair_pool_grid_supported"):                        # both return a STATUS
        assert name not in _lib.VALUE_RETURNS
        assert getattr(_lib.api(), name).errcheck is not None and getattr(_lib.load(), name).errcheck is None


def test_grid_queries():
    lib = _lib.load()
    assert [lib.glam_pair_pool_grid_supported(D) for D in (1, 15, 16, 60, 64, 92, 127, 128)] == [0] * 8                 # GLAM_OK
    assert [lib.glam_pair_pool_grid_supported(D) for D in (0, -4, 129, 132)] == [_lib.GLAM_E_UNSUPPORTED] * 4
    with pytest.raises(GlamHipError, match="D=129 not in 1..128"):
        _lib.api().glam_pair_pool_grid_supported(129)
    ws = lib.glam_pair_pool_grid_workspace_bytes
    assert ws(13, 7) == 13 * 7 * 8 and ws(0, 7) == 0 and ws(13, 0) == 0 and ws(-1, 7) == 0
    assert ws(1 << 20, 1 << 20) == 8 << 40                                      # (a size_t product, not an int one)


def test_grid_entry_point_rejects_bad_arguments_without_a_gpu():
    f = _lib.load().glam_pair_pool_grid_fwd
    fake = ctypes.c_void_p(4096)                                                # (never dereferenced: each call fails a check first)

    def call(x1=fake, x2=fake, p1=fake, p2=fake, rows=fake, R=4, cols=fake, Cs=2, work=fake, T=3, NP=3, Q1=5, Q2=2, D=60, s1=fake, s2=fake,
             slab=0, out=fake, arg=None, ws=fake, wsb=1 << 20):
        return f(x1, x2, p1, p2, rows, R, cols, Cs, work, T, NP, Q1, Q2, D, s1, s2, slab, out, arg, ws, wsb, None)
    nothing = dict(x1=None, x2=None, p1=None, p2=None, rows=None, cols=None, work=None, s1=None, s2=None, out=None, ws=None, wsb=0)
    assert call(R=0, **nothing) == 0 and call(Cs=0, **nothing) == 0             # nothing to do, nothing dereferenced
    assert call(R=0, Cs=0, Q1=0, Q2=0, T=0, NP=0, D=128, **nothing) == 0
    for D in (0, 129):
        assert call(D=D) == _lib.GLAM_E_UNSUPPORTED
        assert call(D=D, **nothing) == _lib.GLAM_E_UNSUPPORTED                  # ... before the pointers are looked at
    for bad in (dict(R=-1), dict(slab=-1), dict(Cs=-1), dict(Q1=-1), dict(Q2=-1), dict(T=-1), dict(NP=-1), dict(R=2 ** 31), dict(Q2=0),
                dict(R=1 << 20, Cs=1 << 20), dict(NP=2), dict(rows=None)):     # (rows = NULL: the identity needs R == Q1)
        assert call(**bad) == _lib.GLAM_E_INVALID, bad
    for name in ("x1", "x2", "p1", "p2", "cols", "work", "s1", "s2", "out", "ws"):
        assert call(**{name: None}) == _lib.GLAM_E_INVALID, name
    assert call(x2=ctypes.c_void_p(4098)) == _lib.GLAM_E_INVALID                # not even a dword boundary
    assert call(wsb=3 * 4 * 8 - 1) == _lib.GLAM_E_INVALID                       # one byte short of [3 partials][4 row drugs]
    assert call(ws=ctypes.c_void_p(4100)) == _lib.GLAM_E_INVALID                # the 8-byte partials on a 4-byte boundary
    with pytest.raises(GlamHipError, match=NAME):
        _lib.api().glam_pair_pool_grid_fwd(*[None] * 5, 4, None, 2, None, 3, 3, 5, 2, 60, None, None, 0, None, None, None, 0, None)


# ---------------------------------------------------------------------------------------------
# ops.grid_plan
# ---------------------------------------------------------------------------------------------
def _runs(plan, w):
    """The chunk's lanes as runs ``(partial, first lane, lanes)``; the idle tail as partial -1."""
    pid = plan.lanes[w, :, 3].tolist()
    out = []
    for lane, p in enumerate(pid):
        if out and out[-1][0] == p:
            out[-1][2] += 1
        else:
            out.append([p, lane, 1])
    return [tuple(r) for r in out]


def _check_cover(plan, sizes):
    """Every selected row sits in exactly one lane, with its own b / n2 / partial; ``part_ptr`` covers every partial exactly once; an
    idle lane holds the row of lane 0."""
    first = np.concatenate([[0], np.cumsum(sizes)])
    want = [(first[q] + k, k, sizes[q], plan.part_ptr[j] + k // 64) for j, q in enumerate(plan.sel.tolist()) for k in range(sizes[q])]
    live = plan.lanes.reshape(-1, 4)[plan.lanes.reshape(-1, 4)[:, 3] >= 0]
    assert sorted(map(tuple, live.tolist())) == sorted(tuple(int(v) for v in t) for t in want)
    assert live.shape[0] == len(want), "a selected row in two lanes"
    n_part = [(sizes[q] + 63) // 64 for q in plan.sel.tolist()]
    assert plan.part_ptr.tolist() == [0] + np.cumsum(n_part).tolist() and plan.n_partials == sum(n_part)
    assert sorted(set(live[:, 3].tolist())) == list(range(plan.n_partials)), "a partial without a lane, or a lane without a partial"
    for w in range(plan.total_chunks):
        assert plan.lanes[w, 0, 3] >= 0, "lane 0 of every chunk holds a row"
        idle = plan.lanes[w, :, 3] < 0
        assert (plan.lanes[w, idle, 0] == plan.lanes[w, 0, 0]).all() and (plan.lanes[w, idle, 1:3] == 0).all()
        pids = [p for p, _, _ in _runs(plan, w)]
        assert len(pids) == len(set(pids)), "the lanes of one partial are contiguous"
    assert abs(plan.fill - len(want) / max(64 * plan.total_chunks, 1)) < 1e-12


def test_grid_plan_packs_small_drugs_and_slices_large_ones():
    plan = ops.grid_plan(_COLS, None)
    assert plan.sel.dtype == np.int32 and plan.sel.tolist() == list(range(11)) and (plan.Cs, plan.Q, plan.N) == (11, 11, sum(_COLS))
    assert plan.work.dtype == np.int32 and plan.work.shape == (256 * 10 + 12,) and plan.lanes.shape == (10, 64, 4)
    assert (plan.total_chunks, plan.n_partials) == (10, 13)
    assert plan.part_ptr.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 12, 13]                 # 65 -> 2, 130 -> 3, the empty drug none
    assert _runs(plan, 0) == [(0, 0, 20), (1, 20, 20), (2, 40, 20), (-1, 60, 4)]             # three drugs, four idle lanes
    assert _runs(plan, 1) == [(3, 0, 20), (-1, 20, 44)]                                      # the fourth 20 alone: 63 does not fit behind it
    assert _runs(plan, 2) == [(4, 0, 63), (5, 63, 1)]                                        # 63 + 1: exactly full
    assert _runs(plan, 3) == [(6, 0, 64)]                                                    # 64 alone
    assert _runs(plan, 4) == [(7, 0, 64)] and _runs(plan, 5) == [(8, 0, 1), (-1, 1, 63)]     # 65 -> 2 slices, the last one not shared
    assert [_runs(plan, w) for w in (6, 7, 8)] == [[(9, 0, 64)], [(10, 0, 64)], [(11, 0, 2), (-1, 2, 62)]]       # 130 -> 3 slices
    assert _runs(plan, 9) == [(12, 0, 5), (-1, 5, 59)]                                       # 5 alone (the empty drug: no lane)
    assert plan.lanes[0, 20].tolist() == [20, 0, 20, 1] and plan.lanes[0, 59].tolist() == [59, 19, 20, 2]
    assert plan.lanes[2, 63].tolist() == [143, 0, 1, 5]
    assert plan.lanes[5, 0].tolist() == [208 + 64, 64, 65, 8], "b runs on through the slices of a drug"
    assert plan.lanes[8, 1].tolist() == [273 + 129, 129, 130, 11]
    _check_cover(plan, _COLS)


def test_grid_plan_seventy_one_row_drugs():
    plan = ops.grid_plan([1] * 70, None)
    assert (plan.total_chunks, plan.n_partials) == (2, 70)
    assert _runs(plan, 0) == [(p, p, 1) for p in range(64)], "64 groups in one chunk"
    assert _runs(plan, 1) == [(64 + p, p, 1) for p in range(6)] + [(-1, 6, 58)]
    _check_cover(plan, [1] * 70)


@pytest.mark.parametrize("as_type", [list, np.asarray, torch.tensor, lambda s: np.asarray(s, dtype=np.uint8)])
def test_grid_plan_permuted_and_duplicated_selection(as_type):
    sel = [8, 0, 0, 5, 9, 2]
    plan = ops.grid_plan(np.asarray(_COLS), as_type(sel))
    assert plan.sel.tolist() == sel and plan.sel.dtype == np.int32 and (plan.Cs, plan.Q) == (6, 11)
    assert plan.part_ptr.tolist() == [0, 3, 4, 5, 6, 6, 7] and plan.n_partials == 7 and plan.total_chunks == 4
    assert _runs(plan, 2) == [(2, 0, 2), (-1, 2, 62)], "the last slice of the 130-row drug is not shared"
    assert _runs(plan, 3) == [(3, 0, 20), (4, 20, 20), (5, 40, 1), (6, 41, 20), (-1, 61, 3)]      # the duplicate: lanes and a partial of its own
    assert plan.lanes[3, 0].tolist() == plan.lanes[3, 20].tolist()[:3] + [3] and plan.lanes[3, 20, 3] == 4
    _check_cover(plan, _COLS)


def test_grid_plan_edges_refusals_and_the_staged_idiom():
    empty = ops.grid_plan(_COLS, [])
    assert (empty.Cs, empty.total_chunks, empty.n_partials) == (0, 0, 0) and empty.work.tolist() == [0]
    only_empty = ops.grid_plan(_COLS, [9, 9])
    assert (only_empty.Cs, only_empty.total_chunks, only_empty.n_partials) == (2, 0, 0) and only_empty.work.tolist() == [0, 0, 0]
    none = ops.grid_plan([], None)
    assert (none.Cs, none.Q, none.N, none.total_chunks) == (0, 0, 0, 0)
    assert ops.grid_plan(torch.tensor(_COLS), None).total_chunks == 10
    for bad in ([0, 11], [-1, 0], np.asarray([11])):
        with pytest.raises(IndexError, match=r"cols must lie in \[0, 11\)"):
            ops.grid_plan(_COLS, bad)
    with pytest.raises(IndexError, match="cols must hold integers"):
        ops.grid_plan(_COLS, [2.0, 0.0])
    with pytest.raises(IndexError, match="cols must hold integers"):
        ops.grid_plan(_COLS, torch.tensor([True, False]))
    with pytest.raises(IndexError, match=r"cols must be a vector of segment numbers: shape \(1, 2\)$"):
        ops.grid_plan(_COLS, [[2, 0]])
    with pytest.raises(GlamHipError, match="^cols lives on a device.*read-back"):
        ops.grid_plan(_COLS, torch.zeros(2, dtype=torch.int64, device="meta"))
    with pytest.raises(GlamHipError, match="grid_plan: the segments' sizes live on a device"):
        ops.grid_plan(torch.zeros(2, dtype=torch.int64, device="meta"), None)
    for bad in ([3, -1], [3.0, 1.0], [[3, 1]]):
        with pytest.raises(IndexError, match="grid_plan: the segments' sizes must be a vector of non-negative integers"):
            ops.grid_plan(bad, None)
    with pytest.raises(IndexError, match="2\\^31"):
        ops.grid_plan([2 ** 30, 2 ** 30], None)
    with pytest.raises(IndexError, match="2\\^31"):                             # the rows fit, the selection's partials do not
        ops.grid_plan([2 ** 30], np.zeros(128, dtype=np.int64))
    # one staged-copy holder: ``on`` and the per-device cache come from _Staged
    assert issubclass(ops.GridPlan, ops_pair._Staged) and "on" not in vars(ops.GridPlan) and ops.GridPlan.on is ops_pair._Staged.on
    plan = ops.grid_plan([70, 3], [1, 0])
    assert plan._parts[0] is plan.sel and plan._parts[1] is plan.work and plan._dev == {}
    assert ops.grid_plan is ops_pair.grid_plan and ops.pair_pool_grid is ops_pair.pair_pool_grid


# ---------------------------------------------------------------------------------------------
# the kernels restated off the table
# ---------------------------------------------------------------------------------------------
def _exact_inputs():
    """Small-integer rows (every product and sum exact) with duplicated rows: ties inside a drug, between packed neighbours of one chunk
    (drugs 0 and 1), between the slices of the 130-row drug, and on the first side.  The first row of drug 8 — the row behind the last
    row of the 65-row drug — is twice a first-side row without a zero: reading past the end of drug 7 would show."""
    g = np.random.default_rng(3)
    D = 8
    ptr1, ptr2 = np.concatenate([[0], np.cumsum(_ROWS)]), np.concatenate([[0], np.cumsum(_COLS)])
    x1 = g.integers(-1, 2, (ptr1[-1], D)).astype(np.float32)
    x2 = g.integers(-1, 2, (ptr2[-1], D)).astype(np.float32)
    x1[3] = np.where(x1[3] == 0, 1, x1[3])                    # row 0 of row drug 2: no zero
    x1[10], x1[36] = x1[3], x1[3]                             # ... again inside drug 2 and in drug 4
    x2[5] = x2[17] = x1[3]                                    # drug 0, twice
    x2[20 + 5] = x2[20 + 2] = x1[3]                           # drug 1, its packed neighbour
    for k in (3, 64 + 3, 129):                                # the three slices of drug 8
        x2[ptr2[8] + k] = x1[3]
    x2[ptr2[7] + 64] = x2[ptr2[7] + 1] = x1[3]                # both slices of drug 7
    x2[ptr2[8]] = 2 * x1[3]
    return x1, x2, ptr1, ptr2


@pytest.mark.parametrize("rows,cols", [([2, 0, 4, 2, 3, 1], None), (None, [8, 0, 0, 5, 9, 2])], ids=["picked rows", "picked cols"])
def test_restated_kernels_agree_with_brute_force_exactly(rows, cols):
    x1, x2, ptr1, ptr2 = _exact_inputs()
    plan = ops.grid_plan(_COLS, cols)
    want, want_arg = brute_force(x1, x2, ptr1, ptr2, list(range(5)) if rows is None else rows, plan.sel.tolist())
    out, arg = grid_restated(x1, x2, ptr1, ptr2, plan, rows)
    assert np.array_equal(out, want) and np.array_equal(arg, want_arg)
    i, j = (0, 0) if rows is not None else (2, 1)              # row drug 2 against column drug 0: the tie, won by the first occurrence
    assert out[i, j, 0] == 8 and arg[i, j].tolist() == [3, 5]
    live = [(i, j) for i in range(out.shape[0]) for j in range(out.shape[1]) if want_arg[i, j, 0] >= 0]
    assert len(live) < out.shape[0] * out.shape[1], "the case must hold empty drugs on both sides"


@pytest.mark.parametrize("wrong", WRONG)
def test_wrong_restatements_fail_on_these_inputs(wrong):
    """The comparison above sees each of the mistakes the packed layout invites."""
    x1, x2, ptr1, ptr2 = _exact_inputs()
    rows = [2, 0, 4, 2, 3, 1]
    plan = ops.grid_plan(_COLS, None)
    want, want_arg = brute_force(x1, x2, ptr1, ptr2, rows, plan.sel.tolist())
    out, arg = grid_restated(x1, x2, ptr1, ptr2, plan, rows, wrong=wrong)
    assert not (np.array_equal(out, want) and np.array_equal(arg, want_arg)), f"the wrong restatement '{wrong}' passes"
    if wrong == "full_last_slice":
        assert out[0, 7, 0] == 16 and want[0, 7, 0] == 8, "the idle lanes of drug 7's last slice read drug 8's first row"


# ---------------------------------------------------------------------------------------------
# ArchitectureDDI.score_matrix: refused on the host
# ---------------------------------------------------------------------------------------------
class _Sp:
    B = 3
    N = 10
    ptr = None


def _fake_encoding(net):
    """``score_matrix`` looks at the encoding's model and stamp, then at both selections, before any tensor of it."""
    return model.DrugEncoding(net, [None, None], [None, None], _Sp(), None, None, net._drug_stamp())


def test_score_matrix_contract_is_refused_before_any_device_work():
    net, other = model.ArchitectureDDI(**_KW), model.ArchitectureDDI(**_KW).eval()
    enc = _fake_encoding(net)
    assert enc.sizes_host is None and enc.sum1 is None and enc.sum2 is None and enc.plans == {}
    with torch.no_grad(), pytest.raises(GlamHipError, match="score_matrix: the model is in training mode"):
        net.score_matrix(enc)
    net.eval()
    with pytest.raises(GlamHipError, match="score_matrix is inference only.*no_grad"):
        net.score_matrix(enc)
    with torch.no_grad():
        with pytest.raises(GlamHipError, match="mol2_flat's norm _LayerNorm|mol1_flat's norm _LayerNorm"):
            model.ArchitectureDDI(**_KW, flat_norm="_LayerNorm").eval().score_matrix(enc)
        with pytest.raises(GlamHipError, match="score_matrix: .*another model"):
            other.score_matrix(enc)
        with pytest.raises(GlamHipError, match="score_matrix: .*another model"):
            net.score_matrix(object())
        for bad in ([0, 3], [-1], np.asarray([3])):                    # both selections: on the host, before the sizes are read back
            with pytest.raises(IndexError, match=r"rows must lie in \[0, 3\)"):
                net.score_matrix(enc, rows=bad)
            with pytest.raises(IndexError, match=r"cols must lie in \[0, 3\)"):
                net.score_matrix(enc, cols=bad)
        with pytest.raises(IndexError, match="cols must hold integers"):
            net.score_matrix(enc, cols=[1.0])
        with pytest.raises(GlamHipError, match="rows lives on a device"):
            net.score_matrix(enc, rows=torch.zeros(2, dtype=torch.int64, device="meta"))
        with pytest.raises(GlamHipError, match="cols lives on a device"):
            net.score_matrix(enc, cols=torch.zeros(2, dtype=torch.int64, device="meta"))
        for bad in (-1, 2.5, True):
            with pytest.raises(GlamHipError, match="block_pairs"):
                net.score_matrix(enc, block_pairs=bad)
        assert enc.sizes_host is None and enc.plans == {}
        next(net.mol2_conv.parameters()).add_(1)
        with pytest.raises(GlamHipError, match="score_matrix: the encoding is stale"):
            net.score_matrix(enc)
        enc = _fake_encoding(net)                                      # ... and a head-side write leaves a fresh one valid
        next(net.lin_out0.parameters()).add_(1)
        with pytest.raises(IndexError):
            net.score_matrix(enc, cols=[5])


@pytest.mark.parametrize("end_norm,one_pass", [("_None", True), ("_BatchNorm", True), ("_LayerNorm", False), ("_PairNorm", False),
                                               ("_GraphSizeNorm", False)])
def test_score_matrix_head_route_and_blocks(end_norm, one_pass):
    net = model.ArchitectureDDI(**_KW, end_norm=end_norm).eval()
    assert net._matrix_head_in_one_pass() is one_pass
    # e_dim = 64: 512 MiB / (64 * 4 B) = 2 Mi pair rows per block
    assert net._matrix_block_rows(0, 5000, 1000) == (2 << 20) // 1000 and net._matrix_block_rows(0, 9, 9) == 9
    assert net._matrix_block_rows(0, 7, 4 << 20) == 1, "at least one row drug"
    assert net._matrix_block_rows(9, 7, 9) == 1 and net._matrix_block_rows(10 ** 9, 7, 9) == 7 and net._matrix_block_rows(20, 7, 9) == 2
    assert model.ArchitectureDDI()._matrix_block_rows(0, 2000, 2000) == (512 << 20) // (2000 * 1024 * 4) == 65
