"""CPU: the restatement of tests/pair_map_restated.py, which tests/test_gpu_pair_map.py holds the HIP kernel against, and the host
side of ``ops.map_plan``.  Three things are established here, without a GPU:

* the restatement, in both precisions, IS a brute-force score matrix on small-integer rows (every dot product exact), ties and empty
  sides included;
* ``map_plan`` covers every owner row exactly once, lays the outputs out pair-major through the indices and refuses what it must;
* the cases discriminate: five wrong kernels, written as mutations of the restatement and evaluated in fp32, each fail the very
  assertions the GPU tests apply, on the GPU tests' own cases."""
import functools

import numpy as np
import pytest
import torch

from glam_amd import ops
from glam_amd._lib import GlamHipError
from tests import pair_map_restated as R


# ---------------------------------------------------------------------------------------------
# the restatement against a brute force
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 15])
def test_restatement_is_the_brute_force_on_exact_rows(D):
    x1, x2 = R.tie_case(D)
    s1, s2 = R.TIE_SIZES1 + [0], R.TIE_SIZES2 + [0]                 # (an empty segment on either side, referenced below)
    i1, i2 = R.TIE_IDX1 + [3, 0, 3], R.TIE_IDX2 + [1, 2, 2]
    r32, r64 = (R.restate(x1, x2, s1, s2, i1, i2, dt) for dt in (torch.float32, torch.float64))
    o1, o2 = R.ptr_of(s1), R.ptr_of(s2)
    ties = 0
    for i, (a, b) in enumerate(zip(i1, i2)):
        A, B = x1[o1[a]:o1[a + 1]], x2[o2[b]:o2[b + 1]]
        S = torch.tensor([[sum(float(u) * float(v) for u, v in zip(ra, rb)) for rb in B] for ra in A], dtype=torch.float64).reshape(len(A), len(B))
        for side, M, first in ((1, S, int(o2[b])), (2, S.T, int(o1[a]))):
            ptr = getattr(r64, f"out_ptr{side}")
            rows = slice(int(ptr[i]), int(ptr[i + 1]))
            assert rows.stop - rows.start == M.size(0)
            for r in (r32, r64):
                mx, arg, mean = (getattr(r, f"{k}{side}")[rows] for k in ("max", "arg", "mean"))
                if M.size(1) == 0:
                    assert (mx == 0).all() and (mean == 0).all() and (arg == -1).all()
                    continue
                for k in range(M.size(0)):
                    want = max(M[k].tolist())
                    assert mx[k].item() == want and arg[k].item() == first + M[k].tolist().index(want)
                    assert abs(mean[k].item() - sum(M[k].tolist()) / M.size(1)) <= 1e-6
                    ties += M[k].tolist().count(want) > 1
    assert ties > 20, "the case must hold ties"
    R.assert_exact(R.as_host(r32), r64, "fp32 restatement on exact rows")


def test_restatement_twins_agree_on_random_rows():
    x1, x2 = R.random_case(60)
    r32, r64 = (R.restate(x1, x2, R.SIZES1, R.SIZES2, R.IDX1, R.IDX2, dt) for dt in (torch.float32, torch.float64))
    R.assert_parity(R.as_host(r32), r64, r32, "fp32 restatement")
    R.assert_fills(R.as_host(r32), r64, "fp32 restatement")
    R.assert_ties_back(R.as_host(r32), r64, r32, torch.stack([r32.fmax, r32.fmean], 1), r32.farg, "fp32 restatement")
    assert r32.unique1.float().mean() > 0.9


# ---------------------------------------------------------------------------------------------
# map_plan
# ---------------------------------------------------------------------------------------------
def _covered(plan, sizes1, sizes2, a, b):
    """Every (pair, side, owner row) -> the output row the table gives it, with a check that no row is given twice."""
    seen = {}
    for it, (wa, wb, sc, o0) in enumerate(plan.work.tolist()):
        i, side, chunk = int(plan.pair_of_item[it]), sc & 1, sc >> 1
        assert (wa, wb) == (a[i], b[i])
        own = sizes2[wb] if side else sizes1[wa]
        assert 0 <= chunk * ops.MAP_CHUNK < own, "an item without owner rows"
        for r in range(chunk * ops.MAP_CHUNK, min(own, (chunk + 1) * ops.MAP_CHUNK)):
            assert (i, side, r) not in seen
            seen[(i, side, r)] = o0 + r - chunk * ops.MAP_CHUNK
    return seen


@pytest.mark.parametrize("mode", ["both", "idx1", "idx2", "neither", "swapped", "duplicated"])
def test_map_plan_covers_every_owner_row_once(mode):
    s1, s2 = R.SIZES1, R.SIZES2
    i1, i2 = {"both": (R.IDX1, R.IDX2), "idx1": (list(range(9))[::-1], None), "idx2": (None, np.asarray(R.IDX2)), "neither": (None, None),
              "swapped": (torch.tensor(R.IDX2), tuple(R.IDX1)), "duplicated": ([7, 7, 7, 0], [0, 0, 4, 0])}[mode]
    plan = ops.map_plan(s1, np.asarray(s2), i1, i2)
    P = plan.P
    a = list(range(P)) if i1 is None else [int(v) for v in i1]
    b = list(range(P)) if i2 is None else [int(v) for v in i2]
    assert (plan.Q1, plan.Q2, plan.N1, plan.N2) == (9, 9, sum(s1), sum(s2))
    assert plan.out_ptr1.dtype == plan.out_ptr2.dtype == plan.work.dtype == np.int32 and plan.work.shape == (plan.n_items, 4)
    assert np.array_equal(plan.out_ptr1, R.ptr_of([s1[q] for q in a])) and np.array_equal(plan.out_ptr2, R.ptr_of([s2[q] for q in b]))
    assert (plan.R1, plan.R2) == (int(plan.out_ptr1[-1]), int(plan.out_ptr2[-1]))
    seen = _covered(plan, s1, s2, a, b)
    want = {(i, side, r): int((plan.out_ptr2 if side else plan.out_ptr1)[i]) + r
            for i in range(P) for side, n in ((0, s1[a[i]]), (1, s2[b[i]])) for r in range(n)}
    assert seen == want
    assert plan.n_items == sum(-(-s1[a[i]] // 64) - (-s2[b[i]] // 64) for i in range(P))
    assert (np.diff(plan.pair_of_item) >= 0).all(), "a pair's items are consecutive"
    assert np.array_equal(ops.map_plan(s1, s2, i1, i2).work, plan.work)


def test_map_plan_of_no_pairs_and_of_empty_sides():
    plan = ops.map_plan([3, 4], [5], [], [])
    assert (plan.P, plan.R1, plan.R2, plan.n_items) == (0, 0, 0, 0) and plan.out_ptr1.tolist() == [0] == plan.out_ptr2.tolist()
    plan = ops.map_plan([3, 0], [0, 5], [0, 1, 1], [0, 1, 0])         # a partner that is empty keeps its items; an empty side has none
    assert plan.work.tolist() == [[0, 0, 0, 0], [1, 1, 1, 0]] and plan.pair_of_item.tolist() == [0, 1]
    assert plan.out_ptr1.tolist() == [0, 3, 3, 3] and plan.out_ptr2.tolist() == [0, 0, 5, 5]


def test_map_plan_refusals():
    s1, s2 = [3, 4, 2], [5, 6]
    ok1, ok2 = [0, 2, 1, 1], [1, 0, 0, 1]
    for bad1, bad2 in (([0, 3, 1, 1], ok2), ([0, -1, 1, 1], ok2), (ok1, [1, 2, 0, 1]), (ok1, [1, 0, 0]), (ok1, [1, 0, 0, 1, 1]),
                       (ok1, None), (None, ok2), (None, None), ([0.0, 1.0, 1.0, 1.0], ok2)):      # range, length, identity with Q != P, dtype
        with pytest.raises(IndexError):
            ops.map_plan(s1, s2, bad1, bad2)
    for bad in ([3, -1, 2], [[3, 4, 2]], [3.0, 4.0, 2.0]):
        with pytest.raises(IndexError, match="sizes of side 1"):
            ops.map_plan(bad, s2, ok1, ok2)
    with pytest.raises(IndexError, match="sizes of side 2"):
        ops.map_plan(s1, [5, -6], ok1, ok2)
    with pytest.raises(IndexError, match="2\\^31"):
        ops.map_plan([2 ** 30, 2 ** 30], [1], [0, 1], [0, 0])
    meta = torch.empty(4, dtype=torch.int64, device="meta")
    with pytest.raises(GlamHipError, match="idx1 lives on a device.*read-back"):
        ops.map_plan(s1, s2, meta, ok2)
    with pytest.raises(GlamHipError, match="sizes of side 2 live on a device"):
        ops.map_plan(s1, torch.empty(2, dtype=torch.int64, device="meta"), ok1, ok2)
    with pytest.raises(GlamHipError, match="map_plan"):
        ops.pair_map(None, None, None, None, plan=[[0, 0, 0, 0]])


# ---------------------------------------------------------------------------------------------
# the cases discriminate
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs(kind, D):
    if kind == "random":
        x1, x2 = R.random_case(D)
        args = (x1, x2, R.SIZES1, R.SIZES2, R.IDX1, R.IDX2)
    else:
        x1, x2 = R.tie_case(D)
        args = (x1, x2, R.TIE_SIZES1, R.TIE_SIZES2, R.TIE_IDX1, R.TIE_IDX2)
    return args, R.restate(*args, torch.float32), R.restate(*args, torch.float64)


def _gpu_assertions(kind, D, got):
    """What tests/test_gpu_pair_map.py asserts of the kernel's outputs on this case."""
    _, r32, r64 = _refs(kind, D)
    if kind == "random":
        R.assert_parity(got, r64, r32, "case")
        R.assert_fills(got, r64, "case")
        R.assert_ties_back(got, r64, r32, torch.stack([r32.fmax, r32.fmean], 1), r32.farg, "case")
    else:
        R.assert_exact(got, r64, "case")


@pytest.mark.parametrize("kind,D", [("random", 15), ("ties", 8)])
def test_the_right_restatement_passes(kind, D):
    args, r32, _ = _refs(kind, D)
    _gpu_assertions(kind, D, R.as_host(r32))


@pytest.mark.parametrize("wrong,kind,D,fails", [
    ("last_tie", "ties", 8, "ties go to the smallest row"),
    ("local_arg", "random", 15, "arg. differs where the maximum is unique"),
    ("own_size", "random", 15, "mean"),
    ("skip_first_chunk", "random", 15, "max"),
    ("neg_inf_empty", "random", 15, "not finite")])
def test_a_wrong_kernel_fails_the_gpu_assertions(wrong, kind, D, fails):
    args, _, _ = _refs(kind, D)
    got = R.as_host(R.restate(*args, torch.float32, wrong=wrong))
    with pytest.raises(AssertionError, match=fails):
        _gpu_assertions(kind, D, got)
