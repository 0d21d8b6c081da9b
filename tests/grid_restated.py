"""The grid fusion (csrc/pairgrid.hip) restated in numpy, lane by lane off the table of ``ops.grid_plan``: per-lane best under ``better``,
the segmented reduction in its six shuffle steps, the finish.  Not a test module: ``tests/test_ddi_matrix_host.py`` compares it with a
brute-force per-pair maximum on inputs whose every product is exact, and checks that each of the deliberately WRONG variants below
(``wrong=``) fails on them — so that the comparison is known to see the mistakes the packed layout invites:

``"unsegmented"``      the whole-wave reduction of the panel kernel: a partner lane is combined whatever partial it belongs to;
``"lane_index"``       the flattened index built from the lane number, as in the panel kernel, instead of the row inside the lane's own drug;
``"full_last_slice"``  the last slice of a drug of more than 64 rows counts 64 rows: its idle lanes read on past the drug's end."""
import numpy as np

NEG, BIG = np.float32(-np.inf), 0x7fffffff
WRONG = ("unsegmented", "lane_index", "full_last_slice")


def better(v, ix, best, bidx):
    return v > best or (v == best and ix < bidx)


def brute_force(x1, x2, ptr1, ptr2, rows, cols):
    """Per pair: the maximum of ``S = x1[seg a] @ x2[seg q].T``, its FIRST flattened occurrence as (row of x1, row of x2), the mean."""
    out = np.zeros((len(rows), len(cols), 2), dtype=np.float32)
    arg = np.full((len(rows), len(cols), 2), -1, dtype=np.int64)
    for i, a in enumerate(rows):
        for j, q in enumerate(cols):
            n1, n2 = ptr1[a + 1] - ptr1[a], ptr2[q + 1] - ptr2[q]
            if n1 == 0 or n2 == 0:
                continue
            S = x1[ptr1[a]:ptr1[a + 1]].astype(np.float64) @ x2[ptr2[q]:ptr2[q + 1]].astype(np.float64).T
            first = int(np.argmax(S.reshape(-1)))                    # (numpy: the first occurrence)
            out[i, j] = S.max(), np.float32(S.sum()) / (np.float32(n1) * np.float32(n2))
            arg[i, j] = ptr1[a] + first // n2, ptr2[q] + first % n2
    return out, arg


def grid_restated(x1, x2, ptr1, ptr2, plan, rows=None, wrong=None):
    """``out`` float32 ``[R, Cs, 2]`` and ``arg`` int64 ``[R, Cs, 2]`` the way the two kernels compute them."""
    assert wrong is None or wrong in WRONG
    rows = np.arange(len(ptr1) - 1) if rows is None else np.asarray(rows)
    R, Cs, D = len(rows), plan.Cs, x1.shape[1]
    ws_v = np.full((plan.n_partials, R), np.nan, dtype=np.float32)          # (a partial nobody writes would show)
    ws_i = np.full((plan.n_partials, R), -7, dtype=np.int64)
    written = np.zeros((plan.n_partials, R), dtype=np.int64)
    for w in range(plan.total_chunks):
        t = plan.lanes[w].astype(np.int64)                                   # [64, 4]: row of x2, b, n2, partial
        if wrong == "full_last_slice":
            for lane in range(1, 64):
                if t[lane, 3] < 0 and t[lane - 1, 2] > 64:
                    t[lane] = min(t[lane - 1, 0] + 1, x2.shape[0] - 1), t[lane - 1, 1] + 1, t[lane - 1, 2], t[lane - 1, 3]
        pid = t[:, 3]
        held = x2[t[:, 0]].astype(np.float32)                                # every lane holds a valid row, idle ones too
        for i, a in enumerate(rows):
            m0, n1 = ptr1[a], ptr1[a + 1] - ptr1[a]
            best, bidx = [NEG] * 64, [BIG] * 64
            S = x1[m0:m0 + n1].astype(np.float32) @ held.T                   # [n1, 64] (every product and sum exact on these inputs: the
            for lane in range(64):                                           #  kernel's ascending chain gives the same numbers)
                if pid[lane] < 0:
                    continue                                                 # (the kernel: a select that leaves -inf, 0x7fffffff)
                for r1 in range(n1):
                    v = S[r1, lane]
                    ix = r1 * t[lane, 2] + (lane if wrong == "lane_index" else t[lane, 1])
                    if better(v, ix, best[lane], bidx[lane]):
                        best[lane], bidx[lane] = v, ix
            o = 1
            while o < 64:                                                    # __shfl_down by 1, 2, 4, ... 32
                nb, ni = list(best), list(bidx)
                for lane in range(64 - o):
                    if (wrong == "unsegmented" or pid[lane + o] == pid[lane]) and better(best[lane + o], bidx[lane + o], best[lane], bidx[lane]):
                        nb[lane], ni[lane] = best[lane + o], bidx[lane + o]
                best, bidx, o = nb, ni, 2 * o
            for lane in range(64):
                if pid[lane] >= 0 and (lane == 0 or pid[lane - 1] != pid[lane]):
                    ws_v[pid[lane], i], ws_i[pid[lane], i] = best[lane], bidx[lane]
                    written[pid[lane], i] += 1
    assert (written == 1).all(), "every partial is stored exactly once per first-side drug"
    sum1 = np.stack([x1[ptr1[a]:ptr1[a + 1]].sum(0) for a in range(len(ptr1) - 1)]).astype(np.float32).reshape(-1, D)
    sum2 = np.stack([x2[ptr2[q]:ptr2[q + 1]].sum(0) for q in range(len(ptr2) - 1)]).astype(np.float32).reshape(-1, D)
    out = np.zeros((R, Cs, 2), dtype=np.float32)
    arg = np.full((R, Cs, 2), -1, dtype=np.int64)
    for i, a in enumerate(rows):
        for j, q in enumerate(plan.sel):
            n1, n2 = ptr1[a + 1] - ptr1[a], ptr2[q + 1] - ptr2[q]
            if n1 <= 0 or n2 <= 0:
                continue
            best, bidx = NEG, BIG
            for c in range(plan.part_ptr[j], plan.part_ptr[j + 1]):
                if better(ws_v[c, i], ws_i[c, i], best, bidx):
                    best, bidx = ws_v[c, i], ws_i[c, i]
            tot = np.float32(0)
            for c in range(D):
                tot = np.float32(tot + sum1[a, c] * sum2[q, c])
            out[i, j] = best, tot / (np.float32(n1) * np.float32(n2))
            arg[i, j] = ptr1[a] + bidx // n2, ptr2[q] + bidx % n2
    return out, arg
