"""The contract of ``ops.pair_map`` (csrc/pairmap.hip) restated in torch, and the assertions that hold an implementation against it.

Pair ``i`` is segment ``a = idx1[i]`` of ``x1`` (rows ``m0 .. m0 + n1``) against segment ``b = idx2[i]`` of ``x2`` (rows ``p0 .. p0 + n2``);
``None`` is the identity on that side.  ``s(r1, r2)`` is one fmaf chain over the channels in ascending order from 0.  Side 1, per row
``r1``: ``max1 = max_r2 s``, ``arg1 = p0 +`` the smallest ``r2`` that attains it, ``mean1 = (sum_r2 s) / n2`` with the sum taken in ascending
``r2``; side 2 the same the other way (``arg2`` a row of ``x1``, divided by ``n1``).  The outputs are ragged and pair-major (``out_ptr1`` /
``out_ptr2``).  An empty partner gives ``max = 0, mean = 0, arg = -1``; an empty side has no rows.

``restate(..., dtype=torch.float32)`` follows the chain and the sum order (an fmaf is the fp64 sum of the exact product, rounded to
fp32 — exact up to a double rounding); ``dtype=torch.float64`` is its twin, a plain matmul.  ``wrong=`` names a deliberately wrong
restatement (``WRONG``): tests/test_pair_map_host.py shows that each fails the assertions below, which tests/test_gpu_pair_map.py
applies to the kernel."""
import types

import numpy as np
import torch

from tests.conftest import assert_fp32_parity

WRONG = ("last_tie", "local_arg", "own_size", "skip_first_chunk", "neg_inf_empty")
CHUNK = 64
FIELDS = ("max1", "arg1", "mean1", "max2", "arg2", "mean2")


def batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])


def gathered(x, sizes, idx):
    """Rows and sizes of the segments ``idx`` laid out one copy per pair (what a collated batch of the selected graphs holds)."""
    off = ptr_of(sizes)
    rows = torch.cat([x[off[q]:off[q + 1]] for q in idx]) if len(idx) else x[:0]
    return rows, [sizes[q] for q in idx]


def scores(A, B, dtype):
    """``S[r1, r2]``: fp64 — the matmul; fp32 — the ascending fmaf chain from 0."""
    if dtype == torch.float64:
        return A.double() @ B.double().T
    S = torch.zeros(A.size(0), B.size(0), dtype=torch.float32)
    for c in range(A.size(1)):
        S = (S.double() + A[:, c, None].double() * B[None, :, c].double()).float()
    return S


def _marginal(S, first_row, own_n, dtype, wrong):
    """max / arg / mean over dim 1 of ``S[own, partner]`` (``first_row``: the partner segment's first row in its matrix)."""
    n, pn = S.shape
    if pn == 0:
        fill = float("-inf") if wrong == "neg_inf_empty" else 0.0
        return (torch.full((n,), fill, dtype=dtype), torch.full((n,), -1, dtype=torch.int32), torch.zeros(n, dtype=dtype),
                torch.zeros(n, dtype=torch.bool))
    if wrong == "skip_first_chunk" and pn > CHUNK:
        T, shift = S[:, CHUNK:], CHUNK
    else:
        T, shift = S, 0
    mx = T.max(dim=1).values
    cols = torch.arange(T.size(1)).expand_as(T)
    hit = T == mx[:, None]
    local = torch.where(hit, cols, -1).max(dim=1).values if wrong == "last_tie" else torch.where(hit, cols, T.size(1)).min(dim=1).values
    arg = (local + shift + (0 if wrong == "local_arg" else first_row)).to(torch.int32)
    total = torch.zeros(n, dtype=dtype)
    for r in range(T.size(1)):                        # ascending partner order, one add per score
        total = total + T[:, r]
    mean = total / torch.tensor(float(own_n if wrong == "own_size" else pn), dtype=dtype)
    unique = hit.sum(dim=1) == 1
    return mx, arg, mean, unique


def restate(x1, x2, sizes1, sizes2, idx1=None, idx2=None, dtype=torch.float32, wrong=None):
    """The six outputs, ``out_ptr1`` / ``out_ptr2`` (int64 numpy), ``unique1`` / ``unique2`` (the row's maximum occurs once) and per
    pair the fusion's own ``fmax`` / ``farg`` (first flattened occurrence; 0 and -1, -1 for an empty pair) and ``fmean``, the mean of
    the pair's ``mean1`` rows."""
    assert wrong is None or wrong in WRONG
    o1, o2 = ptr_of(sizes1), ptr_of(sizes2)
    P = len(idx1) if idx1 is not None else len(idx2) if idx2 is not None else len(sizes1)
    a = list(range(P)) if idx1 is None else [int(v) for v in idx1]
    b = list(range(P)) if idx2 is None else [int(v) for v in idx2]
    parts = {k: [] for k in FIELDS + ("unique1", "unique2")}
    fmax, farg, fmean = torch.zeros(P, dtype=dtype), torch.full((P, 2), -1, dtype=torch.int32), torch.zeros(P, dtype=dtype)
    for i in range(P):
        m0, n1, p0, n2 = int(o1[a[i]]), sizes1[a[i]], int(o2[b[i]]), sizes2[b[i]]
        S = scores(x1[m0:m0 + n1], x2[p0:p0 + n2], dtype)
        for side, M, first, own in ((1, S, p0, n1), (2, S.T, m0, n2)):
            for k, t in zip(("max", "arg", "mean", "unique"), _marginal(M, first, own, dtype, wrong)):
                parts[f"{k}{side}"].append(t)
        if n1 and n2:
            flat = S.reshape(-1)
            first = int((flat == flat.max()).nonzero()[0])
            fmax[i], fmean[i] = flat.max(), parts["mean1"][-1].mean()
            farg[i, 0], farg[i, 1] = m0 + first // n2, p0 + first % n2
    out = {k: torch.cat(v) if v else torch.zeros(0) for k, v in parts.items()}
    out.update(out_ptr1=ptr_of([sizes1[q] for q in a]), out_ptr2=ptr_of([sizes2[q] for q in b]), fmax=fmax, farg=farg, fmean=fmean,
               P=P, seg1=[(int(o1[q]), sizes1[q]) for q in a], seg2=[(int(o2[q]), sizes2[q]) for q in b])
    return types.SimpleNamespace(**out)


def as_host(pm):
    """An ``ops.PairMap`` (or anything with its fields) as CPU tensors."""
    return types.SimpleNamespace(**{k: getattr(pm, k).detach().cpu() for k in FIELDS},
                                 out_ptr1=np.asarray(getattr(pm, "out_ptr1").cpu() if torch.is_tensor(pm.out_ptr1) else pm.out_ptr1, dtype=np.int64),
                                 out_ptr2=np.asarray(getattr(pm, "out_ptr2").cpu() if torch.is_tensor(pm.out_ptr2) else pm.out_ptr2, dtype=np.int64))


# ---------------------------------------------------------------------------------------------
# the assertions
# ---------------------------------------------------------------------------------------------
def assert_layout(got, ref, what):
    assert np.array_equal(got.out_ptr1, ref.out_ptr1) and np.array_equal(got.out_ptr2, ref.out_ptr2), f"{what}: out_ptr"
    for k in FIELDS:
        t = getattr(got, k)
        assert t.shape == getattr(ref, k).shape and t.dtype == (torch.int32 if k.startswith("arg") else torch.float32), f"{what}: {k}"


def assert_parity(got, ref64, ref32, what):
    """Maxima and means within the fp64-twin bound (k = 8); ``arg`` equal to the fp32 restatement's wherever its maximum is unique."""
    assert_layout(got, ref32, what)
    for k in ("max1", "mean1", "max2", "mean2"):
        assert torch.isfinite(getattr(got, k)).all(), f"{what}: {k} is not finite"
        assert_fp32_parity(getattr(got, k), getattr(ref64, k), getattr(ref32, k), f"{what} {k}", k=8)
    for side in (1, 2):
        u = getattr(ref32, f"unique{side}")
        g, r = getattr(got, f"arg{side}"), getattr(ref32, f"arg{side}")
        assert torch.equal(g[u], r[u]), f"{what}: arg{side} differs where the maximum is unique"
        assert torch.equal(g[~u] < 0, r[~u] < 0), f"{what}: arg{side} fill"


def assert_exact(got, ref64, what):
    """Small-integer rows (every score exact): all six outputs against the fp64 brute force, the means to 1e-6."""
    assert_layout(got, ref64, what)
    for side in (1, 2):
        assert torch.equal(getattr(got, f"max{side}").double(), getattr(ref64, f"max{side}")), f"{what}: max{side}"
        assert torch.equal(getattr(got, f"arg{side}"), getattr(ref64, f"arg{side}")), f"{what}: arg{side} (ties go to the smallest row)"
        assert (getattr(got, f"mean{side}").double() - getattr(ref64, f"mean{side}")).abs().max().item() <= 1e-6, f"{what}: mean{side}"


def assert_fills(got, ref, what):
    """Empty partner: 0, -1, 0 on every row of the other side."""
    for side, own, par in ((1, ref.seg1, ref.seg2), (2, ref.seg2, ref.seg1)):
        ptr = getattr(got, f"out_ptr{side}")
        for i in range(ref.P):
            rows = slice(int(ptr[i]), int(ptr[i + 1]))
            assert rows.stop - rows.start == own[i][1], f"{what}: pair {i} side {side} holds {rows.stop - rows.start} rows"
            if par[i][1] == 0 and own[i][1]:
                assert (getattr(got, f"max{side}")[rows] == 0).all() and (getattr(got, f"mean{side}")[rows] == 0).all(), f"{what}: fill pair {i}"
                assert (getattr(got, f"arg{side}")[rows] == -1).all(), f"{what}: fill arg pair {i}"


def assert_ties_back(got, ref64, ref32, fusion_out, fusion_arg, what):
    """The maps against the fusion's own ``[max, mean]`` / argmax of the same pairs (``ops.pair_pool_gather(return_argmax=True)``), bit for
    bit: the largest ``max1`` of a pair = the largest ``max2`` = the max column; the first row that holds it, with its ``arg1``, is the
    argmax, and ``arg2`` at the argmax's second row is its first row; the mean over a pair's ``mean1`` rows is the mean column within
    the twin bound."""
    fusion_out, fusion_arg = fusion_out.detach().cpu(), fusion_arg.detach().cpu()
    pair_mean = torch.zeros(ref64.P, dtype=torch.float64)
    for i in range(ref64.P):
        (m0, n1), (p0, n2) = ref64.seg1[i], ref64.seg2[i]
        if n1 == 0 or n2 == 0:
            assert fusion_out[i].abs().max().item() == 0 and (fusion_arg[i] == -1).all()
            continue
        r1 = slice(int(got.out_ptr1[i]), int(got.out_ptr1[i + 1]))
        r2 = slice(int(got.out_ptr2[i]), int(got.out_ptr2[i + 1]))
        top = fusion_out[i, 0]
        assert torch.equal(got.max1[r1].max(), top) and torch.equal(got.max2[r2].max(), top), f"{what}: pair {i}: max of the maps != fusion max"
        star = int((got.max1[r1] == top).nonzero()[0])
        assert [m0 + star, int(got.arg1[r1][star])] == fusion_arg[i].tolist(), f"{what}: pair {i}: (first best row, its arg1) != fusion argmax"
        assert int(got.arg2[r2][int(fusion_arg[i, 1]) - p0]) == int(fusion_arg[i, 0]), f"{what}: pair {i}: arg2 at the argmax's row"
        pair_mean[i] = got.mean1[r1].double().mean()
    assert_fp32_parity(pair_mean, ref64.fmean, ref32.fmean, f"{what} mean of mean1 per pair", k=8)
    assert_fp32_parity(fusion_out[:, 1], ref64.fmean, ref32.fmean, f"{what} fusion mean", k=8)


# ---------------------------------------------------------------------------------------------
# the cases (shared by the host and the GPU tests; built once)
# ---------------------------------------------------------------------------------------------
# Sizes on both sides from {0, 1, 2, 3, 63, 64, 65, 70, 130}: below, at and above the 64-row chunk on the owner side, odd tails and a
# lone row on the streamed side, three chunks, and an empty segment on either side.  Pair 3 has an empty second side, pair 6 an empty
# first side, pair 8 both; segment 7 of side 1 and 5 of side 2 are referenced twice; P = 1, 4, 5, 9 are prefixes.
SIZES1 = [1, 2, 3, 63, 64, 65, 70, 130, 0]
SIZES2 = [130, 0, 65, 3, 70, 1, 64, 2, 63]
IDX1 = [7, 3, 4, 2, 5, 6, 8, 7, 8]
IDX2 = [0, 8, 2, 1, 5, 6, 4, 5, 1]
WIDTHS = (4, 15, 60, 64, 92, 128)
PAIRS = (1, 4, 5, 9)


def random_case(D):
    g = torch.Generator().manual_seed(1000 + D)
    return torch.randn(sum(SIZES1), D, generator=g), torch.randn(sum(SIZES2), D, generator=g)


# ties: small-integer rows, duplicated rows at 63 / 64 and 0 / 69 of the 70-row segment, and on the small side too
TIE_SIZES1, TIE_SIZES2, TIE_IDX1, TIE_IDX2 = [4, 3, 5], [5, 70], [1, 0, 2, 2], [1, 0, 1, 0]


def tie_case(D):
    g = torch.Generator().manual_seed(D)
    x1 = torch.randint(-1, 2, (sum(TIE_SIZES1), D), generator=g).float()
    x2 = torch.randint(-1, 2, (sum(TIE_SIZES2), D), generator=g).float()
    for a, b in [(3, 0), (2, 1), (5, 4), (6, 4), (9, 7), (10, 8), (11, 7)]:
        x1[a] = x1[b]
    for a, b in [(1, 0), (3, 2), (4, 0), (5 + 69, 5 + 0), (5 + 65, 5 + 3), (5 + 64, 5 + 63)]:
        x2[a] = x2[b]
    return x1, x2


def prefix(ref, P):
    """The first ``P`` pairs of a restatement (the outputs are pair-major and a pair's rows do not depend on the other pairs)."""
    n1, n2 = int(ref.out_ptr1[P]), int(ref.out_ptr2[P])
    cut = {k: getattr(ref, k)[:n1 if k.endswith("1") else n2] for k in FIELDS + ("unique1", "unique2")}
    return types.SimpleNamespace(**cut, out_ptr1=ref.out_ptr1[:P + 1], out_ptr2=ref.out_ptr2[:P + 1], fmax=ref.fmax[:P], farg=ref.farg[:P],
                                 fmean=ref.fmean[:P], P=P, seg1=ref.seg1[:P], seg2=ref.seg2[:P])
