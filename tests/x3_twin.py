"""A CPU twin of the "3 x bf16" products (glam_amd/csrc/bf16x3.h) and a per-element accuracy check that can see its small terms.

Every dense product on the hot path splits each fp32 operand exactly into three bf16 terms, ``x = hi + mid + lo``, and issues six of the
nine partial products (``hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi``) on the bf16 matrix cores with fp32 accumulation.  On unit-scale
``randn`` operands and in max-norm (``max|d| <= tol * max|ref|``, tolerances growing like sqrt(N)) a kernel that loses ``mid.mid``, or
even all three small terms, is indistinguishable from a correct one.  This module supplies

* ``wide``: operands whose elements span 48 binades, so that within every sum ONE term dominates and the error of that term's product is
  not averaged away by the reduction;
* ``cw_err``: the componentwise error ``max_ij |got - ref64|_ij / (|A| @ |B|)_ij`` in units of u = 2^-24;
* ``split3`` / ``emulate``: the split (``x.bfloat16().float()`` is the kernels' round-to-nearest-even conversion) and any subset of the
  nine partial products, accumulated in fp64;
* ``assert_x3_parity``: ``cw_err(got) <= K_PARITY * max(noise32, 1 u)`` where ``noise32`` is the same error of the plain fp32 product
  ``A @ B`` on the CPU — after asserting, on those very operands, that the bound sits at most half way to the error of the best
  five-term product (the "teeth" condition): a test cannot pass on inputs that would not tell a dropped term from a kept one.

On ``wide`` operands (K = 5 .. 1024, 64 x 48 outputs, CPU): fp32 product 2.6 - 11.3 u; six terms, exact accumulation 0.34 - 0.63 u;
``mid.mid`` dropped 125 - 206 u; ``lo.hi`` dropped 89 - 125 u; three terms > 250 u.

K_PARITY is twice the worst ``err / max(noise32, 1 u)`` measured on an MI355X over every check of tests/test_gpu_x3_accuracy.py with the
library in its default mode, rounded up (a max over ~3000 elements of two independent roundings varies by about two between seeds).
Measured worst ratios per entry point (default mode | GLAM_X3=0):

    entry point (kernel)                              default mode      GLAM_X3=0
    glam_ts_gemm (k_tall_x3, k_ts_gemm_x3[_sw])           1.57 (3.4 u)      1.57 (4.6 u)
    glam_ts_gemm_relu / glam_ts_gemm_add                  1.25 / 1.19       0.43 / 1.10
    glam_dense_gemm / its all-ones column (k_dense_x3)    1.54 (10.3 u) / 1.23      same kernel
    glam_linear_dense_fwd / _bwd: y, dx, dw, db           1.11, 1.42, 1.13, 1.29    same kernel
    glam_wgrad_gemm / _add, k_wgrad_x3                    1.53 / 1.26       (k_wgrad)
    glam_wgrad_gemm / _add, k_wgrad (fp32 matrix cores)   0.99 / 1.00       0.99 / 1.00
    glam_wgrad_gemm_split dw, db: k_wgrad_x3 | k_wgrad    1.42, 0.84 | 1.01, 1.07
    glam_wgrad_gemm_linear dw, db: k_wgrad_x3 | k_wgrad   1.27, 1.31 | 1.05, 1.28
    glam_wgrad_gemm_gru_gates_seg: k_wgrad_x3 | k_wgrad   0.90 | 0.88

The worst is 1.57, so K_PARITY = ceil(2 x 1.57) = 4.  The kernels sit at 1 - 10 u where exact accumulation of the six terms gives 0.3 - 0.8 u:
what they add is their fp32 accumulation (the matrix instruction aligns its addends by truncation), the same order as the fp32 matrix
instructions' own error (the GLAM_X3=0 column) and as a CPU fp32 product's.  The teeth condition holds at k = 4 on every operand set of
the module with the smallest margin at 4.5 (K = 300 with a bias and an addend), i.e. up to k = 4 only: a larger k would need other data.

Untested here: subnormal operands (the bf16 matrix cores flush them) and values within one bf16 ulp of FLT_MAX (``hi`` rounds to
infinity).  The GRU and triplet warp-specialised kernels, whose products sit behind sigmoid / tanh / softmax, need a twin of their own.
"""
import os

import torch

U = 2.0 ** -24
K_PARITY = 4

SIX = ("hi.hi", "hi.mid", "mid.hi", "mid.mid", "hi.lo", "lo.hi")
THREE = ("hi.hi", "hi.mid", "mid.hi")
DROPS = ("mid.mid", "hi.lo", "lo.hi")          # the single-term drops of the teeth condition


def without(term):
    return tuple(t for t in SIX if t != term)


def wide(shape, gen, span=24):
    """``randn * 2^randint(-span, span)`` per element, fp32, on the CPU.  With span = 24 magnitudes run from about 2^-45 (a randn draw of
    1e-6) to 2^27: every non-zero ``lo`` term (>= 2^-24 of its value) and every partial product, ``lo.hi`` included (>= 2^-114), is a
    normal number in bf16 and fp32 alike, and a sum of 2^17 products (<= 2^71) is far from overflow."""
    shape = tuple(shape) if not isinstance(shape, int) else (shape,)
    return torch.randn(shape, generator=gen) * torch.exp2(torch.randint(-span, span + 1, shape, generator=gen).float())


def split3(x):
    """``(hi, mid, lo)`` of an fp32 tensor: three bf16-representable fp32 tensors with ``hi + mid + lo == x`` exactly."""
    x = x.float()
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi, mid, lo


def emulate(A, B, terms=SIX):
    """The named partial products of ``A[R, K] @ B[K, C]``, each exact and summed in fp64."""
    pa = dict(zip(("hi", "mid", "lo"), (t.double() for t in split3(A))))
    pb = dict(zip(("hi", "mid", "lo"), (t.double() for t in split3(B))))
    out = torch.zeros(A.size(0), B.size(1), dtype=torch.float64)
    for t in terms:
        a, b = t.split(".")
        out += pa[a] @ pb[b]
    return out


def _extras(extra):
    return [] if extra is None else list(extra) if isinstance(extra, (list, tuple)) else [extra]


def _ref_den(A, B, extra, scale):
    A64, B64 = A.double(), B.double()
    ref, den = A64 @ B64, A64.abs() @ B64.abs()
    for e in _extras(extra):
        ref, den = ref + e.double(), den + e.double().abs()
    if scale is not None:
        ref, den = ref * scale.double(), den * scale.double().abs()
    return ref, den


def cw_err(got, A, B, extra=None, scale=None):
    """``max_ij |got - ref|_ij / den_ij`` in units of u = 2^-24 with ``ref = A @ B (+ extra)`` in fp64 and ``den = |A| @ |B| (+ |extra|)``.
    ``scale`` (an elementwise factor, e.g. the 0 / 1 mask of a ReLU) multiplies both.  Elements whose denominator is 0 must equal the
    reference exactly (``inf`` otherwise).  A NaN anywhere in ``got`` gives NaN, which fails every comparison."""
    ref, den = _ref_den(A, B, extra, scale)
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, f"shape {tuple(g.shape)} vs {tuple(ref.shape)}"
    if g.numel() == 0:
        return 0.0
    if torch.isnan(g).any():
        return float("nan")
    pos = den > 0
    if not torch.equal(g[~pos], ref[~pos]):
        return float("inf")
    if not pos.any():
        return 0.0
    return ((g - ref).abs()[pos] / den[pos]).max().item() / U


def noise32(A, B, extra=None, scale=None):
    """``cw_err`` of the plain fp32 product on the CPU: ``A @ B`` (+ ``extra``) (* ``scale``), every step in fp32."""
    r = A.float() @ B.float()
    for e in _extras(extra):
        r = r + e.float()
    if scale is not None:
        r = r * scale.float()
    return cw_err(r, A, B, extra, scale)


def teeth(A, B, extra=None, scale=None):
    """The smallest ``cw_err`` among the three five-term products (``mid.mid``, ``hi.lo`` or ``lo.hi`` dropped) on these operands.  A term
    that vanishes identically is no drop — an all-ones operand (a bias gradient, a row sum) has neither ``mid`` nor ``lo``, its product
    consists of ``hi.hi + mid.hi + lo.hi`` alone — but at least one of the three must be there."""
    pa, pb = [t.double() for t in split3(A)], [t.double() for t in split3(B)]
    idx = {"hi": 0, "mid": 1, "lo": 2}
    part = {t: pa[idx[t.split(".")[0]]] @ pb[idx[t.split(".")[1]]] for t in SIX}
    worst = float("inf")
    for d in DROPS:
        if not part[d].any():
            continue
        e = sum(part[t] for t in SIX if t != d)
        for x in _extras(extra):
            e = e + x.double()
        if scale is not None:
            e = e * scale.double()
        worst = min(worst, cw_err(e, A, B, extra, scale))
    assert worst < float("inf"), "no small term in these operands"
    return worst


def assert_x3_parity(got, A, B, what, k=K_PARITY, extra=None, scale=None):
    """``got`` (a kernel's ``A @ B (+ extra)``) is as accurate per element as an fp32 product: ``cw_err <= k * max(noise32, 1 u)``.

    First the teeth condition on these very operands: the bound is at most half the error of the best five-term product, so a kernel
    that loses any one small term cannot pass.  Returns ``err / max(noise32, 1 u)``; GLAM_PARITY_REPORT=1 prints it per check."""
    n32 = noise32(A, B, extra, scale)
    bound = k * max(n32, 1.0)
    t = teeth(A, B, extra, scale)
    err = cw_err(got, A, B, extra, scale)
    if os.environ.get("GLAM_PARITY_REPORT"):      # developer aid: every check's error against the fp32 product's (pytest -s)
        print(f"[x3 parity] {what}: err {err:.2f} u noise32 {n32:.2f} u ({err / max(n32, 1.0):.2f}) five-term {t:.1f} u", flush=True)
    assert bound <= 0.5 * t, (f"{what}: the operands do not discriminate: bound {bound:.1f} u (k = {k:g}, fp32 noise {n32:.1f} u) "
                              f"> half the error of a five-term product ({t:.1f} u)")
    assert err <= bound, (f"{what}: componentwise error {err:.2f} u > {k:g} x max(fp32 product's {n32:.2f} u, 1 u) "
                          f"(a five-term product: {t:.1f} u)")
    return err / max(n32, 1.0)
