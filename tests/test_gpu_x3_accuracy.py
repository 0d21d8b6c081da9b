"""The 3 x bf16 products (glam_amd/csrc/bf16x3.h) per element on wide-range operands: every dense entry point against the fp64
product in the componentwise metric of tests/x3_twin.py, which a kernel that loses one of the six partial products cannot pass.

Each case builds ``wide`` operands on the CPU (every element ``randn * 2^randint(-24, 24)``), runs ONE entry point through ctypes with
NaN-filled outputs and calls ``assert_x3_parity`` — which first asserts, on those operands, that the bound is at most half the error
of the best five-term product.  The module passes with GLAM_X3=0 as well (the fp32 matrix instructions): that run is the control which
shows the metric asks nothing an fp32 product does not deliver.  The operand builders are plain CPU functions: tests/test_x3_twin_host.py
runs the emulated six-, five- and three-term products through the same assertion on the same operands without a GPU.
"""
import ctypes

import pytest
import torch

from tests import x3_twin as T

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1009 + int(v) + 1
    return torch.Generator().manual_seed(seed % (2 ** 31))


# ---------------------------------------------------------------------------------------------------------------------------------
# operand sets (CPU): one function per entry-point family, shared with the host test
# ---------------------------------------------------------------------------------------------------------------------------------
# (K1, K2, M1, M2) -> the kernel launch_ts_gemm2 (csrc/gemm.hip) picks with the library in its default mode | with GLAM_X3=0, as the
# kernel timer names it.  k_ts_gemm<12, 4, 4> is the label of all three register-B forms (k_ts_gemm_x3_sw, k_ts_gemm_x3 and the fp32
# k_ts_gemm<12, 4, 4, 512>): that GLAM_TS_SW = 1 / 0 reaches the first / second rests on reading launch_ts_gemm2, not on an assertion.
TS_SHAPES = {
    (16, 0, 48, 8): ("k_tall_x3<2, 4, 1>", "k_ts_gemm<4, 12, 4>"),
    (48, 8, 16, 0): ("k_tall_x3<2, 4, 1>", "k_ts_gemm<4, 12, 4>"),
    (20, 0, 12, 0): ("k_tall_x3<2, 4, 1>", "k_ts_gemm<4, 12, 4>"),       # K, M multiples of 4 only: a ragged k group and column tile
    (60, 0, 180, 8): ("k_ts_gemm<12, 4, 4>", "k_ts_gemm<12, 4, 4>"),
    (92, 0, 276, 8): ("k_tall_x3<3, 4, 5>", "k_ts_gemm<20, 6, 4>"),
    (276, 8, 92, 0): ("k_tall_x3<9, 6, 1>", "k_tall_x3<9, 6, 1>"),        # (K > 192: 3 x bf16 only, in both modes)
    (300, 0, 60, 0): ("k_tall_x3<10, 4, 1>", "k_tall_x3<10, 4, 1>"),
    (100, 4, 8, 4): ("k_tall_x3<4, 4, 1>", "k_ts_gemm<4, 12, 4>"),
}
TS_ROWS = (1, 17, 100)
RELU_ROWS = (4, 17, 100)      # (half the outputs of a ReLU are exact zeros: one row of 60 leaves too few elements to tell a dropped term)


def ts_operands(K1, K2, M1, M2, N, bias, tag=0):
    """A[N, K1 + K2], W[K, M1 + M2], bias[M1] or None, and the bias laid out as ``extra`` [N, M] (zero on the M2 columns)."""
    g = _gen(K1, K2, M1, M2, N, bias, tag)
    K, M = K1 + K2, M1 + M2
    A, W = T.wide((N, K), g), T.wide((K, M), g)
    b = T.wide((M1,), g) if bias else None
    extra = None
    if bias:
        extra = torch.zeros(N, M)
        extra[:, :M1] = b
    return A, W, b, extra


DENSE_SHAPES = [(257, 75, 33), (100, 300, 1024)]
DENSE_OPTIONS = [(False, False, False), (True, True, True), (True, False, False), (False, True, True)]      # gate, bias, all-ones column
GATE_SLOPE = 0.25


def dense_operands(R, Cn, K, a_kc, b_kc):
    g = _gen(R, Cn, K, a_kc, b_kc)
    A, G, B, bv = T.wide((R, K), g), torch.randn(R, K, generator=g), T.wide((K, Cn), g), T.wide((Cn,), g)
    return A, G, B, bv


def gated(A, G):
    """A . (G > 0 ? 1 : 1/4): exact in fp32, the operand the kernel splits."""
    return A * torch.where(G > 0, 1.0, GATE_SLOPE)


LINEAR_SHAPES = [(33, 64, 128, 0), (32, 300, 1024, 1), (8, 300, 1024, 0), (64, 1024, 617, 1)]      # N, K, M, act (0 none, 1 ReLU)


def linear_operands(N, K, M):
    g = _gen(N, K, M)
    return T.wide((N, K), g), T.wide((M, K), g), T.wide((M,), g), T.wide((N, M), g)       # x, w, b, dy


WGRAD_ROWS = (1, 31, 32, 33, 65, 1000)
WGRAD_SHAPES = [(48, 8, 0, 16), (180, 8, 0, 60), (184, 4, 1, 64), (300, 16, 1, 64)]      # I1, I2, ones, J


def wgrad_operands(N, I1, I2, ones, J, tag=0):
    g = _gen(N, I1, I2, ones, J, tag)
    P1, P2, Q = T.wide((N, I1), g), T.wide((N, max(I2, 1)), g)[:, :I2].contiguous(), T.wide((N, J), g)
    P = torch.cat([P1, P2] + ([torch.ones(N, 1)] if ones else []), 1)
    return P1, P2, Q, P


WSPLIT_SHAPES = [(60, 15, 16), (180, 60, 60), (320, 44, 48)]      # I, J, ldq
WLINEAR_SHAPES = [(92, 92), (180, 60), (320, 124)]                # I, J


def split_operands(N, I, J, ldq):
    g = _gen(N, I, J, ldq)
    return T.wide((N, I), g), T.wide((N, J), g)


def wlinear_operands(N, I, J):
    g = _gen(N, I, J, 3)
    return T.wide((N, I), g), T.wide((N, J), g), T.wide((I, J), g), T.wide((I,), g)       # P, Q, add_w, add_b


ONES_ALONE = 65      # reduction lengths up to which a product with an all-ones column is also checked on its own


def with_ones(A, B, extra=None, extra_ones=None):
    """The checks of ``A @ [B | 1]`` (a weight gradient with its bias gradient, a product with its row sums), as the kernels compute it: the
    all-ones column is one more column of B.  An all-ones operand has neither ``mid`` nor ``lo``: the only small term of its column is
    ``lo.hi``, at most 2^-17 of a value, and over a reduction longer than the ~49 binades of ``wide`` the largest terms no longer stand
    alone — ~20 of 1000 share the top binade and their ``lo`` average out, so that column ALONE cannot tell a dropped term from fp32
    noise at any k >= 2.  It is checked as part of the whole product at every length (the bound is the whole product's, the teeth the
    other columns') and on its own up to ONES_ALONE terms, where one term dominates.  Yields (suffix, A, B, extra, pick) with
    ``pick(main, ones_col)`` the kernel outputs to compare."""
    K = A.size(1)
    one = torch.ones(K, 1)
    ex = None
    if extra is not None or extra_ones is not None:
        ex = torch.cat([extra if extra is not None else torch.zeros(A.size(0), B.size(1)),
                        extra_ones if extra_ones is not None else torch.zeros(A.size(0), 1)], 1)
    yield " [product | ones column]", A, torch.cat([B, one], 1), ex, lambda main, col: torch.cat([main, col.reshape(-1, 1)], 1)
    if K <= ONES_ALONE:
        yield " ones column", A, one, extra_ones, lambda main, col: col.reshape(-1, 1)


def relu_mask(ref64):
    return (ref64 > 0).double()


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from glam_amd import _lib as L
    return L, L.load(), L.ptr, L.stream


def _x3():
    from glam_amd import _lib as L
    return L.route_enabled("x3")


def _timed(call):
    """Runs ``call()`` under the library's kernel timer: (return code, names of the kernels it launched)."""
    from glam_amd import _lib as L
    with L.kernel_timer(capacity=16) as kt:
        rc = call()
    torch.cuda.synchronize()
    return rc, [n for n, _, _ in kt.records()]


def _ts_image(W, trans, device):
    L, lib, p, st = _lib()
    K, M = W.shape
    Wd = (W.t().contiguous() if trans else W.contiguous()).to(device)
    img = torch.empty(lib.glam_ts_gemm_image_bytes(K, M) // 4, device=device)
    assert lib.glam_ts_gemm_make_image(p(Wd), K if trans else M, trans, K, M, p(img), st()) == 0, lib.glam_last_error()
    return img


def _ts_run(A, W, b, K1, K2, M1, M2, trans, device, pad=4, img=None):
    """glam_ts_gemm on CPU operands: the [N, M1 + M2] result on the CPU; the output rows are ``pad`` floats longer than their matrices
    and the test asserts that the NaN pre-fill there survives."""
    L, lib, p, st = _lib()
    N = A.size(0)
    A1d = A[:, :K1].contiguous().to(device)
    A2d = A[:, K1:].contiguous().to(device) if K2 else None
    img = _ts_image(W, trans, device) if img is None else img
    bd = b.to(device) if b is not None else None
    o1 = torch.full((N, M1 + pad), NAN, device=device)
    o2 = torch.full((N, max(M2, 4) + pad), NAN, device=device)
    rc, names = _timed(lambda: lib.glam_ts_gemm(p(A1d), K1, K1, p(A2d), K2, K2, p(img), p(bd), p(o1), M1, M1 + pad,
                                                p(o2) if M2 else None, M2, max(M2, 4) + pad, N, st()))
    assert rc == 0, lib.glam_last_error()
    assert torch.isnan(o1[:, M1:]).all() and torch.isnan(o2[:, M2:]).all(), "wrote beyond M"
    return torch.cat([o1[:, :M1], o2[:, :M2]], 1).cpu(), names


# ---------------------------------------------------------------------------------------------------------------------------------
# glam_ts_gemm / glam_ts_gemm_make_image
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("shape,sw", [(s, "1") for s in TS_SHAPES] + [((60, 0, 180, 8), "0")])
def test_ts_gemm_per_element(device, monkeypatch, shape, sw, trans, bias):
    """One shape per branch of launch_ts_gemm2 (the kernel-timer label asserts which kernel ran), both weight layouts of make_image, with
    and without bias, N = 1, 17, 100 (one row, a ragged second tile, several blocks).  K = 20, 60, 92, 284, 300 are no multiples of 8 or
    32: ragged k groups.  GLAM_TS_SW = 0 is run for the register-B shape only (the one shape the switch acts on)."""
    K1, K2, M1, M2 = shape
    monkeypatch.setenv("GLAM_TS_SW", sw)
    for N in TS_ROWS:
        A, W, b, extra = ts_operands(K1, K2, M1, M2, N, bias)
        got, names = _ts_run(A, W, b, K1, K2, M1, M2, trans, device)
        assert names == [TS_SHAPES[shape][0 if _x3() else 1]], names
        T.assert_x3_parity(got, A, W, f"ts_gemm {shape} N={N} trans={trans} bias={bias} sw={sw}", extra=extra)


@pytest.mark.parametrize("K,M", [(16, 60), (300, 60)])
def test_ts_gemm_relu_per_element(device, K, M):
    """glam_ts_gemm_relu: the reference clamped in fp64, the sign taken from the kernel's own output (an element within rounding of zero
    may fall on either side) — and required to agree with the reference's wherever that is clear of zero.  With GLAM_X3=0 the 16 -> 60
    shape has no kernel: the entry point must say so and write nothing."""
    L, lib, p, st = _lib()
    for N in RELU_ROWS:
        A, W, b, extra = ts_operands(K, 0, M, 0, N, True, tag=1)
        img = _ts_image(W, 0, device)
        out = torch.full((N, M + 4), NAN, device=device)
        Ad, bd = A.to(device), b.to(device)
        rc, names = _timed(lambda: lib.glam_ts_gemm_relu(p(Ad), K, K, p(img), p(bd), p(out), M, M + 4, N, st()))
        if not lib.glam_ts_gemm_relu_supported(K, M):
            assert not _x3() and rc == L.GLAM_E_UNSUPPORTED and torch.isnan(out).all()
            continue
        assert rc == 0, lib.glam_last_error()
        assert names == [TS_SHAPES[(K, 0, M, 0)][0] if K == 300 else "k_tall_x3<2, 4, 1>"], names
        assert torch.isnan(out[:, M:]).all()
        got = out[:, :M].cpu()
        assert (got >= 0).all()
        ref, den = T._ref_den(A, W, extra, None)
        clear = ref.abs() > 64 * T.K_PARITY * T.U * den
        assert torch.equal((got > 0)[clear], (ref > 0)[clear]), "ReLU on the wrong side of a clearly signed element"
        T.assert_x3_parity(got, A, W, f"ts_gemm_relu {K}->{M} N={N}", extra=extra, scale=(got > 0).double())


@pytest.mark.parametrize("K,M,label", [(180, 60, "k_tall_x3<6, 4, 1, epi>"), (276, 92, "k_tall_x3<9, 6, 1, epi>"), (300, 60, "k_tall_x3<10, 4, 1, epi>"),
                                       (48, 16, "k_tall_x3<2, 4, 1, epi>")])
def test_ts_gemm_add_per_element(device, K, M, label):
    """glam_ts_gemm_add (A @ W + bias + addend[N, M]): the epilogue forms of k_tall_x3, whose tiles carry the addend rows."""
    L, lib, p, st = _lib()
    for N in TS_ROWS:
        A, W, b, extra = ts_operands(K, 0, M, 0, N, True, tag=2)
        add = T.wide((N, M), _gen(K, M, N, 7))
        img = _ts_image(W, 1, device)
        out = torch.full((N, M + 4), NAN, device=device)
        Ad, bd, addd = A.to(device), b.to(device), torch.cat([add, torch.full((N, 4), NAN)], 1).to(device)
        rc, names = _timed(lambda: lib.glam_ts_gemm_add(p(Ad), K, K, p(img), p(bd), p(out), M, M + 4, p(addd), M + 4, N, st()))
        assert rc == 0, lib.glam_last_error()
        if _x3() or K > 192:
            assert names == [label], names
        assert torch.isnan(out[:, M:]).all()
        T.assert_x3_parity(out[:, :M].cpu(), A, W, f"ts_gemm_add {K}->{M} N={N}", extra=[extra, add])


# ---------------------------------------------------------------------------------------------------------------------------------
# glam_dense_gemm, glam_linear_dense_fwd / _bwd (+ the k-split _ws forms)
# ---------------------------------------------------------------------------------------------------------------------------------
def _dense_run(A, G, B, bv, a_kc, b_kc, gate, bias, ones, device):
    L, lib, p, st = _lib()
    (R, K), Cn = A.shape, B.size(1)
    Ad = (A if a_kc else A.t().contiguous()).to(device)
    Gd = (G if a_kc else G.t().contiguous()).to(device) if gate else None
    Bd = (B.t().contiguous() if b_kc else B).to(device)
    bd = bv.to(device) if bias else None
    ldc = Cn + 4
    C = torch.full((R, ldc), NAN, device=device)
    rs = torch.full((R + 4,), NAN, device=device)
    rc = lib.glam_dense_gemm(p(Ad), K if a_kc else 1, 1 if a_kc else R, p(Gd), GATE_SLOPE, p(Bd), 1 if b_kc else Cn, K if b_kc else 1, p(bd), 0,
                             0.0, p(C), ldc, p(rs) if ones else None, R, Cn, K, st())
    assert rc == 0, lib.glam_last_error()
    assert torch.isnan(C[:, Cn:]).all(), "wrote beyond Cn"
    assert torch.isnan(rs[R:]).all() and (ones or torch.isnan(rs).all())
    return C[:, :Cn].cpu(), rs[:R].cpu()


@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("R,Cn,K", DENSE_SHAPES)
def test_dense_gemm_per_element(device, R, Cn, K, a_kc, b_kc):
    """glam_dense_gemm in its four layout combinations (16-byte and scalar access paths, ragged tiles, a partial last k chunk), with the
    gate (it multiplies A before the metric's |A|), the bias and the all-ones column."""
    A, G, B, bv = dense_operands(R, Cn, K, a_kc, b_kc)
    for gate, bias, ones in DENSE_OPTIONS:
        ones = ones and not b_kc
        Ag = gated(A, G) if gate else A
        got, rs = _dense_run(A, G, B, bv, a_kc, b_kc, gate, bias, ones, device)
        what = f"dense_gemm {(R, Cn, K)} a_kc={a_kc} b_kc={b_kc} gate={gate} bias={bias}"
        ex = bv.expand(R, Cn) if bias else None
        T.assert_x3_parity(got, Ag, B, what, extra=ex)
        if ones:
            for sfx, a, b2, e, pick in with_ones(Ag, B, ex):
                T.assert_x3_parity(pick(got, rs), a, b2, what + sfx, extra=e)


@pytest.mark.parametrize("ws", [False, True])
@pytest.mark.parametrize("N,K,M,act", LINEAR_SHAPES)
def test_linear_dense_per_element(device, N, K, M, act, ws):
    """glam_linear_dense_fwd / _bwd and, ws, the forms that split k across blocks (few tiles, a long reduction): y, dx, dw, db each against
    its own operand pair — dw = (dy . gate)^T x, db = (dy . gate)^T 1.  act = 1: ReLU, the mask taken from the kernel's y."""
    L, lib, p, st = _lib()
    x, w, b, dy = linear_operands(N, K, M)
    xd, wd, bd, dyd = (t.to(device) for t in (x, w, b, dy))
    nan = lambda *s: torch.full(s, NAN, device=device)
    y, dx, dw, db = nan(N, M), nan(N, K), nan(M, K), nan(M)
    nb = lib.glam_dense_ws_bytes()
    wsd = torch.full((nb,), 0xFF, dtype=torch.uint8, device=device) if ws else None      # (NaN patterns: nothing of it may reach a result)
    if ws:
        assert lib.glam_linear_dense_fwd_ws(p(xd), p(wd), p(bd), N, K, M, act, 0.0, p(y), p(wsd), nb, st()) == 0, lib.glam_last_error()
        assert lib.glam_linear_dense_bwd_ws(p(xd), p(wd), p(dyd), p(y) if act else None, 0.0, N, K, M, p(dx), p(dw), p(db), p(wsd), nb, st()) == 0, \
            lib.glam_last_error()
    else:
        assert lib.glam_linear_dense_fwd(p(xd), p(wd), p(bd), N, K, M, act, 0.0, p(y), st()) == 0, lib.glam_last_error()
        assert lib.glam_linear_dense_bwd(p(xd), p(wd), p(dyd), p(y) if act else None, 0.0, N, K, M, p(dx), p(dw), p(db), st()) == 0, lib.glam_last_error()
    y, dx, dw, db = y.cpu(), dx.cpu(), dw.cpu(), db.cpu()
    what = f"linear_dense {(N, K, M)} act={act} ws={ws}"
    extra = b.expand(N, M)
    mask = (y > 0).float() if act else torch.ones(N, M)
    if act:
        ref, den = T._ref_den(x, w.t(), extra, None)
        clear = ref.abs() > 64 * T.K_PARITY * T.U * den
        assert (y >= 0).all() and torch.equal((y > 0)[clear], (ref > 0)[clear])
    T.assert_x3_parity(y, x, w.t(), what + " y", extra=extra, scale=mask.double() if act else None)
    g = dy * mask                                                                       # exact: the operand the kernel splits
    T.assert_x3_parity(dx, g, w, what + " dx")
    for sfx, a, b2, e, pick in with_ones(g.t(), x):
        T.assert_x3_parity(pick(dw, db), a, b2, what + " dw" + sfx, extra=e)


# ---------------------------------------------------------------------------------------------------------------------------------
# the weight-gradient products
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["default", "x3"])
def wgrad_route(request, monkeypatch):
    """Both weight-gradient kernels: "default" = k_wgrad (fp32 matrix instructions) below 32 768 rows, "x3" = k_wgrad_x3
    (csrc/wgrad_x3.hip) at every size (GLAM_WGRAD_X3_ROWS is read at each launch)."""
    if request.param == "x3":
        monkeypatch.setenv("GLAM_WGRAD_X3_ROWS", "1")
    return request.param


def _wgrad_kernel(route):
    from glam_amd import _lib as L
    return "k_wgrad_x3<" if route == "x3" and L.route_enabled("wgrad_x3") else "k_wgrad<"


def _ws(device):
    L, lib, p, st = _lib()
    return torch.empty(lib.glam_wgrad_workspace_bytes(), dtype=torch.uint8, device=device)


@pytest.mark.parametrize("I1,I2,ones,J", WGRAD_SHAPES)
@pytest.mark.parametrize("N", WGRAD_ROWS)
def test_wgrad_gemm_per_element(device, wgrad_route, N, I1, I2, ones, J):
    """glam_wgrad_gemm and glam_wgrad_gemm_add, [P1 | P2 | 1]^T Q in both output strides; N straddles k_wgrad_x3's 32-row step and its
    first row split.  The addend is the metric's ``extra``."""
    L, lib, p, st = _lib()
    P1, P2, Q, P = wgrad_operands(N, I1, I2, ones, J)
    I = P.size(1)
    ws = _ws(device)
    P1d, P2d, Qd = P1.to(device), P2.to(device), Q.to(device)
    add = T.wide((I, J), _gen(N, I, J, 11))
    for si, sj, shape in [(J, 1, (I, J)), (1, I, (J, I))]:
        out = torch.full(shape, NAN, device=device)
        rc, names = _timed(lambda: lib.glam_wgrad_gemm(p(P1d), I1, I1, p(P2d) if I2 else None, I2, I2, ones, p(Qd), J, J, 0, N, p(out), si, sj,
                                                       p(ws), ws.numel(), st()))
        assert rc == 0, lib.glam_last_error()
        assert names[0].startswith(_wgrad_kernel(wgrad_route)), names
        got = (out if si == J else out.t()).cpu()
        T.assert_x3_parity(got, P.t(), Q, f"wgrad_gemm N={N} {(I1, I2, ones, J)} strides {(si, sj)} {wgrad_route}")
        addd = (add if si == J else add.t().contiguous()).to(device)
        out = torch.full(shape, NAN, device=device)
        rc = lib.glam_wgrad_gemm_add(p(P1d), I1, I1, p(P2d) if I2 else None, I2, I2, ones, p(Qd), J, J, 0, N, p(out), si, sj, p(addd), p(ws),
                                     ws.numel(), st())
        assert rc == 0, lib.glam_last_error()
        got = (out if si == J else out.t()).cpu()
        T.assert_x3_parity(got, P.t(), Q, f"wgrad_gemm_add N={N} {(I1, I2, ones, J)} strides {(si, sj)} {wgrad_route}", extra=add)


@pytest.mark.parametrize("I,J,ldq", WSPLIT_SHAPES)
@pytest.mark.parametrize("N", WGRAD_ROWS)
def test_wgrad_gemm_split_per_element(device, wgrad_route, N, I, J, ldq):
    """glam_wgrad_gemm_split: dw[I, J] = P^T Q contiguous and db[I] = P^T 1 apart; J = 15 reads rows of Q padded to 16."""
    L, lib, p, st = _lib()
    P, Q = split_operands(N, I, J, ldq)
    Qd = torch.zeros(N, ldq)
    Qd[:, :J] = Q
    Pd, Qd, ws = P.to(device), Qd.to(device), _ws(device)
    dw, db = torch.full((I * J + 8,), NAN, device=device), torch.full((I + 4,), NAN, device=device)
    rc, names = _timed(lambda: lib.glam_wgrad_gemm_split(p(Pd), I, I, p(Qd), J, ldq, p(dw), p(db), N, p(ws), ws.numel(), st()))
    assert rc == 0, lib.glam_last_error()
    assert names[0].startswith(_wgrad_kernel(wgrad_route)), names
    assert torch.isnan(dw[I * J:]).all() and torch.isnan(db[I:]).all()
    what = f"wgrad_gemm_split N={N} {(I, J, ldq)} {wgrad_route}"
    for sfx, a, b2, e, pick in with_ones(P.t(), Q):
        T.assert_x3_parity(pick(dw[:I * J].view(I, J).cpu(), db[:I].cpu()), a, b2, what + sfx, extra=e)


@pytest.mark.parametrize("I,J", WLINEAR_SHAPES)
@pytest.mark.parametrize("N", WGRAD_ROWS)
def test_wgrad_gemm_linear_per_element(device, wgrad_route, N, I, J):
    """glam_wgrad_gemm_linear (up to 127 inputs: beyond 63 as two column chunks in one launch), with both addends."""
    L, lib, p, st = _lib()
    P, Q, aw, ab = wlinear_operands(N, I, J)
    Pd, Qd, awd, abd, ws = P.to(device), Q.to(device), aw.to(device), ab.to(device), _ws(device)
    dw, db = torch.full((I * J + 8,), NAN, device=device), torch.full((I + 4,), NAN, device=device)
    rc, names = _timed(lambda: lib.glam_wgrad_gemm_linear(p(Pd), I, I, p(Qd), J, J, 0, p(dw), p(db), p(awd), p(abd), N, p(ws), ws.numel(), st()))
    assert rc == 0, lib.glam_last_error()
    assert names[0].startswith(_wgrad_kernel(wgrad_route)), names
    assert torch.isnan(dw[I * J:]).all() and torch.isnan(db[I:]).all()
    what = f"wgrad_gemm_linear N={N} {(I, J)} {wgrad_route}"
    for sfx, a, b2, e, pick in with_ones(P.t(), Q, aw, ab[:, None]):
        T.assert_x3_parity(pick(dw[:I * J].view(I, J).cpu(), db[:I].cpu()), a, b2, what + sfx, extra=e)


def gates_operands(N, C, nseg):
    g = _gen(N, C, nseg)
    return [T.wide((N, 4 * C), g) for _ in range(nseg)], [T.wide((N, C), g) for _ in range(nseg)], [T.wide((N, C), g) for _ in range(nseg)]


@pytest.mark.parametrize("N,C", [(1000, 60), (65, 24), (32, 24)])
def test_wgrad_gru_gates_two_segments_per_element(device, wgrad_route, N, C):
    """glam_wgrad_gemm_gru_gates_seg with two operand sets: the sum over the sets is ONE product over the stacked rows."""
    L, lib, p, st = _lib()
    nseg, M = 2, 3 * C
    D, X, H = gates_operands(N, C, nseg)
    Dd, Xd, Hd = ([t.to(device) for t in ts] for ts in (D, X, H))
    arr = lambda ts: (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in ts])
    f = lambda *s: torch.full(s, NAN, device=device)
    got, ws = [f(M, C), f(M), f(M, C), f(M)], _ws(device)
    rc = lib.glam_wgrad_gemm_gru_gates_seg(nseg, arr(Dd), C, arr(Xd), C, 0, arr(Hd), C, p(got[0]), p(got[1]), p(got[2]), p(got[3]), N, p(ws), ws.numel(),
                                           None, None, None, None, st())
    if rc == L.GLAM_E_UNSUPPORTED:      # (k_wgrad: sets shorter than a wave's row range are refused, the caller runs them one by one)
        assert N < 1024 and _wgrad_kernel(wgrad_route) == "k_wgrad<" and all(torch.isnan(t).all() for t in got)
        return
    assert rc == 0, lib.glam_last_error()
    Dall, Xall, Hall = torch.cat(D), torch.cat(X), torch.cat(H)
    dgi, dgh = Dall[:, :M], torch.cat([Dall[:, :2 * C], Dall[:, M:]], 1)
    what = f"gru_gates_seg N={N} C={C} {wgrad_route}"
    got = [t.cpu() for t in got]
    for name, A, B, dw, db in (("ih", dgi.t(), Xall, got[0], got[1]), ("hh", dgh.t(), Hall, got[2], got[3])):
        T.assert_x3_parity(dw, A, B, f"{what} dw_{name}")
        for sfx, a, b2, e, pick in with_ones(A, B):
            T.assert_x3_parity(pick(dw, db), a, b2, f"{what} {name}{sfx}", extra=e)


# ---------------------------------------------------------------------------------------------------------------------------------
# edges: zeros, signed zeros, containment of non-finite values
# ---------------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _runner(kind, device):
    """``run(A, B, bias) -> [R, C] on the CPU`` of one small ragged shape per kernel family, and that shape (R, K, C)."""
    L, lib, p, st = _lib()
    if kind.startswith("ts"):
        K1, K2, M1, M2 = {"ts_tall": (20, 0, 12, 0), "ts_wide": (60, 0, 180, 8), "ts_long": (276, 8, 92, 0), "ts_two": (48, 8, 16, 0)}[kind]
        trans = 1 if kind == "ts_long" else 0
        def run(A, W, b):
            bb = b[:M1].contiguous() if b is not None else None
            return _ts_run(A, W, bb, K1, K2, M1, M2, trans, device)[0]
        return run, (17, K1 + K2, M1 + M2), M1
    if kind.startswith("dense"):
        a_kc, b_kc = {"dense_kc": (True, True), "dense_ck": (False, False)}[kind]
        def run(A, B, b):
            bv = b if b is not None else torch.zeros(B.size(1))
            return _dense_run(A, torch.ones_like(A), B, bv, a_kc, b_kc, False, b is not None, False, device)[0]
        return run, (33, 35, 75), 75
    assert kind in ("wgrad", "wgrad_x3")      # (the fixture sets GLAM_WGRAD_X3_ROWS for the second)
    def run(A, B, b):      # A = P^T [I, N], B = Q [N, J]
        P, Q, ws = A.t().contiguous().to(device), B.contiguous().to(device), _ws(device)
        (N, I), J = P.shape, Q.size(1)
        out = torch.full((I, J + 4), NAN, device=device)
        rc = lib.glam_wgrad_gemm(p(P), I, I, None, 0, 0, 0, p(Q), J, J, 0, N, p(out), J + 4, 1, p(ws), ws.numel(), st())
        assert rc == 0, lib.glam_last_error()
        assert torch.isnan(out[:, J:]).all(), "wrote beyond J"
        return out[:, :J].cpu()
    return run, (52, 37, 20), 0


EDGE_KINDS = ["ts_tall", "ts_two", "ts_wide", "ts_long", "dense_kc", "dense_ck", "wgrad", "wgrad_x3"]


@pytest.fixture(params=EDGE_KINDS)
def edge(request, device, monkeypatch):
    if request.param == "wgrad_x3":
        monkeypatch.setenv("GLAM_WGRAD_X3_ROWS", "1")
    run, shape, nbias = _runner(request.param, device)
    R, K, C = shape
    g = _gen(R, K, C, len(request.param))
    A, B = T.wide((R, K), g), T.wide((K, C), g)
    b = T.wide((C,), g) if nbias else None
    if b is not None:
        b[nbias:] = 0
    return request.param, run, A, B, b


def test_zero_rows_and_columns_give_exact_zeros(edge):
    """An all-zero row of A and an all-zero column of W give exactly zero (or exactly the bias); flipping the sign of those zeros changes no
    bit of any other element, and at most the sign of these."""
    kind, run, A, B, b = edge
    A, B = A.clone(), B.clone()
    r0, c0 = A.size(0) - 1, B.size(1) - 1
    A[r0] = 0
    A[2] = 0
    B[:, c0] = 0
    B[:, 1] = 0
    got = run(A, B, b)
    want = torch.zeros(B.size(1)) if b is None else b
    for r in (2, r0):
        assert torch.equal(got[r], want), (kind, r)
    for c in (1, c0):
        assert torch.equal(got[:, c], want[c].expand(A.size(0))), (kind, c)
    T.assert_x3_parity(got, A, B, f"{kind} with zero rows and columns", extra=None if b is None else b.expand_as(got))
    A2, B2 = A.clone(), B.clone()
    A2[r0] = -0.0
    B2[:, 1] = -0.0
    got2 = run(A2, B2, b)
    assert torch.equal(got2, got), kind            # (== : -0.0 equals 0.0)
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[r0] = False
    keep[:, 1] = False
    assert _same_bits(got2[keep], got[keep]), kind


@pytest.mark.parametrize("value", [NAN, float("inf")])
@pytest.mark.parametrize("where", ["A last", "A first", "B last", "B first"])
def test_non_finite_values_stay_in_their_row_or_column(edge, where, value):
    """One NaN (one +inf) in A at (last row, last k) or (0, 0) of a ragged shape: that output row is NaN (non-finite) throughout, every
    other row keeps every bit, the cells beyond the matrix keep their NaN pre-fill (asserted by the runners); in W: its column, and only
    its column.  The ragged tails re-read the last weight group / row and must zero it by select — a tail zeroed by multiplication
    would carry the NaN into every row."""
    kind, run, A, B, b = edge
    base = run(A, B, b)
    assert torch.isfinite(base).all()
    A2, B2 = A.clone(), B.clone()
    hit = torch.zeros_like(base, dtype=torch.bool)
    if where.startswith("A"):
        r, k = (A.size(0) - 1, A.size(1) - 1) if where.endswith("last") else (0, 0)
        A2[r, k] = value
        hit[r] = True
    else:
        k, c = (B.size(0) - 1, B.size(1) - 1) if where.endswith("last") else (0, 0)
        B2[k, c] = value
        hit[:, c] = True
    got = run(A2, B2, b)
    bad = torch.isnan(got) if value != value else ~torch.isfinite(got)
    assert bad[hit].all(), f"{kind}: {int((~bad[hit]).sum())} finite elements in the affected row / column"
    assert _same_bits(got[~hit], base[~hit]), f"{kind}: {int((got[~hit] != base[~hit]).sum())} elements outside the affected row / column changed"
