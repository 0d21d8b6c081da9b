"""Shared by tests/test_dense_cases_host.py (CPU) and tests/test_gpu_dense_ops.py (GPU): the cases of the dense operators of
``glam_amd/ops_dense.py`` — ``linear``, ``linear_relu``, ``linear_act``, ``matmul_tall``, ``linear_split``, ``gru_tail`` —, one on each side
of every shape predicate that chooses an autograd node or a kernel, with the launches each must make.  Imports neither ``glam_amd.ops``
nor the library.

A ``Case`` names the op, its shape ``N, K, M`` (``gru_tail``: ``K = C``, ``M = 3 C``), its options, the ROUTE (which node, which entry
point) and the product launches expected forward and backward in the library's default mode, as ``_lib.kernel_timer().records()`` names
them.  The expectation is written from the sources: the route by the constructor a case is built with (``_mfma`` = ``_Linear``,
``_narrow`` = ``_LinearNarrow`` ...), the label from the kernel tables restated below (``ts_label`` = ``launch_ts_gemm2`` +
``launch_tall_x3``, ``dense_label`` = ``launch_products``, the ``k_wgrad`` labels of ``launch_wgrad_partials``).  ``classify`` restates
the Python predicates; the host test holds every case's route against it.

Only PRODUCT launches are compared (``product_labels``): weight images, pads, the fixed-order reductions behind a product and zero
fills run under kernel names of their own and follow from the product in front of them.

Every case has ``K != M``: a transposed result has another shape.  Inputs are seeded by the case's name; ``reference`` evaluates the
plain torch restatement once per case in fp64 and fp32 (shared, do not modify)."""
import dataclasses
import functools
import zlib

import torch
import torch.nn.functional as F

import oracle.glam_oracle as O


def ceil4(v):
    return (v + 3) // 4 * 4


# ---- the kernel tables, restated -------------------------------------------------------------------------------------------------------
def linear_supported(K, M):
    Kp, Mp = ceil4(K), ceil4(M)
    return (Kp <= 60 and Mp <= 192) or (Kp <= 188 and Mp <= 64)


def ts_variant(K, M):
    """csrc/gemm.hip: ts_variant — ``[N, K] @ [K, M]``."""
    if M <= 64 and K <= 192:
        return 0
    if K <= 64 and M <= 192:
        return 1
    if K <= 96 and M <= 320:
        return 2
    if K <= 288 and M <= 96:
        return 3
    if K <= 320 and M <= 64:
        return 4
    return -1


def ts_label(K, M, epi=False):
    """The label of one ``glam_ts_gemm*`` launch ``[N, K] @ image(K, M)`` in default mode (3 x bf16 on): ``launch_ts_gemm2`` hands variants
    0, 3, 4 and the plain variant 2 to ``launch_tall_x3``.  ``epi``: a ``celu'`` factor or an addend in the epilogue."""
    v = ts_variant(K, M)
    assert v >= 0, (K, M)
    e = ", epi" if epi else ""
    if v == 0:
        return f"k_tall_x3<{2 if K <= 64 else 4 if K <= 128 else 6}, 4, 1{e}>"
    if v == 1:
        return "k_ts_gemm<12, 4, 4>"
    if v == 2:
        return "k_ts_gemm<20, 6, 4>" if epi else "k_tall_x3<3, 4, 5>"
    if v == 3:
        return f"k_tall_x3<9, 6, 1{e}>"
    return f"k_tall_x3<10, 4, 1{e}>"


WG, WG_CELU, WG_SETS, WG_RELU = "k_wgrad<false>", "k_wgrad<true>", "k_wgrad<true, sets>", "k_wgrad<relu mask>"
GT_F, GT_B = "k_gru_tail_fwd<false>", "k_gru_tail_bwd<false>"
GB_F, GB_B = "k_gru_fwd_ws<false, gates>", "k_gru_bwd_ws<false, gates>"
COLSUM = "k_colsum"


def narrow_label(M, bwd=False):
    return f"k_linear_narrow_{'bwd' if bwd else 'fwd'}<{1 if M == 1 else 2 if M <= 2 else 4 if M <= 4 else 8 if M <= 8 else 16}>"


def dense_label(products, kc_ok=False):
    """csrc/dense_x3.hip: launch_products — ``products = [(rows, columns incl. the all-ones one), ...]``; ``kc_ok``: one product whose
    operands both run along k (the forward)."""
    t64 = sum(-(-r // 64) * -(-c // 64) for r, c in products)
    if kc_ok and len(products) == 1 and t64 >= 128:
        return "k_dense_kc"
    return "k_dense_x3<64>" if t64 >= 100 else "k_dense_x3<32>"


def dense_fwd_label(N, K, M):
    return dense_label([(N, M)], kc_ok=True)


def dense_bwd_label(N, K, M, grad, bias=True):
    db = bias and "b" in grad
    prods = ([(M, K + (1 if db else 0))] if ("w" in grad or db) else []) + ([(N, K)] if "x" in grad else [])
    return dense_label(prods)


_PRODUCT_PREFIXES = ("k_ts_gemm", "k_tall_x3", "k_wgrad", "k_linear_narrow_fwd", "k_linear_narrow_bwd", "k_dense_x3", "k_dense_kc",
                     "k_gru_fwd", "k_gru_bwd", "k_gru_tail", "k_gru_fused_fwd", "k_gru_gates")


def product_labels(names):
    """The product launches among the recorded kernel names, in order (``k_colsum`` itself counts, its reduction does not)."""
    return [n for n in names if n.startswith(_PRODUCT_PREFIXES) or n == COLSUM]


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    op: str
    N: int
    K: int
    M: int
    route: str
    fwd: tuple
    bwd: tuple
    opts: tuple = ()

    def opt(self, key, default=None):
        return dict(self.opts).get(key, default)

    @property
    def C(self):
        return self.K

    @property
    def grad(self):
        return self.opt("grad", "xhiwb" if self.op == "gru_tail" else "xwb")

    @property
    def bias(self):
        return self.opt("bias", True)

    @property
    def apps(self):
        return self.opt("apps", 1)


CASES = []


def _add(op, N, K, M, route, fwd, bwd, **opts):
    tags = ",".join(f"{k}={v}" for k, v in sorted(opts.items()) if k not in ("lib", "none"))      # (derived from the route)
    c = Case(f"{op}:{N}x{K}->{M}" + (f"[{tags}]" if tags else ""), op, N, K, M, route, tuple(fwd), tuple(bwd), tuple(sorted(opts.items())))
    CASES.append(c)
    return c


def _g(o, default="xwb"):
    return o.get("grad", default)


# ``ops.linear`` ---------------------------------------------------------------------------------------------------------------------------
def _mfma(N, K, M, pad="", op="linear", **o):
    """``_Linear``: forward and ``d_x`` on ``glam_ts_gemm``, ``[d_w | d_b]`` on ``k_wgrad`` — two contiguous tensors for ``Kp + 1 <= 64``
    (``glam_wgrad_gemm_split``), one ``[M + 1, Kp + 1]`` buffer written through transposed strides beyond (``glam_wgrad_gemm``, ones
    column).  ``pad``: ``"/image15"`` = a zero-padded data input on the narrow-weight image, ``"/padded"`` = padded weights."""
    Kp, Mp, g = ceil4(K), ceil4(M), _g(o)
    assert linear_supported(K, M) and (pad == "/image15") == (Kp != K and Mp == M and "x" not in g) and (pad == "/padded") == (
        (Kp != K or Mp != M) and pad != "/image15")
    fwd = [ts_label(Kp, Mp)] if N else []
    bwd = (([ts_label(Mp, Kp)] if "x" in g else []) + [WG]) if (N and g) else []
    return _add(op, N, K, M, f"_Linear[{'split' if Kp + 1 <= 64 else 'ones-column'}]{pad}", fwd, bwd, **o)


def _narrow(N, K, M, **o):
    """``_LinearNarrow``: row dot products, one launch each way (+ its reduction beyond 256 rows)."""
    assert M <= 16 and K >= 64 and K % 4 == 0 and not linear_supported(K, M)
    return _add("linear", N, K, M, "_LinearNarrow", [narrow_label(M)] if N else [], [narrow_label(M, True)] if (N and _g(o)) else [], **o)


def _dense(N, K, M, op="linear", **o):
    """``_LinearDense``: ``glam_linear_dense_fwd_ws`` / ``_bwd_ws``, one launch each way."""
    assert not linear_supported(K, M) and M > 16 and K % 4 == 0 and M % 4 == 0 and K >= 32 and N >= 4
    g = _g(o)
    if not o.get("bias", True):
        g = g.replace("b", "")
    return _add(op, N, K, M, "_LinearDense", [dense_fwd_label(N, K, M)], [dense_bwd_label(N, K, M, g, o.get("bias", True))] if g else [], **o)


def _lib(N, K, M, **o):
    """``_LinearLib``: the products on the GEMM library (bit-equal to ``torch.addmm`` / ``torch.mm``), ``d_b`` on ``glam_colsum`` unless
    ``dy`` sits at a storage offset that is not 16-byte aligned (``dy.sum(0)``)."""
    assert not linear_supported(K, M) and M % 4 == 0 and o.get("bias", True)
    bwd = [COLSUM] if ("b" in _g(o) and not o.get("dy_offset")) else []
    return _add("linear", N, K, M, "_LinearLib", [], bwd, lib="addmm", **o)


def _torch(N, K, M, **o):
    return _add("linear", N, K, M, "F.linear", [], [], lib="F.linear", **o)


ROWS = (1, 15, 16, 17, 63, 64, 65)
for _b in (True, False):
    _mfma(33, 16, 60, bias=_b)          # K + 1 <= 64
    _mfma(33, 60, 180, bias=_b)         # ... on the 192-column variant, d_x over a 180-deep reduction
    _mfma(33, 64, 60, bias=_b)          # K + 1 > 64: the ones column, transposed strides (si = 1, sj = K + 1)
    _mfma(33, 188, 64, bias=_b)
    _narrow(33, 300, 12, bias=_b)
    _dense(33, 200, 80, bias=_b)
    _dense(64, 300, 1024, bias=_b)
_mfma(33, 60, 192)                      # linear_supported: Mp <= 192 at Kp <= 60 ...
_dense(33, 60, 196)
_dense(33, 64, 180)                     # ... Kp <= 60 beyond 64 columns
_mfma(33, 64, 16)                       # (in the MFMA table, so not a narrow head: K >= 64 alone does not make one)
_dense(33, 192, 64)                     # linear_supported: Kp <= 188 at Mp <= 64
_dense(33, 64, 68)                      # ... Mp <= 64 from 64 inputs on
_mfma(33, 32, 20)                       # (in the MFMA table, so not the dense class)
_mfma(33, 15, 60, "/image15", grad="wb")            # atom features 15 -> 16 on the narrow-weight image
_mfma(33, 49, 60, "/image15", grad="wb")            # ... 49 -> 52
_mfma(33, 15, 60, "/padded")                        # a differentiable padded input: padded weights
_mfma(33, 15, 45, "/padded", grad="wb")             # both sides padded: padded weights for a data input too
_mfma(33, 57, 33, "/padded")                        # padded M (and K): the [N, 33] view of [N, 36] rows
_mfma(33, 60, 17, "/padded")
_mfma(33, 60, 20)
_mfma(33, 60, 12)                       # one step outside the narrow head by K
_mfma(33, 60, 16)
_narrow(33, 192, 16)                    # the first K the MFMA table leaves to the narrow head at M <= 16
_mfma(33, 188, 16)
_narrow(33, 300, 16)
_torch(33, 300, 17)                     # one step outside by M: no multiple of 4
_dense(33, 300, 20)
for _m in (1, 2, 4, 8):
    _narrow(33, 1024 if _m == 1 else 300, _m)
_narrow(300, 300, 12)                   # more than 256 rows: row splits + the fixed-order reduction
_dense(33, 32, 200)                     # linear_dense_supported: K >= 32
_lib(33, 28, 200)
_dense(4, 200, 80)                      # ... N >= 4
_lib(3, 200, 80)
_torch(3, 200, 80, bias=False)
_dense(480, 32, 1024)                   # 8 x 16 tiles: k_dense_kc
_lib(33, 450, 1024)
_lib(33, 450, 1024, dy_offset=True)
_torch(33, 450, 1024, bias=False)
_torch(33, 300, 617)
for _n in (0,) + ROWS:
    if _n != 33:
        _mfma(_n, 16, 60)
        _narrow(_n, 300, 12)
for _n in ROWS:
    _mfma(_n, 64, 60)
    if _n >= 4:
        _dense(_n, 200, 80)
# gradient requests: every subset the nodes distinguish (a frozen weight with a trainable bias: "b"; all frozen: "")
for _gr in ("wb", "x", "b", "xb", "w", ""):
    _mfma(33, 16, 60, grad=_gr)
    _mfma(33, 64, 60, grad=_gr)
    _dense(33, 200, 80, grad=_gr)
    _narrow(33, 300, 12, grad=_gr)
for _gr in ("x", "b", "wb", ""):
    _lib(33, 450, 1024, grad=_gr)
# strides: a column slice as the input; a stride-0 cotangent
for _kw in ({"x_slice": True}, {"sum_cot": True}):
    _mfma(33, 16, 60, **_kw)
    _mfma(33, 64, 60, **_kw)
    _narrow(33, 300, 12, **_kw)
    _dense(33, 200, 80, **_kw)
    _lib(33, 450, 1024, **_kw)


# ``ops.linear_relu`` / ``ops.linear_act`` -----------------------------------------------------------------------------------------------
def _relu(N, K, M, pad="", **o):
    """``_Linear`` with the ReLU in the epilogue (``glam_ts_gemm_relu``: the shapes of ``k_tall_x3``); backward: the mask inside the
    weight-gradient product (``glam_wgrad_gemm_split_relu``) when ``x`` needs no gradient, ``Kp + 1 <= 64`` and ``ops.RELU_IN_WGRAD``,
    else an ATen mask launch in front of the plain products."""
    Kp, g = ceil4(K), _g(o)
    assert M % 4 == 0 and linear_supported(K, M) and ts_variant(Kp, M) in (0, 3, 4) and (Kp == K or "x" not in g)
    in_wgrad = "x" not in g and Kp + 1 <= 64 and o.get("knob") is None
    bwd = (([ts_label(M, Kp)] if "x" in g else []) + [WG_RELU if in_wgrad else WG]) if g else []
    route = f"_Linear[relu, {'mask in k_wgrad' if in_wgrad else 'mask launch'}]{pad}"
    return _add("linear_relu", N, K, M, route, [ts_label(Kp, M)], bwd, **o)


def _none(op, N, K, M, **o):
    return _add(op, N, K, M, "None", [], [], none=True, **o)


_relu(33, 16, 60)
_relu(33, 16, 60, grad="wb")
_relu(33, 16, 60, grad="wb", knob="RELU_IN_WGRAD=False")
_relu(33, 15, 60, "/image15", grad="wb")
_relu(33, 60, 64, grad="wb")            # K + 1 <= 64 ...
_relu(33, 64, 60, grad="wb")            # ... and beyond: the mask launch
_relu(33, 60, 64)                       # glam_ts_gemm_relu_supported: M <= 64 at K <= 64 ...
_none("linear_relu", 33, 60, 68)        # ... (the 192-column variant has no ReLU epilogue)
_none("linear_relu", 33, 60, 180)
_none("linear_relu", 33, 57, 33)        # M no multiple of 4
_none("linear_relu", 33, 15, 60)        # a padded differentiable input
_none("linear_relu", 33, 300, 1024)     # the dense class is linear_act's
_relu(33, 16, 60, bias=False, grad="w")
_relu(33, 16, 60, sum_cot=True, grad="wb")
_relu(33, 16, 60, x_slice=True)
for _a in ("none", "relu", "leaky"):
    _dense(33, 200, 80, op="linear_act", act=_a)
    _dense(33, 200, 80, op="linear_act", act=_a, grad="x")
_dense(64, 300, 1024, op="linear_act", act="relu")
_dense(33, 200, 80, op="linear_act", act="leaky", bias=False)
_none("linear_act", 33, 16, 60, act="relu")
_none("linear_act", 33, 300, 12, act="relu")
_none("linear_act", 3, 200, 80, act="relu")


# ``ops.matmul_tall`` --------------------------------------------------------------------------------------------------------------------
def _tall(N, K, M, **o):
    """``_MatmulTall`` (``N >= 64``, K and M multiples of 4).  Forward: ``k_tall_x3`` for ``K <= 320, M <= 64``, the library beyond.
    ``d_a``: ``glam_ts_gemm`` for a layer-sized product (the identity's gradient added in its epilogue) and for ``K > 64, M <= 96``, the
    library beyond.  ``[d_w ; d_b]``: ``k_wgrad`` — ``[a | 1]^T dy`` with a bias in the node (``K + 1 <= 320, M <= 128``), ``a^T dy`` up
    to 128 columns (two 64-column chunks beyond 64), ``dy^T a`` through transposed strides up to ``M = 320``."""
    g, bias, ident = _g(o), o.get("bias", True), o.get("with_identity", False)
    assert N >= 64 and K % 4 == 0 and M % 4 == 0 and ((K <= 320 and M <= 128) or (K <= 128 and M <= 320))
    in_node = bias and K + 1 <= 320 and M <= 128
    x3 = K <= 320 and M <= 64
    fwd = [ts_label(K, M)] if x3 else []
    layer = M <= 64 and K <= 64 and linear_supported(M, K)
    wide = M <= 96 and 64 < K <= 320
    da = "none" if "x" not in g else "layer" if layer else "wide" if wide else "lib"
    bwd = [ts_label(M, K, epi=bool(ident and layer))] if da in ("layer", "wide") else []
    if "w" in g or (in_node and g):
        bwd.append(WG)
    w = "[a | 1]^T dy" if in_node else "a^T dy" if M <= 128 else "dy^T a"
    route = f"_MatmulTall[fwd {'x3' if x3 else 'lib'}; {w}{', chunks' if (M > 64 if M <= 128 else K > 64) else ''}; d_a {da}{' + identity' if ident and 'x' in g else ''}]"
    if not x3:
        o = dict(o, lib="addmm" if in_node else "matmul")
    return _add("matmul_tall", N, K, M, route, fwd, bwd if g else [], **o)


def _rows(N, K, M, **o):
    """``_MatmulTallRows``: fewer than 64 rows or an output width that is no multiple of 4 — the forward kernel on zero-padded columns,
    the gradients plain library products."""
    assert 0 < N and K % 4 == 0 and K <= 320 and M <= 64 and (N < 64 or M % 4)
    return _add("matmul_tall", N, K, M, "_MatmulTallRows", [ts_label(K, ceil4(M))], [], **o)


def _tall_torch(N, K, M, **o):
    return _add("matmul_tall", N, K, M, "torch.matmul", [], [], lib="matmul", **o)


for _b in (True, False):
    _tall(65, 60, 64, bias=_b)          # x3 forward, layer-sized d_a
    _tall(65, 300, 60, bias=_b)         # NNConv's relation product: K <= 320; d_a on the 320-column variant
    _tall(65, 60, 68, bias=_b)          # forward just outside by M
    _tall(65, 60, 128, bias=_b)         # two 64-column chunks
    _tall(65, 60, 132, bias=_b)         # beyond 128 columns: transposed strides (a bias is added outside the node)
    _rows(63, 60, 64, bias=_b)
    _rows(65, 60, 62, bias=_b)          # padded output columns
_tall(64, 60, 64)                       # the 64-row line
_tall(65, 320, 60, bias=False)          # forward K <= 320 ...
_tall_torch(65, 324, 60, bias=False)    # ... and just outside
_tall(65, 316, 60)                      # the bias inside the node: K + 1 <= 320 ...
_tall(65, 320, 60)                      # ... and added outside it
_tall(65, 60, 320, bias=False)          # the transposed-stride route up to M = 320 ...
_tall_torch(65, 60, 324, bias=False)
_tall(65, 128, 132, bias=False)         # ... for K <= 128 (two chunks of a)
_tall_torch(65, 132, 136, bias=False)
_tall(65, 64, 60, bias=False)           # d_a: layer-sized up to K = 64 ...
_tall(65, 68, 60, bias=False)           # ... K > 64 on the 192-column variant
_tall(65, 128, 96, bias=False)          # d_a: M <= 96 ...
_tall(65, 128, 100, bias=False)         # ... the library beyond
for _k, _m in ((48, 60), (128, 96), (128, 100)):
    _tall(65, _k, _m, bias=False, with_identity=True)
_tall(65, 48, 60, with_identity=True, grad="wb")      # (no alias for an input without a gradient)
_rows(63, 320, 60)                      # the bias outside the rows node: K + 1 > 320
_rows(63, 60, 62)
for _n in (1, 15, 16, 17):
    _rows(_n, 60, 64)
_tall_torch(0, 60, 64)
for _gr in ("wb", "x", "b", "w", ""):
    _tall(65, 300, 60, grad=_gr)
    _rows(63, 60, 64, grad=_gr)
_tall(65, 300, 60, bias=False, grad="x")
for _kw in ({"x_slice": True}, {"sum_cot": True}):
    _tall(65, 300, 60, **_kw)
    _rows(63, 60, 64, **_kw)


# ``ops.linear_split`` -------------------------------------------------------------------------------------------------------------------
def _split(N, K, M, M1, **o):
    """``_LinearSplit``: ``x @ wt`` into two column blocks; ``d_x`` from both cotangents as the two K blocks of one product, ``d_wt`` on
    ``k_wgrad`` through transposed strides (``si = 1, sj = M``)."""
    g = _g(o, "xw")
    fwd = [ts_label(K, M)] if N else []
    bwd = (([ts_label(M, K)] if "x" in g else []) + [WG]) if (N and g) else []
    return _add("linear_split", N, K, M, "_LinearSplit", fwd, bwd, M1=M1, **o)


for _gr in ("xw", "w", "x", ""):
    _split(33, 60, 68, 60, grad=_gr)    # the 192-column variant
    _split(33, 48, 56, 48, grad=_gr)    # k_tall_x3
for _n in (0,) + ROWS:
    _split(_n, 60, 68, 60)
_split(33, 60, 68, 60, x_slice=True)
_split(33, 60, 68, 60, sum_cot=True)


# ``ops.gru_tail`` -----------------------------------------------------------------------------------------------------------------------
def _gru_opts(o):
    return o.get("grad", "xhiwb"), o.get("celu_in", False)


def _gru_block(N, C, pad="", **o):
    """``_GruBlock``: the warp-specialised step, one launch each way + both weight gradients in one ``k_wgrad`` launch (the forward
    wrote ``celu(x)``: no CELU fold in it).  ``pad``: odd widths at ``Cp = ceil4(C)`` on gate-wise padded parameters."""
    Cp = ceil4(C)
    assert Cp + 1 <= 64 and 3 * Cp > 64 and 24 <= Cp and (pad == "/padded") == (Cp != C)
    g, _ = _gru_opts(o)
    return _add("gru_tail", N, C, 3 * C, "_GruBlock" + pad, [GB_F], [GB_B, WG] if g else [], **o)


def _gru_wide(N, C, **o):
    """Two ``_LinearTall`` + ``_GruTail`` at ``Cp``: the gate products on ``k_tall_x3`` up to ``Cp = 96`` (the CELU folded into all three
    products of the input's linear), on the library beyond; ``[d_w | d_b]`` on ``glam_wgrad_gemm_linear``.  Backward order: the tail,
    the state's linear (created last), the input's."""
    Cp = ceil4(C)
    g, celu = _gru_opts(o)
    assert N >= 64 and 3 * Cp <= 320 and Cp + 1 <= 128 and Cp != 64
    x3 = Cp <= 96
    fold = celu and x3
    fwd = ([ts_label(Cp, 3 * Cp)] * 2 if x3 else []) + [GT_F]
    bwd = ([GT_B] + ([ts_label(3 * Cp, Cp)] if (x3 and "h" in g) else []) + [WG]
           + ([ts_label(3 * Cp, Cp, epi=fold)] if (x3 and "x" in g) else []) + [WG_CELU if fold else WG])
    return _add("gru_tail", N, C, 3 * C, f"_LinearTall[{'x3' if x3 else 'lib'}{', celu folded' if fold else ''}] x 2 + _GruTail",
                fwd, bwd if g else [], **o)


def _gru_fallback(N, C, lin, **o):
    """``linear`` x 2 + ``_GruTail`` (``lin``: the class of the two linears ``C -> 3 C``)."""
    Cp = ceil4(C)
    g, _ = _gru_opts(o)
    if lin == "_Linear":
        f, b = [ts_label(Cp, 3 * Cp)], lambda code: ([ts_label(3 * Cp, Cp)] if code in g else []) + [WG]
    elif lin == "_LinearDense":
        f, b = [dense_fwd_label(N, C, 3 * C)], lambda code: [dense_bwd_label(N, C, 3 * C, "xwb")]
    else:
        f, b = [], lambda code: []
    return _add("gru_tail", N, C, 3 * C, f"{lin} x 2 + _GruTail", f * 2 + [GT_F], ([GT_B] + b("h") + b("x")) if g else [], **o)


for _celu in (False, True):
    for _id in (False, True):
        for _a in ("none", "relu", "leaky", "celu"):
            _kw = dict(celu_in=_celu, identity=_id, act=_a)
            _gru_block(33, 60, **_kw)
            _gru_block(33, 45, "/padded", **_kw)
            _gru_wide(65, 90, **_kw)
            _gru_fallback(63, 15, "_Linear", **_kw)
            _gru_fallback(63, 90, "F.linear", **_kw)
_kw = dict(celu_in=True, identity=True, act="celu")
for _n in ROWS:
    _gru_block(_n, 60, **_kw)
_gru_block(33, 24, **_kw)               # gru_block_supported: 3 C > 64 ...
_gru_fallback(33, 20, "_Linear", **_kw)
_gru_wide(65, 20, **_kw)                # ... (from 64 rows on the narrow widths take the wide route)
_gru_wide(65, 15, **_kw)
_gru_block(33, 57, "/padded", **_kw)    # C + 1 <= 64 at Cp = 60 ...
_gru_fallback(65, 61, "F.linear", **_kw)      # ... Cp = 64: neither the block (C + 1 > 64) nor _LinearTall (its ones column would be a chunk of its own)
_gru_fallback(65, 64, "_LinearDense", **_kw)
_gru_wide(64, 90, **_kw)                # the wide route from 64 rows on
_gru_wide(65, 96, **_kw)                # _LinearTall: K <= 96 on k_tall_x3 ...
_gru_wide(65, 100, **_kw)               # ... the library beyond
_gru_wide(65, 104, **_kw)               # linear_tall_supported: M = 3 Cp <= 320 ...
_gru_fallback(65, 108, "_LinearDense", **_kw)
for _gr in ("xhi", "wb", ""):
    _gru_block(33, 60, grad=_gr, **_kw)
    _gru_wide(65, 90, grad=_gr, **_kw)
    _gru_fallback(63, 15, "_Linear", grad=_gr, **_kw)
for _x in ({"x_slice": True}, {"sum_cot": True}):
    _gru_block(33, 60, **_kw, **_x)
    _gru_wide(65, 90, **_kw, **_x)
    _gru_fallback(63, 15, "_Linear", **_kw, **_x)

# inside ``ops.weight_scope()``: the same weights applied 1, 2 and 3 times.  From 512 rows on every application but the first parks its
# weight-gradient operands and the first one (its backward runs last) multiplies all sets in ONE launch (``k_wgrad<true, sets>``; one set
# alone runs under the single-set label); below 512 rows each application launches its own product, the carry added in its reduction.
for _n in (512, 511):
    for _apps in (1, 2, 3):
        _park = _n >= 512
        _one = WG_SETS if _apps > 1 else WG
        _add("matmul_tall", _n, 300, 60, "_MatmulTall[scope]", [ts_label(300, 60)] * _apps, [_one] if _park else [WG] * _apps,
             scope=True, apps=_apps, grad="wb")
        _add("gru_tail", _n, 60, 180, "_GruBlock[scope]", [GB_F] * _apps, ([GB_B] * _apps + [_one]) if _park else [GB_B, WG] * _apps,
             scope=True, apps=_apps, **_kw)
        _t, _te = ts_label(276, 92), ts_label(276, 92, epi=True)
        if _park:
            _bw = [GT_B, _t, _te] * (_apps - 1) + [GT_B, _t, _one, _te, WG_SETS if _apps > 1 else WG_CELU]
        else:
            _bw = [GT_B, _t, WG, _te, WG_CELU] * _apps
        _add("gru_tail", _n, 90, 270, "_LinearTall[scope] x 2 + _GruTail", ([ts_label(92, 276)] * 2 + [GT_F]) * _apps, _bw,
             scope=True, apps=_apps, **_kw)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"
assert all(c.K != c.M for c in CASES)


def find(op, N, K, M, **opts):
    """The case of that op and shape whose options are exactly ``opts``."""
    want = tuple(sorted(opts.items()))
    hits = [c for c in CASES if (c.op, c.N, c.K, c.M) == (op, N, K, M) and c.opts == want]
    assert len(hits) == 1, (op, N, K, M, opts, [c.name for c in hits])
    return hits[0]


# ---- the Python predicates, restated: the route of a call ------------------------------------------------------------------------------
def classify(op, N, K, M, bias=True, xgrad=True, with_identity=False, knob=None, scope=False, celu_in=False):
    """The route string the constructors above give a case, from the predicates of ``glam_amd/ops_dense.py`` alone."""
    Kp, Mp = ceil4(K), ceil4(M)
    dense = not linear_supported(K, M) and M > 16 and K % 4 == 0 and M % 4 == 0 and K >= 32 and N >= 4
    if op == "linear":
        if M <= 16 and K >= 64 and K % 4 == 0 and not linear_supported(K, M):
            return "_LinearNarrow"
        if dense:
            return "_LinearDense"
        if not linear_supported(K, M):
            return "_LinearLib" if (bias and M % 4 == 0) else "F.linear"
        pad = "/image15" if (Kp != K and Mp == M and not xgrad) else "/padded" if (Kp != K or Mp != M) else ""
        return f"_Linear[{'split' if Kp + 1 <= 64 else 'ones-column'}]{pad}"
    if op == "linear_relu":
        if not (M % 4 == 0 and linear_supported(K, M) and ts_variant(Kp, M) in (0, 3, 4)) or (Kp != K and xgrad):
            return "None"
        in_wgrad = knob is None and not xgrad and Kp + 1 <= 64
        return f"_Linear[relu, {'mask in k_wgrad' if in_wgrad else 'mask launch'}]{'/image15' if Kp != K else ''}"
    if op == "linear_act":
        return "_LinearDense" if dense else "None"
    if op == "linear_split":
        return "_LinearSplit"
    if op == "matmul_tall":
        ok = K % 4 == 0 and M % 4 == 0 and N >= 64
        if ok and ((K <= 320 and M <= 128) or (K <= 128 and M <= 320)):
            if scope:
                return "_MatmulTall[scope]"
            in_node = bias and K + 1 <= 320 and M <= 128
            x3 = K <= 320 and M <= 64
            layer = M <= 64 and K <= 64 and linear_supported(M, K)
            da = "none" if not xgrad else "layer" if layer else "wide" if (M <= 96 and 64 < K <= 320) else "lib"
            w = "[a | 1]^T dy" if in_node else "a^T dy" if M <= 128 else "dy^T a"
            return (f"_MatmulTall[fwd {'x3' if x3 else 'lib'}; {w}{', chunks' if (M > 64 if M <= 128 else K > 64) else ''}; "
                    f"d_a {da}{' + identity' if with_identity and xgrad else ''}]")
        if N > 0 and K % 4 == 0 and K <= 320 and M <= 64 and (N < 64 or M % 4):
            return "_MatmulTallRows"
        return "torch.matmul"
    assert op == "gru_tail" and M == 3 * K
    C, Cp = K, ceil4(K)
    if C % 4 == 0 and C + 1 <= 64 and linear_supported(C, 3 * C) and 3 * C > 64:
        return "_GruBlock" + ("[scope]" if scope else "")
    if Cp != C and linear_supported(Cp, 3 * Cp) and 3 * Cp > 64 and Cp + 1 <= 64:
        return "_GruBlock/padded"
    if 3 * Cp <= 320 and Cp + 1 <= 128 and Cp != 64 and N >= 64:
        if scope:
            return "_LinearTall[scope] x 2 + _GruTail"
        return f"_LinearTall[{'x3' if Cp <= 96 else 'lib'}{', celu folded' if celu_in and Cp <= 96 else ''}] x 2 + _GruTail"
    return classify("linear", N, C, 3 * C).split("[")[0] + " x 2 + _GruTail"


def classify_case(c):
    return classify(c.op, c.N, c.K, c.M, bias=c.bias, xgrad="x" in c.grad, with_identity=c.opt("with_identity", False), knob=c.opt("knob"),
                    scope=c.opt("scope", False), celu_in=c.opt("celu_in", False))


ROUTES = ["_Linear[split]", "_Linear[ones-column]", "_Linear[split]/image15", "_Linear[split]/padded", "_LinearNarrow", "_LinearDense",
          "_LinearLib", "F.linear", "_Linear[relu, mask in k_wgrad]", "_Linear[relu, mask launch]", "_Linear[relu, mask in k_wgrad]/image15",
          "None", "_MatmulTall[fwd x3; [a | 1]^T dy; d_a layer]", "_MatmulTall[fwd x3; a^T dy; d_a layer + identity]",
          "_MatmulTall[fwd x3; [a | 1]^T dy; d_a wide]", "_MatmulTall[fwd lib; a^T dy, chunks; d_a wide + identity]",
          "_MatmulTall[fwd lib; a^T dy, chunks; d_a lib + identity]", "_MatmulTall[fwd lib; [a | 1]^T dy, chunks; d_a lib]",
          "_MatmulTall[fwd lib; a^T dy, chunks; d_a lib]", "_MatmulTall[fwd lib; a^T dy, chunks; d_a wide]",
          "_MatmulTall[fwd x3; [a | 1]^T dy; d_a none]", "_MatmulTall[fwd x3; a^T dy; d_a layer]", "_MatmulTall[fwd x3; a^T dy; d_a wide]",
          "_MatmulTall[fwd lib; dy^T a; d_a lib]", "_MatmulTall[fwd lib; dy^T a, chunks; d_a lib]", "_MatmulTallRows", "torch.matmul",
          "_LinearSplit", "_GruBlock", "_GruBlock/padded", "_LinearTall[x3, celu folded] x 2 + _GruTail", "_LinearTall[x3] x 2 + _GruTail",
          "_LinearTall[lib] x 2 + _GruTail", "_Linear x 2 + _GruTail", "F.linear x 2 + _GruTail", "_LinearDense x 2 + _GruTail",
          "_MatmulTall[scope]", "_GruBlock[scope]", "_LinearTall[scope] x 2 + _GruTail"]

# ---- every route-deciding boundary: (predicate, op, the dimension it moves, last value inside, first value outside in steps the op
# accepts, the other dimensions and options of the two cases) ------------------------------------------------------------------------------
THRESHOLDS = [
    ("linear_supported: Kp <= 60 beyond 64 columns", "linear", "K", 60, 64, dict(N=33, M=180)),
    ("linear_supported: Mp <= 192 at Kp <= 60", "linear", "M", 192, 196, dict(N=33, K=60)),
    ("linear_supported: Kp <= 188 at Mp <= 64", "linear", "K", 188, 192, dict(N=33, M=64)),
    ("linear_supported: Mp <= 64 beyond 60 inputs", "linear", "M", 60, 68, dict(N=33, K=64)),
    ("_Linear: K + 1 <= 64 (split outputs | ones column)", "linear", "K", 60, 64, dict(N=33, M=16)),
    ("narrow head: M <= 16", "linear", "M", 16, 17, dict(N=33, K=300)),
    ("narrow head: M <= 16 (next multiple of 4)", "linear", "M", 16, 20, dict(N=33, K=300)),
    ("narrow head: K >= 64 outside the MFMA table", "linear", "K", 192, 188, dict(N=33, M=16)),
    ("narrow head: K >= 64", "linear", "K", 300, 60, dict(N=33, M=12)),
    ("dense class: M > 16", "linear", "M", 20, 16, dict(N=33, K=300)),
    ("dense class: K >= 32", "linear", "K", 32, 28, dict(N=33, M=200)),
    ("dense class: N >= 4", "linear", "N", 4, 3, dict(K=200, M=80)),
    ("linear_relu: M <= 64 (glam_ts_gemm_relu_supported)", "linear_relu", "M", 64, 68, dict(N=33, K=60)),
    ("linear_relu: mask inside k_wgrad for K + 1 <= 64", "linear_relu", "K", 16, 64, dict(N=33, M=60, grad="wb")),
    ("matmul_tall: the 64-row line", "matmul_tall", "N", 64, 63, dict(K=60, M=64)),
    ("_MatmulTall forward: K <= 320", "matmul_tall", "K", 320, 324, dict(N=65, M=60, bias=False)),
    ("_MatmulTall forward: M <= 64", "matmul_tall", "M", 64, 68, dict(N=65, K=60)),
    ("matmul_tall bias route: K + 1 <= 320", "matmul_tall", "K", 316, 320, dict(N=65, M=60)),
    ("matmul_tall: M <= 128", "matmul_tall", "M", 128, 132, dict(N=65, K=60)),
    ("matmul_tall: transposed strides up to M = 320", "matmul_tall", "M", 320, 324, dict(N=65, K=60, bias=False)),
    ("matmul_tall: K <= 128 beyond 128 columns", "matmul_tall", "K", 128, 132, dict(N=65, bias=False)),
    ("_MatmulTall d_a: layer-sized up to K = 64", "matmul_tall", "K", 64, 68, dict(N=65, M=60, bias=False)),
    ("_MatmulTall d_a: M <= 96 for K > 64", "matmul_tall", "M", 96, 100, dict(N=65, K=128, bias=False)),
    ("gru_block_supported: C + 1 <= 64", "gru_tail", "K", 60, 64, dict()),
    ("gru_block_supported: 3 C > 64", "gru_tail", "K", 24, 20, dict(N=33)),
    ("_gru_padded_supported: Cp + 1 <= 64", "gru_tail", "K", 57, 61, dict()),
    ("gru_tail wide route: N >= 64", "gru_tail", "N", 64, 63, dict(K=90)),
    ("_LinearTall: K <= 96 on k_tall_x3", "gru_tail", "K", 96, 100, dict(N=65)),
    ("linear_tall_supported: M <= 320", "gru_tail", "K", 104, 108, dict(N=65)),
    ("parking: 512 rows inside a weight_scope", "matmul_tall", "N", 512, 511, dict(scope=True)),
    ("parking: 512 rows inside a weight_scope (GRU block)", "gru_tail", "N", 512, 511, dict(scope=True, K=60)),
    ("parking: 512 rows inside a weight_scope (_LinearTall)", "gru_tail", "N", 512, 511, dict(scope=True, K=90)),
]


def threshold_cases(entry, value):
    """The cases at ``value`` of the entry's dimension that match its fixed dimensions and options."""
    _, op, dim, _, _, fixed = entry
    out = []
    for c in CASES:
        if c.op != op or getattr(c, dim) != value:
            continue
        if all((getattr(c, k) if k in ("N", "K", "M") else c.opt(k, {"bias": True}.get(k))) == v for k, v in fixed.items()):
            out.append(c)
    return out


# ---- the (K, M) products of the reference's search space (src_1gp/glam.py:60: hid_dim = 15 a) --------------------------------------------
HID = [15 * a for a in (1, 2, 3, 4, 6)]
E_DIMS = [256, 512, 1024, 2048]
SEARCH_SHAPES = ([("gru_tail", C, 3 * C) for C in HID]                                                   # GRU C -> 3 C
                 + [("linear", 5 * C, e) for C in HID for e in E_DIMS]                                    # readout 5 C -> e_dim
                 + [("matmul_tall", De * C, C) for C in HID for De in (4, 8)]                             # NNConv De C -> C
                 + [("linear", k, C) for C in HID for k in (15, 49)]                                      # embeddings
                 + [("linear", e, m) for e in E_DIMS for m in (1, 2, 12, 617)])                           # heads


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
XOFF = 3        # x_slice: the op's input is the column slice ``leaf[:, 3:]`` of a wider leaf (non-contiguous, not 16-byte aligned)

LEAVES = {"linear": ("x", "w", "b"), "linear_relu": ("x", "w", "b"), "linear_act": ("x", "w", "b"), "matmul_tall": ("x", "w", "b"),
          "linear_split": ("x", "w"), "gru_tail": ("x", "h", "i", "w_ih", "w_hh", "b_ih", "b_hh")}
_CODE = {"x": "x", "h": "h", "i": "i", "w": "w", "b": "b", "w_ih": "w", "w_hh": "w", "b_ih": "b", "b_hh": "b"}


def leaf_names(c):
    """The leaves of the case in order: ``x`` once per application (``x``, ``x2``, ``x3``), no bias / identity where the case has none."""
    names = []
    for n in LEAVES[c.op]:
        if (n == "b" and not c.bias) or (n == "i" and not c.opt("identity", False)):
            continue
        names.append(n)
        if n == "x":
            names += [f"x{k}" for k in range(2, c.apps + 1)]
    return names


def requires_grad(c, name):
    return _CODE[name.rstrip("23")] in c.grad


@functools.lru_cache(maxsize=None)
def inputs(name):
    """``(leaves, cots)``: fp32 CPU tensors of the case, seeded by its name.  ``cots[k]``: the cotangents of application k's outputs.
    Unit-normal rows, weights scaled by ``1 / sqrt(fan-in)``, biases by 0.1.  Shared: do not modify."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    N, K, M = c.N, c.K, c.M
    rn = lambda *s: torch.randn(*s, generator=g)
    wide = K + (XOFF if c.opt("x_slice") else 0)
    t = {}
    for n in leaf_names(c):
        base = n.rstrip("23")
        if base == "x":
            t[n] = rn(N, wide)
        elif base in ("h", "i"):
            t[n] = rn(N, K)
        elif base == "w":
            t[n] = rn(K, M) / K ** 0.5 if c.op in ("matmul_tall", "linear_split") else rn(M, K) / K ** 0.5
        elif base in ("w_ih", "w_hh"):
            t[n] = rn(M, K) / K ** 0.5
        else:
            t[n] = 0.1 * rn(M)
    cots = []
    for _ in range(c.apps):
        if c.op == "gru_tail":
            cots.append([rn(N, K), rn(N, K)])
        elif c.op == "linear_split":
            cots.append([rn(N, c.opt("M1")), rn(N, M - c.opt("M1"))])
        elif c.op == "matmul_tall" and c.opt("with_identity"):
            cots.append([rn(N, M), rn(N, K)])
        else:
            cots.append([rn(N, M)])
    if c.opt("sum_cot"):
        cots[0][0] = torch.ones(cots[0][0].shape)
    return t, cots


def op_input(c, leaf):
    return leaf[:, XOFF:] if c.opt("x_slice") else leaf


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
_ACT = {"none": lambda v, s: v, "relu": lambda v, s: torch.relu(v), "leaky": lambda v, s: F.leaky_relu(v, s), "celu": lambda v, s: F.celu(v)}
SLOPE = {"leaky": 0.1}


def slope(c):
    return SLOPE.get(c.opt("act", "none"), 0.0)


def forward(c, t):
    """The op in plain torch on the leaves ``t`` (any dtype): a list of applications, each the list of its outputs."""
    xs = [op_input(c, t[n]) for n in leaf_names(c) if n.rstrip("23") == "x"]
    b = t.get("b")
    if c.op == "linear":
        return [[F.linear(x, t["w"], b)] for x in xs]
    if c.op == "linear_relu":
        return [[torch.relu(F.linear(x, t["w"], b))] for x in xs]
    if c.op == "linear_act":
        return [[_ACT[c.opt("act")](F.linear(x, t["w"], b), slope(c))] for x in xs]
    if c.op == "matmul_tall":
        outs = []
        for x in xs:
            y = x @ t["w"]
            y = y if b is None else y + b
            outs.append([y, x * 1] if c.opt("with_identity") else [y])
        return outs
    if c.op == "linear_split":
        M1 = c.opt("M1")
        return [[(x @ t["w"])[:, :M1], (x @ t["w"])[:, M1:]] for x in xs]
    outs, h = [], t["h"]
    for x in xs:      # the block's applications: the state handed on
        h = O.gru_step(F.celu(x) if c.opt("celu_in") else x, h, t["w_ih"], t["w_hh"], t["b_ih"], t["b_hh"])
        y = h + t["i"] if c.opt("identity") else h
        outs.append([_ACT[c.opt("act", "none")](y, slope(c)), h])
    return outs


def typed_leaves(c, dtype):
    t, cots = inputs(c.name)
    return ({n: v.to(dtype).requires_grad_(requires_grad(c, n)) for n, v in t.items()}, [[ct.to(dtype) for ct in app] for app in cots])


def run(c, dtype, fwd=forward):
    """``(outs, grads)`` of the restatement with autograd on the CPU: ``outs`` flat over applications and outputs, ``grads`` in
    ``leaf_names`` order (None where the request excludes the leaf)."""
    t, cots = typed_leaves(c, dtype)
    outs = [o for app in fwd(c, t) for o in app]
    flat_cots = [ct for app in cots for ct in app]
    names = leaf_names(c)
    req = [n for n in names if t[n].requires_grad]
    live = [(o, ct) for o, ct in zip(outs, flat_cots) if o.requires_grad]      # (an identity handed back for a frozen input has no history)
    got = {}
    if req and live:
        got = dict(zip(req, torch.autograd.grad([o for o, _ in live], [t[n] for n in req], grad_outputs=[ct for _, ct in live], allow_unused=True)))
    return [o.detach() for o in outs], [got.get(n) for n in names]


@functools.lru_cache(maxsize=None)
def reference(name):
    """``{fp64: (outs, grads), fp32: (outs, grads)}`` of the case, computed once and shared (do not modify)."""
    return {dt: run(BY_NAME[name], dt) for dt in (torch.float64, torch.float32)}


def twin(name, k):
    """``run(dtype) -> (out, [grads])`` in the form ``assert_twin_parity`` takes: output k of the case, the gradients with output 0."""
    ref = reference(name)
    return lambda dt: (ref[dt][0][k], ref[dt][1] if k == 0 else [])
