"""CPU: the cases and the restatements of tests/dense_cases.py, which tests/test_gpu_dense_ops.py holds the dense operators against.
Established here, without a GPU:

* every route-deciding boundary has a case at its last value inside and one at its first value outside, and the two differ in route or
  in launches; every product of the reference's search space falls into the class of some case; every route has a case;
* the route written into each case is the one the predicates of ``glam_amd/ops_dense.py`` give (restated in ``classify``, whose shape
  predicates are held against the package's own);
* each restatement in fp64 equals the obvious torch expression (explicit products, ``torch.nn.GRU``) to 1e-12, and in fp32 it passes
  the bound against its own fp64 twin;
* the cases discriminate: ten wrong operators, written as mutations of the hand-derived backward and evaluated in fp32, each fail the very
  bound the GPU tests apply (``assert_fp32_parity``, k = 8) on a named case — and the unmutated derivation passes it there."""
import pytest
import torch
import torch.nn.functional as F

from glam_amd import ops_dense
from tests import dense_cases as C
from tests.conftest import assert_fp32_parity, assert_twin_parity

F64, F32 = torch.float64, torch.float32


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", C.THRESHOLDS, ids=[e[0] for e in C.THRESHOLDS])
def test_threshold_has_a_case_on_each_side(entry):
    inside, outside = C.threshold_cases(entry, entry[3]), C.threshold_cases(entry, entry[4])
    assert inside and outside, (len(inside), len(outside))
    # the boundary decides something: some pair across it differs in its route or in its launches
    assert any((a.route, a.fwd, a.bwd) != (b.route, b.fwd, b.bwd) for a in inside for b in outside)


def test_search_space_shapes_fall_into_a_case_class():
    routes = {c.route for c in C.CASES}
    for op, K, M in C.SEARCH_SHAPES:
        data_input = op == "linear" and K in (15, 49)          # atom / residue features: no gradient
        for N in (20, 1024):                                    # a batch of one molecule and the benchmark's
            assert C.classify(op, N, K, M, xgrad=not data_input) in routes, (op, N, K, M)


def test_every_route_has_a_case():
    routes = {c.route for c in C.CASES}
    assert set(C.ROUTES) == routes, (sorted(set(C.ROUTES) - routes), sorted(routes - set(C.ROUTES)))


def test_case_routes_follow_the_predicates():
    for c in C.CASES:
        assert C.classify_case(c) == c.route, c.name
        assert (not c.fwd and not c.bwd) or c.route != "None"
        if not c.grad or c.opt("none"):
            assert c.bwd == (), c.name


def test_restated_predicates_are_the_package_s():
    z = torch.zeros(1)
    for K in range(1, 400):
        for M in (1, 2, 12, 16, 17, 20, 33, 45, 60, 64, 68, 96, 128, 180, 192, 196, 276, 288, 320, 324, 1024):
            assert C.linear_supported(K, M) == ops_dense.linear_supported(K, M), (K, M)
            mine = C.classify("linear_act", 64, K, M) == "_LinearDense"
            theirs = (not ops_dense.linear_supported(K, M)) and M > 16 and ops_dense.linear_dense_supported(64, K, M)
            assert mine == theirs, (K, M)
    for Cw in range(1, 140):
        w = torch.empty(3 * Cw, Cw)
        route = C.classify("gru_tail", 1024, Cw, 3 * Cw)
        assert (route == "_GruBlock") == bool(ops_dense.gru_block_supported(Cw, w, z, z)), Cw
        assert (route == "_GruBlock/padded") == bool(ops_dense._gru_padded_supported(Cw, w, z, z) and not ops_dense.gru_block_supported(Cw, w, z, z)), Cw
        Cp = C.ceil4(Cw)
        assert route.startswith("_LinearTall") == (not route.startswith("_GruBlock") and ops_dense.linear_tall_supported(Cp, 3 * Cp)), Cw


def test_label_tables():
    """The label helpers on the shapes DESIGN §4.4 names for each kernel class."""
    assert C.ts_label(180, 60) == "k_tall_x3<6, 4, 1>" and C.ts_label(276, 92) == "k_tall_x3<9, 6, 1>"
    assert C.ts_label(92, 276) == "k_tall_x3<3, 4, 5>" and C.ts_label(300, 60) == "k_tall_x3<10, 4, 1>"
    assert C.ts_label(60, 180) == "k_ts_gemm<12, 4, 4>" and C.ts_label(16, 60) == "k_tall_x3<2, 4, 1>"
    assert C.ts_label(60, 60, epi=True) == "k_tall_x3<2, 4, 1, epi>" and C.ts_label(60, 300, epi=True) == "k_ts_gemm<20, 6, 4>"
    assert C.dense_fwd_label(1024, 300, 1024) == "k_dense_kc" and C.dense_fwd_label(64, 300, 1024) == "k_dense_x3<32>"
    assert C.dense_bwd_label(1024, 300, 1024, "xwb") == "k_dense_x3<64>"
    assert C.product_labels(["k_ts_make_image", "k_tall_x3<2, 4, 1>", "k_final_reduce", "k_wgrad<false>", "k_colsum", "k_colsum_reduce",
                             "k_pad_group<true>", "k_gru_ws_pre"]) == ["k_tall_x3<2, 4, 1>", "k_wgrad<false>", "k_colsum"]


# ---------------------------------------------------------------------------------------------
# the restatement against the obvious expression
# ---------------------------------------------------------------------------------------------
def _act_grad(c, pre):
    act = "relu" if c.op == "linear_relu" else c.opt("act", "none") if c.op == "linear_act" else "none"
    if act == "relu":
        return torch.relu(pre), (pre > 0).to(pre.dtype)
    if act == "leaky":
        return torch.where(pre > 0, pre, pre * C.slope(c)), torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, C.slope(c)))
    return pre, torch.ones_like(pre)


def _widen(c, dx):
    """The gradient of the leaf behind a column slice: zero in the columns the op never saw."""
    return F.pad(dx, (C.XOFF, 0)) if c.opt("x_slice") else dx


def obvious(c, dtype=F64):
    """``(outs, grads)`` like ``dense_cases.run``, from explicit products (``gru_tail``: ``torch.nn.GRU`` under autograd)."""
    t, cots = C.inputs(c.name)
    t = {n: v.to(dtype) for n, v in t.items()}
    cots = [[ct.to(dtype) for ct in app] for app in cots]
    names = C.leaf_names(c)
    xs = [n for n in names if n.rstrip("23") == "x"]
    g = {n: None for n in names}
    outs = []
    acc = lambda n, v: g.__setitem__(n, v if g[n] is None else g[n] + v)
    if c.op in ("linear", "linear_relu", "linear_act"):
        x, w, b = C.op_input(c, t["x"]), t["w"], t.get("b")
        pre = x @ w.t() + (0 if b is None else b)
        y, dact = _act_grad(c, pre)
        dpre = cots[0][0] * dact
        outs, g["x"], g["w"] = [y], _widen(c, dpre @ w), dpre.t() @ x
        if b is not None:
            g["b"] = dpre.sum(0)
    elif c.op == "matmul_tall":
        for n, ct in zip(xs, cots):
            x = C.op_input(c, t[n])
            y = x @ t["w"] + (0 if "b" not in t else t["b"])
            outs.append(y)
            da = ct[0] @ t["w"].t()
            if c.opt("with_identity"):
                outs.append(x.clone())
                da = da + ct[1]
            acc(n, _widen(c, da))
            acc("w", x.t() @ ct[0])
            if "b" in t:
                acc("b", ct[0].sum(0))
    elif c.op == "linear_split":
        x, M1 = C.op_input(c, t["x"]), c.opt("M1")
        y, dy = x @ t["w"], torch.cat(cots[0], 1)
        outs, g["x"], g["w"] = [y[:, :M1], y[:, M1:]], _widen(c, dy @ t["w"].t()), x.t() @ dy
    else:
        gru = torch.nn.GRU(c.C, c.C).to(dtype)
        gru.load_state_dict({"weight_ih_l0": t["w_ih"], "weight_hh_l0": t["w_hh"], "bias_ih_l0": t["b_ih"], "bias_hh_l0": t["b_hh"]})
        leaf = {n: t[n].clone().requires_grad_(True) for n in names if n[0] in "xhi"}
        leaf.update(w_ih=gru.weight_ih_l0, w_hh=gru.weight_hh_l0, b_ih=gru.bias_ih_l0, b_hh=gru.bias_hh_l0)
        h = leaf["h"]
        fn = {"none": lambda v: v, "relu": torch.relu, "leaky": lambda v: F.leaky_relu(v, C.slope(c)), "celu": torch.celu}[c.opt("act", "none")]
        for n in xs:
            x = C.op_input(c, leaf[n])
            y, _ = gru((torch.celu(x) if c.opt("celu_in") else x).unsqueeze(0), h.unsqueeze(0))
            h = y.squeeze(0)
            outs += [fn(h + leaf["i"] if c.opt("identity") else h), h]
        gs = torch.autograd.grad(outs, [leaf[n] for n in names], grad_outputs=[ct for app in cots for ct in app], allow_unused=True)
        g = dict(zip(names, gs))
        outs = [o.detach() for o in outs]
    return outs, [g[n] if C.requires_grad(c, n) else None for n in names]


def _close(a, b, tol, what):
    assert a.shape == b.shape, what
    if a.numel():
        assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), what


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_restatement(name):
    """fp64: the restatement is the obvious expression (1e-12); fp32: it stays inside the bound its own fp64 twin sets (k = 8, forward
    1e-5) — the reference alone passes the check the kernels are held to."""
    c = C.BY_NAME[name]
    ref = C.reference(name)
    outs, grads = obvious(c)
    r_outs, r_grads = ref[F64]
    assert len(outs) == len(r_outs) and len(grads) == len(r_grads) == len(C.leaf_names(c))
    for k, (a, b) in enumerate(zip(r_outs, outs)):
        _close(a, b, 1e-12, f"{name} out[{k}]")
    for n, a, b in zip(C.leaf_names(c), r_grads, grads):
        assert (a is None) == (not C.requires_grad(c, n)), (name, n)
        if a is not None:
            _close(a, b, 1e-12, f"{name} grad.{n}")
    o32, g32 = ref[F32]
    for k in range(len(o32)):
        assert_twin_parity(C.twin(name, k), o32[k], g32 if k == 0 else [], f"{name}[{k}]", C.leaf_names(c))


# ---------------------------------------------------------------------------------------------
# the cases discriminate
# ---------------------------------------------------------------------------------------------
def _f32(name):
    c = C.BY_NAME[name]
    t, cots = C.inputs(name)
    return c, t, cots


def _grad_ref(name, leaf):
    ref, k = C.reference(name), C.leaf_names(C.BY_NAME[name]).index(leaf)
    return ref[F64][1][k], ref[F32][1][k]


def _bias_column(wrong):
    """``[d_w | d_b]`` in one ``[M, K + 1]`` buffer (``_Linear`` beyond 63 inputs): the bias gradient is column K — not K - 1."""
    name = "linear:33x64->60[bias=True]"
    c, t, cots = _f32(name)
    dy = cots[0][0]
    dwb = torch.cat([dy.t() @ t["x"], dy.sum(0)[:, None]], 1)
    return name, "b", dwb[:, c.K - 1 if wrong else c.K]


def _dw_transposed(wrong):
    """``out[k, m]`` written at ``dwb[m, k]`` (``si = 1, sj = K + 1``) — not at ``dwb[k, m]`` of the same buffer."""
    name = "linear:33x64->60[bias=True]"
    c, t, cots = _f32(name)
    out_km = t["x"].t() @ cots[0][0]                     # the product as the kernel forms it: [K, M]
    buf = torch.empty(c.M * c.K)
    si, sj = (c.M, 1) if wrong else (1, c.K)
    torch.as_strided(buf, (c.K, c.M), (si, sj)).copy_(out_km)
    return name, "w", buf.view(c.M, c.K)


def _pad_column(wrong):
    """A 15 -> 16 padded product: the 16th column is zero on both sides — not a one in the input beside whatever follows the weight's
    row in memory."""
    name = "linear:33x15->60[grad=wb]"
    c, t, cots = _f32(name)
    x_p, w_p = F.pad(t["x"], (0, 1)), F.pad(t["w"], (0, 1))
    if wrong:
        x_p[:, 15] = 1.0
        w_p[:-1, 15] = t["w"][1:, 0]
    return name, None, x_p @ w_p.t() + t["b"]


def _carry(mode):
    """Three applications of one weight inside a scope: the carry hands the later applications' gradients on once — not twice, not never."""
    name = "matmul_tall:511x300->60[apps=3,grad=wb,scope=True]"
    c, t, cots = _f32(name)
    g = [t[n].t() @ ct[0] for n, ct in zip(("x", "x2", "x3"), cots)]
    total = g[2]                                         # the last application's backward runs first
    for k in (1, 0):
        total = g[k] + (total if mode != "dropped" else 0) + (g[2] if (mode == "twice" and k == 1) else 0)
    return name, "w", total


def _tail_rows(wrong):
    """The weight gradient sums ALL rows — not the whole 16-row tiles only."""
    name = "linear:17x16->60"
    c, t, cots = _f32(name)
    n = c.N - c.N % 16 if wrong else c.N
    return name, "w", cots[0][0][:n].t() @ t["x"][:n]


def _celu_point(wrong):
    """The folded CELU's derivative is taken at ``x`` — not at ``celu(x)``, which the forward also keeps."""
    name = "gru_tail:65x90->270[act=celu,celu_in=True,identity=True]"
    c, t, cots = _f32(name)
    xc = F.celu(t["x"]).requires_grad_(True)
    h = C.O.gru_step(xc, t["h"], t["w_ih"], t["w_hh"], t["b_ih"], t["b_hh"])
    (d_xc,) = torch.autograd.grad([F.celu(h + t["i"]), h], [xc], grad_outputs=cots[0])
    v = F.celu(t["x"]) if wrong else t["x"]
    return name, "x", d_xc * torch.where(v > 0, torch.ones_like(v), torch.exp(v))


def _relu_mask(wrong):
    """The ReLU's backward masks ``dy`` by the sign of the saved OUTPUT — not by its own."""
    name = "linear_relu:33x16->60[grad=wb]"
    c, t, cots = _f32(name)
    dy = cots[0][0]
    y = torch.relu(t["x"] @ t["w"].t() + t["b"])
    return name, "w", (dy * ((dy if wrong else y) > 0)).t() @ t["x"]


def _identity_grad(wrong):
    """``with_identity``: the gradient of the handed-back input joins ``dy @ w^T`` — it is not lost."""
    name = "matmul_tall:65x48->60[bias=False,with_identity=True]"
    c, t, cots = _f32(name)
    da = cots[0][0] @ t["w"].t()
    return name, "x", da if wrong else da + cots[0][1]


def _second_chunk(wrong):
    """``64 < M <= 128``: both 64-column chunks of ``dy`` are multiplied — not the first alone."""
    name = "matmul_tall:65x60->128[bias=False]"
    c, t, cots = _f32(name)
    dw = t["x"].t() @ cots[0][0]
    if wrong:
        dw[:, 64:] = 0.0
    return name, "w", dw


MUTATIONS = {
    "bias gradient from the wrong column of [d_w | d_b]": (_bias_column, True),
    "d_w written transposed": (_dw_transposed, True),
    "16th column of a 15 -> 16 product not zero": (_pad_column, True),
    "carry added twice": (_carry, "twice"),
    "carry dropped": (_carry, "dropped"),
    "last N % 16 rows left out of the weight gradient": (_tail_rows, True),
    "celu' taken at celu(x)": (_celu_point, True),
    "ReLU mask from dy's sign": (_relu_mask, True),
    "with_identity's gradient dropped": (_identity_grad, True),
    "second 64-column chunk left out": (_second_chunk, True),
}


def _hold(name, leaf, got, what):
    if leaf is None:
        r64, r32 = C.reference(name)[F64][0][0], C.reference(name)[F32][0][0]
        return assert_fp32_parity(got, r64, r32, what, k=8.0, out_tol=1e-5)
    return assert_fp32_parity(got, *_grad_ref(name, leaf), what, k=8.0)


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_mutation_fails_the_bound(mutation):
    fn, wrong = MUTATIONS[mutation]
    name, leaf, got = fn(False)
    _hold(name, leaf, got, f"{mutation} (unmutated) on {name}")            # the derivation itself is right ...
    name, leaf, got = fn(wrong)
    with pytest.raises(AssertionError, match="max\\|d\\|"):                    # ... and the mutation is seen, by the bound (not by a shape)
        _hold(name, leaf, got, f"{mutation} on {name}")
