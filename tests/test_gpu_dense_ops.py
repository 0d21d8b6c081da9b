"""GPU (MI355X): every autograd route of the dense operators (``glam_amd/ops_dense.py``: ``linear``, ``linear_relu``, ``linear_act``,
``matmul_tall``, ``linear_split``, ``gru_tail``) on the cases of tests/dense_cases.py — one on each side of every shape predicate that
picks a node or a kernel, every gradient request the nodes distinguish, column-slice inputs, stride-0 cotangents, shared weights inside
a ``weight_scope``.  tests/test_dense_cases_host.py shows on the CPU that ten subtly wrong operators fail this very bound on these cases.

Every case runs twice from fresh leaves under ``_lib.kernel_timer()`` and must
* give the same bits both times (every sum of the kernels runs in a fixed order),
* make exactly the product launches the case expects, in order (skipped when the 3 x bf16 route is switched off: the labels are the
  default mode's); a library route makes none and equals the torch expression it names bit for bit,
* sit inside the fp64-twin bound of the case's plain torch restatement (``assert_twin_parity``, k = 8, forward 1e-5), padded views on
  their real columns, the pad columns exactly zero,
* return ``None`` — not a zero fill — for every gradient the request excludes."""
import pytest
import torch
import torch.nn.functional as F

from glam_amd import _lib, ops
from tests import dense_cases as C
from tests.conftest import assert_fp32_parity, assert_twin_parity

pytestmark = pytest.mark.gpu


def _apply(c, t):
    """The op on the device leaves ``t``: a list of applications, each the list of its outputs; None where the op declines."""
    xs = [C.op_input(c, t[n]) for n in C.leaf_names(c) if n.rstrip("23") == "x"]
    b = t.get("b")
    outs = []
    for x in xs:
        if c.op == "linear":
            r = ops.linear(x, t["w"], b)
        elif c.op == "linear_relu":
            r = ops.linear_relu(x, t["w"], b)
        elif c.op == "linear_act":
            r = ops.linear_act(x, t["w"], b, c.opt("act"), C.slope(c))
        elif c.op == "matmul_tall":
            r = ops.matmul_tall(x, t["w"], b, with_identity=c.opt("with_identity", False))
        elif c.op == "linear_split":
            r = ops.linear_split(x, t["w"], c.opt("M1"))
        else:
            r = ops.gru_tail(x, t["h"] if not outs else outs[-1][1], t.get("i"), t["w_ih"], t["w_hh"], t["b_ih"], t["b_hh"],
                             act=c.opt("act", "none"), slope=C.slope(c), celu_in=c.opt("celu_in", False))
        if r is None:
            return None
        outs.append(list(r) if isinstance(r, tuple) else [r])
    return outs


def _one_float_in(v):
    """``v`` again, contiguous, but one float into its storage: not 16-byte aligned."""
    buf = torch.empty(v.numel() + 1, device=v.device)
    buf[1:].copy_(v.reshape(-1))
    out = buf[1:].view(v.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _once(c, device):
    """One run from fresh leaves: ``(outs, grads by leaf, leaves, forward kernel names, backward kernel names)``."""
    t_cpu, cots_cpu = C.inputs(c.name)
    t = {n: v.to(device).requires_grad_(C.requires_grad(c, n)) for n, v in t_cpu.items()}
    cots = [ct.to(device) for app in cots_cpu for ct in app]
    if c.opt("sum_cot"):                # what ``out.sum().backward()`` hands the node: every stride 0
        cots[0] = torch.ones((), device=device).expand(cots[0].shape)
    if c.opt("dy_offset"):
        cots[0] = _one_float_in(cots[0])
    with _lib.kernel_timer() as kt:
        if c.opt("scope"):
            with ops.weight_scope():
                apps = _apply(c, t)
        else:
            apps = _apply(c, t)
        torch.cuda.synchronize()
    fwd = [r[0] for r in kt.records()]
    if apps is None:
        return None, {}, t, fwd, []
    outs = [o for app in apps for o in app]
    names = C.leaf_names(c)
    req = [n for n in names if t[n].requires_grad]
    live = [(o, ct) for o, ct in zip(outs, cots) if o.requires_grad]
    grads = {}
    with _lib.kernel_timer() as kt:
        if req and live:
            gs = torch.autograd.grad([o for o, _ in live], [t[n] for n in req], grad_outputs=[ct for _, ct in live], allow_unused=True)
            grads = dict(zip(req, gs))
        torch.cuda.synchronize()
    return outs, grads, t, fwd, [r[0] for r in kt.records()]


def _library_value(c, t):
    """The torch expression a library route names, on the same device tensors."""
    x, w, b = C.op_input(c, t["x"]), t["w"], t.get("b")
    kind = c.opt("lib")
    if kind == "F.linear":
        return F.linear(x, w, b)
    if kind == "addmm":
        return torch.addmm(b, x, w.t() if c.op == "linear" else w)
    y = torch.matmul(x, w)
    return y if b is None else y + b


def _padded_view_expected(c):
    if c.op == "linear":
        return c.route.endswith("/padded") and c.M % 4 != 0
    if c.op == "matmul_tall":
        return c.route == "_MatmulTallRows" and c.M % 4 != 0
    return c.op == "gru_tail" and c.C % 4 != 0 and (c.route.startswith("_GruBlock") or c.route.startswith("_LinearTall"))


def _assert_pad_columns_zero(c, out, what):
    """``out`` is the ``[:, :cols]`` view of rows of ``ceil4(cols)`` floats whose other columns are exactly zero."""
    N, cols = out.shape
    Cp = C.ceil4(cols)
    assert out.stride() == (Cp, 1) and out.storage_offset() == 0, f"{what}: not the view of [N, {Cp}] rows (strides {out.stride()})"
    full = out.detach().as_strided((N, Cp), (Cp, 1))
    assert (full[:, cols:] == 0).all(), f"{what}: pad columns not zero"


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_dense_case(device, monkeypatch, name):
    c = C.BY_NAME[name]
    if c.opt("knob"):
        knob, value = c.opt("knob").split("=")
        assert knob == "RELU_IN_WGRAD" and value == "False" and ops.RELU_IN_WGRAD is True
        monkeypatch.setattr(ops, knob, False)
    try:
        runs = [_once(c, device) for _ in range(2)]
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):      # a faulted device: nothing more is started on it
            pytest.exit(f"{name}: {e}", returncode=3)
        raise
    (o1, g1, t1, _, _), (o2, g2, _, fwd, bwd) = runs
    if c.opt("none"):
        assert o1 is None and o2 is None and fwd == [], (name, fwd)         # outside the class: the caller applies linear + activation
        return
    assert o1 is not None, f"{name}: the op declined"
    # determinism
    assert len(o1) == len(o2) and all(torch.equal(a, b) for a, b in zip(o1, o2)), f"{name}: two runs differ in an output"
    assert g1.keys() == g2.keys()
    for n in g1:
        assert (g1[n] is None) == (g2[n] is None) and (g1[n] is None or torch.equal(g1[n], g2[n])), f"{name}: two runs differ in grad.{n}"
    # labels
    if _lib.route_enabled("x3"):
        assert C.product_labels(fwd) == list(c.fwd), f"{name} ({c.route}) forward launches: {fwd}"
        assert C.product_labels(bwd) == list(c.bwd), f"{name} ({c.route}) backward launches: {bwd}"
    if c.opt("lib") and not c.opt("x_slice"):
        assert torch.equal(o1[0], _library_value(c, t1)), f"{name}: not the bits of the library expression '{c.opt('lib')}'"
    if c.route == "_LinearLib" and c.opt("dy_offset") and "b" in g1:
        dy = _one_float_in(C.inputs(name)[1][0][0].to(device))      # (the reduction's order follows the alignment: the same view)
        assert torch.equal(g1["b"], dy.sum(0)), f"{name}: d_b is not dy.sum(0)"
    # None gradients: exactly the leaves of the request get one
    names = C.leaf_names(c)
    ref64 = C.reference(name)[torch.float64]
    for n, r in zip(names, ref64[1]):
        assert t1[n].grad is None
        if C.requires_grad(c, n) and r is not None:
            assert g1.get(n) is not None, f"{name}: grad.{n} missing"
        else:
            assert g1.get(n) is None, f"{name}: grad.{n} returned for a leaf outside the request"
    if not c.grad:
        assert all(not o.requires_grad for o in o1) and bwd == [], f"{name}: all frozen, yet {bwd}"
    # parity
    assert len(o1) == len(ref64[0])
    if _padded_view_expected(c):
        for k, o in enumerate(o1):
            _assert_pad_columns_zero(c, o, f"{name} out[{k}]")
    assert_twin_parity(C.twin(name, 0), o1[0], [g1.get(n) for n in names], name, names)
    for k in range(1, len(o1)):
        run = C.twin(name, k)
        assert_fp32_parity(o1[k], run(torch.float64)[0], run(torch.float32)[0], f"{name} out[{k}]", k=8.0, out_tol=1e-5)
    if c.op == "matmul_tall" and c.opt("with_identity"):
        assert torch.equal(o1[1], C.op_input(c, t1["x"])), f"{name}: the identity output is not the input"
