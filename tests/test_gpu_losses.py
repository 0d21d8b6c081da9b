"""GPU: the cross-entropy family (``glam_ce_loss_fwd``) and the elementwise kinds 2-4 of ``glam_loss_fwd`` against torch in float64,
the reference's fixtures (tests/golden/loss_*.npz), run-to-run bit equality, the absence of ATen compute in a HIP-routed criterion,
the torch fallbacks, the nan of a label outside [0, C), and a captured two-tower screening step with 'wce' and 'focal'."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from glam_amd import loss
from tests.conftest import GOLD

pytestmark = pytest.mark.gpu

G_UP = 1.7          # a non-unit gradient arriving at the loss


def hip_run(fn, x, *args):
    x = x.detach().clone().requires_grad_(True)
    v = fn(x, *args)
    (g,) = torch.autograd.grad(v, x, torch.full((), G_UP, device=x.device))
    return v.detach(), g


def ref_run(fn, x, *args):
    x = x.detach().double().requires_grad_(True)
    v = fn(x, *args)
    (g,) = torch.autograd.grad(v, x, torch.full((), G_UP, dtype=torch.float64, device=x.device))
    return v.detach(), g


def check(got, ref, what):
    (v, g), (rv, rg) = got, ref
    v, rv = float(v), float(rv)
    assert abs(v - rv) <= 2e-6 * abs(rv) + 1e-30, f"{what}: value {v!r} vs {rv!r}"
    err = (g.double() - rg).abs().max().item()
    assert err <= 1e-6 * max(1.0, rg.abs().max().item()), f"{what}: gradient max|d| {err:.3e}"


def focal_ref(x, y, alpha, gamma):
    ce = F.cross_entropy(x, y, reduction="none")
    pt = torch.exp(-ce)
    return (alpha * (1 - pt) ** gamma * ce).mean()


def class_inputs(B, C, device, seed, scale=2.0, ignored=True):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(B, C, generator=g) * scale).to(device)
    y = torch.randint(0, C, (B,), generator=g)
    if ignored and B > 1:
        y[torch.randperm(B, generator=g)[: max(1, B // 7)]] = -100
    return x, y.to(device)


@pytest.mark.parametrize("C", [2, 3, 86, 1024])
@pytest.mark.parametrize("B", [1, 31, 32, 1024, 40000])
def test_cross_entropy_family_matches_torch_fp64(device, B, C):
    x, y = class_inputs(B, C, device, seed=B * 7 + C)
    w = (torch.rand(C, generator=torch.Generator().manual_seed(C)) * 3 + 0.1).to(device)
    check(hip_run(loss.cross_entropy, x, y), ref_run(F.cross_entropy, x, y), f"ce B={B} C={C}")
    check(hip_run(loss.cross_entropy, x, y, w), ref_run(lambda a, b: F.cross_entropy(a, b, weight=w.double()), x, y),
          f"wce B={B} C={C}")
    check(hip_run(loss.focal_loss, x, y), ref_run(focal_ref, x, y, 0.25, 2), f"focal B={B} C={C}")
    m = loss.CrossEntropyLoss(weight=w)
    check(hip_run(m, x, y), ref_run(lambda a, b: F.cross_entropy(a, b, weight=w.double()), x, y), f"module wce B={B} C={C}")


@pytest.mark.parametrize("gamma", [0, 1, 2, 3.5])
@pytest.mark.parametrize("B,C", [(31, 2), (1024, 2), (1024, 86), (40000, 3), (32, 1024)])
def test_focal_gammas_match_torch_fp64(device, B, C, gamma):
    x, y = class_inputs(B, C, device, seed=B + C + int(gamma * 10), scale=3.0)
    mod = loss.FocalLoss(alpha=0.4, gamma=gamma)
    check(hip_run(mod, x, y), ref_run(focal_ref, x, y, 0.4, gamma), f"focal gamma={gamma} B={B} C={C}")


@pytest.mark.parametrize("C", [2, 86])
def test_large_logits(device, C):
    x, y = class_inputs(1024, C, device, seed=C, scale=1.0)
    x = torch.where(x > 0, 80.0, -80.0) + x * 0.01               # logits of about +-80: confident rows, right and wrong
    w = torch.linspace(0.5, 2.0, C, device=device)
    check(hip_run(loss.cross_entropy, x, y), ref_run(F.cross_entropy, x, y), "ce +-80")
    check(hip_run(loss.cross_entropy, x, y, w), ref_run(lambda a, b: F.cross_entropy(a, b, weight=w.double()), x, y), "wce +-80")
    for gamma in (0, 1, 2, 3.5):
        check(hip_run(loss.focal_loss, x, y, 0.25, gamma), ref_run(focal_ref, x, y, 0.25, gamma), f"focal +-80 gamma={gamma}")


def test_all_rows_ignored_give_nan_like_torch(device):
    x = torch.randn(40, 3, device=device)
    y = torch.full((40,), -100, dtype=torch.int64, device=device)
    v, g = hip_run(loss.cross_entropy, x, y)
    rv, rg = ref_run(F.cross_entropy, x, y)
    assert torch.isnan(v) and torch.isnan(rv)
    assert torch.equal(g, rg.float())                          # torch's zero gradient
    v, g = hip_run(loss.focal_loss, x, y)                      # the focal mean runs over all rows: 0
    assert v.item() == 0.0 and not g.any()
    y2 = torch.full((40,), 5, dtype=torch.int64, device=device)
    v, g = hip_run(loss.CrossEntropyLoss(ignore_index=5), x, y2)
    assert torch.isnan(v) and not g.any()


@pytest.mark.parametrize("name,kind_fn,ref_fn", [
    ("mae", loss.L1Loss(), F.l1_loss), ("huber", loss.SmoothL1Loss(), F.smooth_l1_loss), ("smae", loss.get_loss("smae"), F.smooth_l1_loss),
    ("bce", loss.BCELoss(), F.binary_cross_entropy)])
@pytest.mark.parametrize("n", [1, 33, 1025, 631808])
def test_elementwise_kinds_match_torch_fp64(device, name, kind_fn, ref_fn, n):
    g = torch.Generator().manual_seed(n)
    if name == "bce":
        p = torch.sigmoid(torch.randn(n, generator=g) * 3).to(device)
        t = (torch.rand(n, generator=g) < 0.3).float().to(device)
        p[: min(n, 3)] = torch.tensor([0.0, 1.0, 0.5])[: min(n, 3)].to(device)     # the -100 clamp and the 1e-12 floor
    else:
        p = (torch.randn(n, generator=g) * 2).to(device)
        t = (torch.randn(n, generator=g) * 2).to(device)
        t[: n // 3] = p[: n // 3]                               # d = 0
    tt = t.double()
    check(hip_run(kind_fn, p, t), ref_run(lambda a: ref_fn(a, tt), p), f"{name} n={n}")


def test_bce_clamps_like_torch(device):
    p = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.3], device=device)
    t = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.5], device=device)
    v, g = hip_run(loss.bce_loss, p, t)
    rv, rg = ref_run(lambda a: F.binary_cross_entropy(a, t.double()), p)
    assert abs(v.item() - rv.item()) <= 2e-6 * abs(rv.item())
    assert torch.allclose(g.double(), rg, rtol=2e-6, atol=0)


@pytest.mark.parametrize("name", ["ce", "wce", "focal", "mae", "huber", "bce"])
def test_reference_fixtures(device, name):
    z = np.load(os.path.join(GOLD, f"loss_{name}.npz"), allow_pickle=False)
    if "x" in z.files:
        x, y = torch.from_numpy(z["x"]).to(device), torch.from_numpy(z["y"]).to(device)
        if name == "focal":
            mod, args = loss.FocalLoss(alpha=float(z["alpha"]), gamma=float(z["gamma"])), (y,)
        else:
            mod = loss.CrossEntropyLoss(weight=torch.from_numpy(z["weight"]).to(device) if "weight" in z.files else None)
            args = (y,)
    else:
        x, args = torch.from_numpy(z["pred"]).to(device), (torch.from_numpy(z["target"]).to(device),)
        mod = loss.get_loss(name)
    xx = x.clone().requires_grad_(True)
    v = mod(xx, *args)
    (g,) = torch.autograd.grad(v, xx)
    rv, rg = float(z["loss"]), torch.from_numpy(z["grad"]).to(device)
    assert abs(v.item() - rv) <= 2e-6 * abs(rv)
    assert (g.double() - rg).abs().max().item() <= 1e-6 * max(1.0, rg.abs().max().item())


def test_bit_reproducible(device):
    cases = []
    x, y = class_inputs(40000, 2, device, seed=1)
    w = torch.tensor([0.6, 3.1], device=device)
    cases += [(loss.cross_entropy, x, y, w), (loss.focal_loss, x, y)]
    x, y = class_inputs(40000, 86, device, seed=2)
    cases += [(loss.cross_entropy, x, y), (loss.focal_loss, x, y, 0.25, 3.5)]
    x, y = class_inputs(3000, 1024, device, seed=3)
    cases += [(loss.cross_entropy, x, y)]
    p, t = torch.randn(631808, device=device), torch.randn(631808, device=device)
    cases += [(loss.l1_loss, p, t), (loss.smooth_l1_loss, p, t), (loss.bce_loss, torch.sigmoid(p), torch.sigmoid(t))]
    for fn, a, *rest in cases:
        v1, g1 = hip_run(fn, a, *rest)
        v2, g2 = hip_run(fn, a, *rest)
        assert torch.equal(v1, v2) and torch.equal(g1, g2), fn.__name__


_VIEWS = ("empty", "empty_like", "empty_strided", "view", "_unsafe_view", "as_strided", "select", "slice", "alias", "detach",
          "reshape", "expand", "lift_fresh", "t", "unsqueeze", "squeeze")


def _routed_criteria(device):
    x2, y2 = class_inputs(1024, 2, device, seed=5)
    x86, y86 = class_inputs(256, 86, device, seed=6)
    w = torch.tensor([0.6, 3.1], device=device)
    p, t = torch.randn(4096, device=device), torch.randn(4096, device=device)
    return [("wce", loss.CrossEntropyLoss(weight=w), x2, y2, "k_ce_fwd"),
            ("ce", loss.get_loss("ce"), x86, y86, "k_ce_fwd"),
            ("focal", loss.get_loss("focal"), x2, y2, "k_ce_fwd"),
            ("mae", loss.get_loss("mae"), p, t, "k_loss_fwd"),
            ("huber", loss.get_loss("huber"), p, t, "k_loss_fwd"),
            ("bce", loss.get_loss("bce"), torch.sigmoid(p), torch.sigmoid(t), "k_loss_fwd")]


def test_no_aten_compute_in_the_criterion(device):
    from torch.utils._python_dispatch import TorchDispatchMode
    one = torch.ones((), device=device)
    for name, mod, a, b, _ in _routed_criteria(device):
        x = a.clone().requires_grad_(True)
        mod(x, b).backward(gradient=one)                       # warm: the ticket buffer, the caching allocator
        x = a.clone().requires_grad_(True)
        torch.cuda.synchronize()
        seen = []

        class Log(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                op = str(func).split(".")[1]
                if op not in _VIEWS:
                    seen.append(str(func))
                return func(*args, **(kwargs or {}))
        with Log():
            mod(x, b).backward(gradient=one)
        torch.cuda.synchronize()
        assert x.grad is not None and torch.isfinite(x.grad).all()
        assert not seen, f"{name}: {seen}"


def test_two_device_kernels_per_step(device):
    from torch.profiler import ProfilerActivity, profile
    one = torch.ones((), device=device)
    for name, mod, a, b, fwd in _routed_criteria(device):
        x = a.clone().requires_grad_(True)
        mod(x, b).backward(gradient=one)
        x = a.clone().requires_grad_(True)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            mod(x, b).backward(gradient=one)
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        assert len(kernels) == 2, f"{name}: {kernels}"
        assert any(fwd in k for k in kernels) and any("k_loss_bwd" in k for k in kernels), f"{name}: {kernels}"


def test_fallbacks_equal_torch(device):
    x, y = class_inputs(64, 5, device, seed=9)
    yc = y.clamp(min=0)
    w = torch.rand(5, device=device) + 0.5
    soft = torch.softmax(torch.randn(64, 5, device=device), 1)
    cases = [(loss.CrossEntropyLoss(weight=w, reduction="none"), torch.nn.CrossEntropyLoss(weight=w, reduction="none"), x, y),
             (loss.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(), x, soft),
             (loss.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(), x.double(), y),
             (loss.CrossEntropyLoss(label_smoothing=0.1), torch.nn.CrossEntropyLoss(label_smoothing=0.1), x, y),
             (loss.FocalLoss(gamma=0.5), None, x, yc),           # (no ignored rows: torch's own gradient is 0 * inf there)
             (loss.FocalLoss(), None, x.double(), y)]
    p, t = torch.rand(300, device=device), torch.rand(300, device=device)
    for ours, theirs in ((loss.L1Loss, torch.nn.L1Loss), (loss.SmoothL1Loss, torch.nn.SmoothL1Loss), (loss.BCELoss, torch.nn.BCELoss)):
        cases += [(ours(reduction="none"), theirs(reduction="none"), p, t), (ours(), theirs(), p.double(), t.double())]
    cases += [(loss.SmoothL1Loss(beta=0.5), torch.nn.SmoothL1Loss(beta=0.5), p, t)]
    for ours, theirs, a, b in cases:
        if theirs is None:
            theirs = lambda u, v, m=ours: focal_ref(u, v, m.alpha, m.gamma)      # noqa: E731
        xa, xb = a.clone().requires_grad_(True), a.clone().requires_grad_(True)
        va, vb = ours(xa, b), theirs(xb, b)
        assert torch.equal(va, vb)
        va.sum().backward()
        vb.sum().backward()
        assert torch.equal(xa.grad, xb.grad)


def test_label_out_of_range_gives_nan_without_a_fault(device):
    x, y = class_inputs(256, 3, device, seed=11, ignored=False)
    for bad in (3, 1 << 40, -1, -7):
        yb = y.clone()
        yb[17] = bad
        for fn in (loss.cross_entropy, loss.focal_loss):
            v, g = hip_run(fn, x, yb)
            assert torch.isnan(v), (fn.__name__, bad)
            assert torch.isnan(g[17]).all() and torch.isfinite(torch.cat([g[:17], g[18:]])).all()
    torch.cuda.synchronize()
    v, _ = hip_run(loss.cross_entropy, x, y)                   # the device is unharmed
    assert torch.isfinite(v)


def _dti_step_matches_replay(device, make_criterion):
    from glam_amd import model, ops, optim
    saved = ops.USE_TORCH_EXT
    ops.USE_TORCH_EXT = False          # the route a capture takes (ops._want_torch_ext), for the eager steps too
    try:
        _dti_steps(device, make_criterion, model, optim)
    finally:
        ops.USE_TORCH_EXT = saved


def _dti_steps(device, make_criterion, model, optim):
    from glam_amd.data import synth_batch, synth_protein_batch
    B = 16
    torch.manual_seed(0)
    net_e = model.ArchitectureDTI(out_dim=2, graph_do="_None()", end_do="_None()", pre_act="ReLU", graph_act="ReLU",
                                  flat_act="ReLU", end_act="ReLU").to(device)
    net_g = copy.deepcopy(net_e)
    mol = synth_batch(B, seed=0).to(device)
    pro = synth_protein_batch(B, seed=1, n_min=60, n_max=200).to(device)
    y = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(3)).to(device)
    crit = make_criterion()
    one = torch.ones((), device=device)
    nets = {}
    for key, net in (("e", net_e), ("g", net_g)):
        opt = optim.Adam(net.parameters(), lr=1e-3)
        out = {}

        def body(net=net, opt=opt, out=out):
            opt.zero_grad(set_to_none=True)
            l = crit(net(mol, pro), y)
            l.backward(gradient=one)
            opt.step()
            out["loss"] = l.detach()
        nets[key] = (net, body, out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for key in ("e", "g"):                                  # the same eager warm-up steps on both copies
            for _ in range(2):
                nets[key][1]()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for pe, pg in zip(net_e.parameters(), net_g.parameters()):
        assert torch.equal(pe, pg)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nets["g"][1]()
    static_loss = nets["g"][2]["loss"]
    for step in range(3):
        nets["e"][1]()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(nets["e"][2]["loss"], static_loss), step
        assert torch.isfinite(static_loss)
        for (n, pe), pg in zip(net_e.named_parameters(), net_g.parameters()):
            assert torch.equal(pe, pg), (step, n)


def test_captured_dti_step_wce(device):
    w = torch.tensor([0.6, 3.1], device=device)
    _dti_step_matches_replay(device, lambda: loss.CrossEntropyLoss(weight=w))


def test_captured_dti_step_focal(device):
    _dti_step_matches_replay(device, lambda: loss.get_loss("focal"))
