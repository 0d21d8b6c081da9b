"""CPU: the criteria table of glam_amd.loss against the reference's (``src_1gp/loss.py:39-58``, ``src_2gi_dti_scr/utils.py:89-92``),
the modules' torch interfaces, the new C ABI symbols, and the focal gradient the kernel computes restated in float64
against the reference's own results (tests/golden/loss_*.npz, from tools/gen_loss_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from glam_amd import _lib, loss
from tests.conftest import GOLD, ROOT

REFERENCE_NAMES = ["mse", "mae", "huber", "smae", "bce", "bcen", "bcel", "bceln", "mtce", "kl", "hinge", "nll", "ce", "focal"]


def fixture(name):
    z = np.load(os.path.join(GOLD, f"loss_{name}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", REFERENCE_NAMES)
def test_get_loss_resolves_every_name_of_the_reference(name):
    assert isinstance(loss.get_loss(name), torch.nn.Module)


def test_get_loss_wce_and_unknown_names():
    assert loss.get_loss("wce") is None                    # the screening trainer builds it (trainer.py:265-267)
    with pytest.raises(ValueError):
        loss.get_loss("no_such_loss")


def test_modules_keep_the_torch_interfaces():
    classes = {"mae": torch.nn.L1Loss, "huber": torch.nn.SmoothL1Loss, "smae": torch.nn.SmoothL1Loss, "bce": torch.nn.BCELoss,
               "ce": torch.nn.CrossEntropyLoss, "bcen": torch.nn.BCELoss, "bceln": torch.nn.BCEWithLogitsLoss,
               "kl": torch.nn.KLDivLoss, "hinge": torch.nn.HingeEmbeddingLoss, "nll": torch.nn.NLLLoss}
    for name, cls in classes.items():
        assert isinstance(loss.get_loss(name), cls), name
    assert loss.get_loss("bcen").reduction == "none" and loss.get_loss("bceln").reduction == "none"
    assert isinstance(loss.get_loss("mse"), loss.MSELoss) and isinstance(loss.get_loss("bcel"), loss.BCEWithLogitsLoss)
    assert isinstance(loss.get_loss("bcel_masked"), loss.MaskedBCEWithLogitsLoss)
    f = loss.get_loss("focal")
    assert isinstance(f, loss.FocalLoss) and f.alpha == 0.25 and f.gamma == 2
    f = loss.FocalLoss(alpha=0.5, gamma=3)
    assert (f.alpha, f.gamma) == (0.5, 3)
    assert isinstance(loss.get_loss("mtce"), loss.MultiTargetCrossEntropy)


def test_cross_entropy_module_state_matches_torch():
    w = torch.tensor([0.6, 3.1])
    ours, theirs = loss.CrossEntropyLoss(weight=w), torch.nn.CrossEntropyLoss(weight=w)
    assert isinstance(ours, torch.nn.CrossEntropyLoss)
    assert ours.state_dict().keys() == theirs.state_dict().keys() == {"weight"}
    assert torch.equal(ours.state_dict()["weight"], theirs.state_dict()["weight"])
    for a in ("ignore_index", "reduction", "label_smoothing"):
        assert getattr(ours, a) == getattr(theirs, a)
    ours2 = loss.CrossEntropyLoss(weight=torch.ones(2))
    ours2.load_state_dict(theirs.state_dict())
    assert torch.equal(ours2.weight, w)
    assert "weight" in dict(ours.named_buffers())


def test_cpu_inputs_run_the_torch_parents():
    # the HIP route is for device tensors; on the CPU every module is its torch parent (the kernels never see a host pointer)
    x, y = torch.randn(6, 3), torch.tensor([0, 2, 1, -100, 2, 0])
    assert torch.equal(loss.CrossEntropyLoss()(x, y), torch.nn.functional.cross_entropy(x, y))
    p, t = torch.rand(9), torch.rand(9)
    assert torch.equal(loss.L1Loss()(p, t), torch.nn.functional.l1_loss(p, t))
    assert torch.equal(loss.SmoothL1Loss()(p, t), torch.nn.functional.smooth_l1_loss(p, t))
    assert torch.equal(loss.BCELoss()(p, t), torch.nn.functional.binary_cross_entropy(p, t))
    x3, y3 = torch.randn(4, 3, 3), torch.randint(0, 3, (4, 3))     # the reference's NLLLoss reads dim 1 as the classes
    ref = torch.nn.functional.nll_loss(torch.log_softmax(x3, dim=2), y3)
    assert torch.equal(loss.get_loss("mtce")(x3, y3), ref)


def test_abi_symbols_in_header_and_bindings():
    header = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    for sym in ("glam_ce_loss_fwd", "glam_ce_loss_max_classes"):
        assert re.search(rf"\b{sym}\(", header), sym
        assert sym in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 4
    assert "kind 4" in header


def test_abi_rejects_bad_arguments_without_touching_a_gpu():
    lib = _lib.load()
    assert lib.glam_ce_loss_max_classes() == 1024
    E = _lib.GLAM_E_INVALID
    p = ctypes.c_void_p(16)             # never dereferenced: every call below fails its checks first
    ok = dict(x=p, y=p, w=None, B=4, C=2, ign=-100, focal=0, alpha=0.25, gamma=2.0)

    def call(**kw):
        a = {**ok, **kw}
        return lib.glam_ce_loss_fwd(a["x"], a["y"], a["w"], a["B"], a["C"], a["ign"], a["focal"], a["alpha"], a["gamma"],
                                    p, p, p, p, 4096, p, None)
    assert call(C=1025) == E and call(C=0) == E and call(B=0) == E and call(B=1 << 22, C=1024) == E
    assert call(focal=2) == E
    assert call(focal=1, gamma=0.5) == E and call(focal=1, w=p) == E
    assert call(x=None) == E
    assert "glam_ce_loss_fwd" in lib.glam_last_error().decode()
    assert lib.glam_loss_fwd(p, p, 4, 5, 0, p, p, p, None, 0, None, None) == E


def focal_f64(x, y, alpha, gamma, ignore_index=-100):
    """The kernel's focal loss and gradient in float64: per row ce, pt = exp(-ce), the factor
    alpha [(1 - pt)^gamma + gamma (1 - pt)^(gamma - 1) pt ce] on (softmax - onehot), the mean over all B rows."""
    x = x.astype(np.float64)
    B, C = x.shape
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    keep = y != ignore_index
    yy = np.where(keep, y, 0)
    ce = np.where(keep, (m[:, 0] - x[np.arange(B), yy]) + np.log(s[:, 0]), 0.0)
    pt = np.exp(-ce)
    omp = -np.expm1(-ce)
    l = alpha * omp ** gamma * ce
    f = alpha * omp ** gamma if gamma == 0 else alpha * (omp ** gamma + gamma * omp ** (gamma - 1) * pt * ce)
    onehot = np.zeros_like(x)
    onehot[np.arange(B), yy] = 1.0
    g = np.where(keep[:, None], f[:, None] * (e / s - onehot), 0.0)
    return l.mean(), g / B


def test_focal_gradient_formula_matches_the_reference():
    z = fixture("focal")
    assert (z["y"] == -100).any()
    val, grad = focal_f64(z["x"], z["y"], float(z["alpha"]), float(z["gamma"]))
    assert abs(val - z["loss"]) <= 1e-12 * max(1.0, abs(float(z["loss"])))
    np.testing.assert_allclose(grad, z["grad"], rtol=0, atol=1e-13)


@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 3.5])
def test_focal_gradient_formula_matches_torch_autograd(gamma):
    rng = np.random.default_rng(int(gamma * 10))
    x = (rng.standard_normal((40, 3)) * 4).astype(np.float32)
    y = rng.integers(0, 3, 40)
    y[::7] = -100
    val, grad = focal_f64(x, y, 0.25, gamma)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(xt, torch.from_numpy(y), reduction="none")
    ref = (0.25 * (1 - torch.exp(-ce)) ** gamma * ce).mean()
    ref.backward()
    assert abs(val - ref.item()) <= 1e-12
    np.testing.assert_allclose(grad, xt.grad.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["ce", "wce"])
def test_cross_entropy_fixtures_match_torch(name):
    z = fixture(name)
    assert (z["y"] == -100).any()
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    w = torch.from_numpy(z["weight"]).double() if "weight" in z else None
    v = torch.nn.functional.cross_entropy(x, torch.from_numpy(z["y"]), weight=w)
    v.backward()
    assert abs(v.item() - z["loss"]) <= 1e-12
    np.testing.assert_allclose(x.grad.numpy(), z["grad"], rtol=0, atol=1e-14)


@pytest.mark.parametrize("name,fn", [("mae", torch.nn.functional.l1_loss), ("huber", torch.nn.functional.smooth_l1_loss),
                                     ("bce", torch.nn.functional.binary_cross_entropy)])
def test_elementwise_fixtures_match_torch(name, fn):
    z = fixture(name)
    p = torch.from_numpy(z["pred"]).double().requires_grad_(True)
    v = fn(p, torch.from_numpy(z["target"]).double())
    v.backward()
    assert abs(v.item() - z["loss"]) <= 1e-12
    np.testing.assert_allclose(p.grad.numpy(), z["grad"], rtol=0, atol=1e-14)
    if name == "mae":
        assert (z["grad"][:8] == 0).all()                 # sign(0) = 0
