"""Ranger (RAdam + Lookahead + gradient centralisation; csrc/optim.hip `k_ranger`, glam_amd.optim.Ranger), host side: the update
restated in float64 against the reference's trajectories (tests/golden/ranger_*.npz, tools/gen_ranger_golden.py), the optimizer's
interface and checkpoint layout, and the C ABI entry point."""
import ctypes
import io
import math
import os
import re

import numpy as np
import pytest
import torch

from glam_amd import _lib
from glam_amd.optim import Ranger  # noqa: F401  (the optimizer these fixtures and the ABI below belong to)
from tests.conftest import ROOT, golden_names

NAMES = golden_names("ranger_")


def load_case(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False)
    n = int(z["n_tensors"])
    hp = {k[3:]: float(z[k]) if z[k].ndim == 0 else tuple(z[k].tolist()) for k in z.files if k.startswith("hp_")}
    case = dict(lr=float(z["lr"]), steps=int(z["steps"]), hp=hp, p0=[z[f"p0_{i}"] for i in range(n)], gin=[z[f"gin_{i}"] for i in range(n)])
    for key in ("p", "exp_avg", "exp_avg_sq", "slow_buffer", "grad"):
        case[key] = [z[f"{key}_{i}"] for i in range(n)]
    return case


def centralised(x, hp):
    """Whether ``centralized_gradient`` touches a tensor of this rank."""
    return bool(hp["use_gc"]) and x.ndim > (3 if hp["gc_conv_only"] else 1)


def row_mean(x):
    return x.mean(axis=tuple(range(1, x.ndim)), keepdims=True)


def ranger64(case):
    """The reference's per-tensor update (ranger.py:117-205) in float64, one step count for all tensors.  Yields per step the
    parameters, exp_avg, exp_avg_sq, slow_buffer and the gradient as the reference leaves it in p.grad."""
    hp, lr = case["hp"], case["lr"]
    b1, b2 = hp["betas"]
    p = [x.astype(np.float64) for x in case["p0"]]
    m = [np.zeros_like(x) for x in p]
    v = [np.zeros_like(x) for x in p]
    slow = [x.copy() for x in p]
    for s in range(1, case["steps"] + 1):
        b2t = b2 ** s
        n_max = 2 / (1 - b2) - 1
        n_sma = n_max - 2 * s * b2t / (1 - b2t)
        rect = n_sma > hp["N_sma_threshhold"]
        if rect:
            step_size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** s)
        else:
            step_size = 1.0 / (1 - b1 ** s)
        out = []
        for i in range(len(p)):
            g = case["gin"][i][s - 1].astype(np.float64)
            gc = centralised(g, hp)
            if gc and hp["gc_loc"]:
                g = g - row_mean(g)
            v[i] = b2 * v[i] + (1 - b2) * g * g
            m[i] = b1 * m[i] + (1 - b1) * g
            G = m[i] / (np.sqrt(v[i]) + hp["eps"]) if rect else m[i]
            if hp["weight_decay"] != 0:
                G = G + hp["weight_decay"] * p[i]
            if gc and not hp["gc_loc"]:
                G = G - row_mean(G)
            if not rect:
                m[i] = G                          # G aliases exp_avg in the reference's un-rectified branch
            p[i] = p[i] - step_size * lr * G
            if s % int(hp["k"]) == 0:
                slow[i] = slow[i] + hp["alpha"] * (p[i] - slow[i])
                p[i] = slow[i].copy()
            out.append((p[i], m[i], v[i], slow[i], g))
        yield s, rect, out


def test_goldens_cover_the_cases_the_issue_names():
    assert NAMES == sorted(["ranger_k1", "ranger_k3", "ranger_k6", "ranger_gc_late", "ranger_gc_conv_only", "ranger_wd"])
    ks = set()
    for name in NAMES:
        c = load_case(name)
        ks.add(int(c["hp"]["k"]))
        assert c["steps"] >= 12
        shapes = [x.shape for x in c["p0"]]
        assert any(s[0] == 1 and len(s) == 2 and s[1] > 256 for s in shapes)       # a [1, N] row longer than one pass of a wave
        assert (1,) in shapes and any(x.size % 2 for x in c["p0"][1:] if x.size > 1)
        assert any(len(s) > 3 for s in shapes)                          # something gc_conv_only centralises
    assert {1, 3, 6} <= ks


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_reproduces_the_golden(name):
    c = load_case(name)
    saw = set()
    for s, rect, out in ranger64(c):
        saw.add(rect)
        for i, (p, m, v, slow, g) in enumerate(out):
            for what, mine, ref in (("p", p, c["p"][i][s - 1]), ("exp_avg", m, c["exp_avg"][i][s - 1]),
                                    ("exp_avg_sq", v, c["exp_avg_sq"][i][s - 1]), ("slow_buffer", slow, c["slow_buffer"][i][s - 1]),
                                    ("grad", g, c["grad"][i][s - 1])):
                scale = max(float(np.abs(ref).max()), 1e-30)
                err = float(np.abs(mine - ref).max())
                # fp32 rounding of the reference, grown over the steps: a few units of 2^-23 per step, relative to the tensor's scale
                assert err <= 2e-6 * s * scale, f"{name} step {s} tensor {i} {what}: {err:.3e} vs scale {scale:.3e}"
    assert saw == {False, True}                                         # the run crosses the rectification switch


def test_goldens_show_the_reference_side_effects():
    c = load_case("ranger_k6")
    # gc_loc=True leaves the centralised gradient in p.grad: 2-D rows have zero mean, 1-D gradients are untouched
    for i, x in enumerate(c["p0"]):
        if x.ndim > 1:
            assert np.abs(row_mean(c["grad"][i][0])).max() < 1e-6
            assert np.abs(row_mean(c["gin"][i][0])).max() > 1e-4
        else:
            np.testing.assert_array_equal(c["grad"][i], c["gin"][i])
    # weight decay in the un-rectified steps lands in exp_avg: the moment is no longer the plain running mean of the gradients
    w, d = load_case("ranger_wd"), load_case("ranger_k6")
    assert np.abs(w["exp_avg"][2][0] - d["exp_avg"][2][0]).max() > 1e-4


def test_constructor_checks_keys_and_attributes():
    from glam_amd.optim import Ranger
    p = [torch.nn.Parameter(torch.zeros(3, 4))]
    for kw, msg in ((dict(alpha=1.5), "Invalid slow update rate: 1.5"), (dict(k=0), "Invalid lookahead steps: 0"),
                    (dict(lr=0.0), "Invalid Learning Rate: 0.0"), (dict(eps=0.0), "Invalid eps: 0.0")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            Ranger(p, **kw)
    opt = Ranger(p, lr=2e-3, k=3)
    g = opt.param_groups[0]
    assert set(g) == {"params", "lr", "alpha", "k", "step_counter", "betas", "N_sma_threshhold", "eps", "weight_decay", "capturable"}
    assert (g["lr"], g["alpha"], g["k"], g["step_counter"], g["betas"], g["N_sma_threshhold"], g["eps"], g["weight_decay"], g["capturable"]) \
        == (2e-3, 0.5, 3, 0, (.95, 0.999), 5, 1e-5, 0, True)
    assert (opt.alpha, opt.k, opt.N_sma_threshhold, opt.use_gc, opt.gc_conv_only, opt.gc_loc) == (0.5, 3, 5, True, False, True)
    assert isinstance(opt, torch.optim.Optimizer)


def test_state_dict_writes_int_steps_and_independent_buffers():
    from glam_amd.optim import Ranger
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]
    opt = Ranger(ps, k=3)
    step = torch.tensor(7.0)                        # the group's device counter, shared by every parameter
    for p in ps:                                    # (planted: building the device plan needs a HIP device)
        opt.state[p].update(step=step, exp_avg=torch.randn_like(p), exp_avg_sq=torch.rand_like(p), slow_buffer=p.detach().clone())
    sd = opt.state_dict()
    for i, p in enumerate(ps):
        st = sd["state"][i]
        assert type(st["step"]) is int and st["step"] == 7
        for b in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            assert torch.equal(st[b], opt.state[p][b]) and st[b].data_ptr() != opt.state[p][b].data_ptr()
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    back = torch.load(buf)
    assert back["param_groups"] == sd["param_groups"]
    assert all(type(st["step"]) is int for st in back["state"].values())
    assert torch.equal(back["state"][0]["exp_avg"], sd["state"][0]["exp_avg"])


def test_no_cpu_fallback():
    from glam_amd.optim import Ranger
    from glam_amd.ops import GlamHipError
    q = torch.nn.Parameter(torch.randn(3, 4))
    q.grad = torch.randn_like(q)
    with pytest.raises(GlamHipError):
        Ranger([q]).step()


def test_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    for name in ("glam_ranger_step", "glam_ranger_max_tensors"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define GLAM_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4


def test_abi_rejects_bad_arguments_without_touching_a_gpu():
    lib = _lib.load()
    assert lib.glam_ranger_max_tensors() >= 36          # a default-shaped model's parameter list goes in one launch
    tab = (ctypes.c_uint64 * 5)(0, 0, 0, 0, 0)
    numel = (ctypes.c_int64 * 1)(8)
    row = (ctypes.c_int64 * 1)(4)
    ok = dict(lr=1e-3, b1=0.95, b2=0.999, eps=1e-5, wd=0.0, alpha=0.5, k=6, thr=5.0, gc_loc=1)

    def call(t=tab, nm=numel, rw=row, n=1, step=8, ticket=8, **over):
        h = dict(ok, **over)
        return lib.glam_ranger_step(t, nm, rw, n, step, ticket, None, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["alpha"], h["k"],
                                    h["thr"], h["gc_loc"], None)

    assert call(step=None, ticket=None) == _lib.GLAM_E_INVALID           # no step counter / ticket
    assert call(rw=None) == _lib.GLAM_E_INVALID                          # no row table
    assert call() == _lib.GLAM_E_INVALID                                 # null tensor addresses
    for bad in (dict(b1=1.0), dict(b2=1.0), dict(eps=0.0), dict(wd=-1.0), dict(alpha=1.5), dict(k=0), dict(thr=float("nan"))):
        assert call(**bad) == _lib.GLAM_E_INVALID, bad
    full = (ctypes.c_uint64 * 5)(*[4096] * 5)
    assert call(t=full, rw=(ctypes.c_int64 * 1)(3)) == _lib.GLAM_E_INVALID   # a row length that does not divide the tensor
    assert call(n=0) == 0                                                # nothing to do
