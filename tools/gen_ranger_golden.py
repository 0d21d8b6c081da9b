"""Writes tests/golden/ranger_*.npz: trajectories of the reference's Ranger optimizer (``src_1gp/ranger.py``, RAdam + Lookahead + gradient
centralisation) on CPU in fp32, the fixtures of tests/test_ranger_host.py and tests/test_gpu_ranger.py.

    python tools/gen_ranger_golden.py --reference <checkout of the reference project>

Only data is written: per case the hyper-parameters, the initial parameters, a fixed sequence of gradients and, after every step, the
parameters, exp_avg, exp_avg_sq, slow_buffer and p.grad (which the reference centralises in place).  The shapes are the row lengths
and ranks of a default-shaped model's parameters (fewer rows, to keep each file near 0.5 MB) plus a 1-D bias, a [1, N] row walked in
several passes, odd-length tensors and a 4-D tensor (the only rank gc_conv_only centralises).  The full-size shapes — [1024, 300],
[1, 1024], a 307 200-element row — are checked on the device against a restatement (tests/test_gpu_ranger.py).  Deterministic: rerunning reproduces the files."""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 15), (60,), (2, 180), (1, 3, 180), (3, 60), (1, 300), (1, 520), (1,), (5, 13), (37,), (3, 2, 2, 7)]
STEPS = 12
LR = 1e-2
CASES = {
    "ranger_k1": dict(k=1),
    "ranger_k3": dict(k=3),
    "ranger_k6": dict(k=6),
    "ranger_gc_late": dict(k=6, gc_loc=False),
    "ranger_gc_conv_only": dict(k=3, gc_conv_only=True),
    "ranger_wd": dict(k=6, weight_decay=0.05),
}


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_ranger", os.path.join(root, "src_1gp", "ranger.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Ranger


def inputs(seed=0):
    rng = np.random.default_rng(seed)
    p0 = [rng.standard_normal(s).astype(np.float32) * 0.5 for s in SHAPES]
    # a per-row offset on top of the noise, so that centralisation changes the gradients visibly
    grads = [(rng.standard_normal((STEPS,) + s) * 0.1 + rng.standard_normal((STEPS, s[0]) + (1,) * (len(s) - 1)) * 0.05).astype(np.float32)
             for s in SHAPES]
    return p0, grads


def trajectory(Ranger, kw, p0, grads):
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    opt = Ranger(params, lr=LR, **kw)
    rec = {key: [[] for _ in params] for key in ("p", "exp_avg", "exp_avg_sq", "slow_buffer", "grad")}
    for s in range(STEPS):
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g[s].copy())
        opt.step()
        for i, p in enumerate(params):
            st = opt.state[p]
            rec["p"][i].append(p.detach().numpy().copy())
            rec["grad"][i].append(p.grad.numpy().copy())
            for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
                rec[key][i].append(st[key].numpy().copy())
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project (src_1gp/ranger.py is imported from it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    Ranger = load_reference(args.reference)
    p0, grads = inputs()
    for name, kw in CASES.items():
        full = dict(alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0.0, use_gc=True, gc_conv_only=False,
                    gc_loc=True)
        full.update(kw)
        rec = trajectory(Ranger, kw, p0, grads)
        arrays = {"lr": np.float64(LR), "steps": np.int64(STEPS), "n_tensors": np.int64(len(SHAPES))}
        for key, val in full.items():
            arrays["hp_" + key] = np.asarray(val, dtype=np.float64)
        for i in range(len(SHAPES)):
            arrays[f"p0_{i}"] = p0[i]
            arrays[f"gin_{i}"] = grads[i]
            for key, per in rec.items():
                arrays[f"{key}_{i}"] = np.stack(per[i])
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
