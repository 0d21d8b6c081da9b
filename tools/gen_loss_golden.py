"""Writes tests/golden/loss_*.npz: the reference's criteria (``get_loss`` and ``FocalLoss`` of ``src_1gp/loss.py``; the screening
trainer's ``'wce'``, ``nn.CrossEntropyLoss(weight=train_dataset.weight)``, ``src_2gi_dti_scr/trainer.py:265-267``) on fixed synthetic
inputs, the fixtures of tests/test_losses_host.py and tests/test_gpu_losses.py.

    python tools/gen_loss_golden.py --reference <checkout of the reference project>

Only data is written: per case the float32 inputs (logits / labels / class weights or prediction / target), alpha / gamma where they
apply, and the reference module's mean loss and input gradient evaluated on the inputs cast to float64.  Labels of -100 (the
default ``ignore_index``) mark ignored rows.  Deterministic: rerunning reproduces the files."""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(root, "src_1gp", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(module, inp, target):
    x = torch.from_numpy(inp).double().requires_grad_(True)
    t = torch.from_numpy(target)
    loss = module(x, t.double() if t.is_floating_point() else t)
    loss.backward()
    return np.float64(loss.item()), x.grad.numpy()


def class_case(rng, B, C, ignored, scale):
    x = (rng.standard_normal((B, C)) * scale).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int64)
    y[rng.choice(B, ignored, replace=False)] = -100
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ref = load_reference(ap.parse_args().reference)
    rng = np.random.default_rng(20261016)
    os.makedirs(OUT, exist_ok=True)
    files = {}

    x, y = class_case(rng, 48, 7, 5, 2.0)
    files["ce"] = dict(x=x, y=y, **dict(zip(("loss", "grad"), run(ref.get_loss("ce"), x, y))))
    x, y = class_case(rng, 64, 2, 6, 3.0)
    w = np.array([0.6, 3.1], dtype=np.float32)           # compute_class_weight('balanced') of a screening set with ~16 % binders
    files["wce"] = dict(x=x, y=y, weight=w,
                        **dict(zip(("loss", "grad"), run(torch.nn.CrossEntropyLoss(weight=torch.from_numpy(w).double()), x, y))))
    x, y = class_case(rng, 64, 2, 6, 3.0)
    focal = ref.get_loss("focal")
    files["focal"] = dict(x=x, y=y, alpha=np.float64(focal.alpha), gamma=np.float64(focal.gamma),
                          **dict(zip(("loss", "grad"), run(focal, x, y))))

    n = 257
    for name in ("mae", "huber"):
        p = (rng.standard_normal(n) * 2).astype(np.float32)
        t = (rng.standard_normal(n) * 2).astype(np.float32)
        t[:8] = p[:8]                                    # d = 0: sign(0) = 0
        t[8:12] = p[8:12] + np.float32(1.0)              # |d| at the smooth-L1 threshold (up to the rounding of the sum)
        files[name] = dict(pred=p, target=t, **dict(zip(("loss", "grad"), run(ref.get_loss(name), p, t))))
    p = (1.0 / (1.0 + np.exp(-rng.standard_normal(n) * 3))).astype(np.float32)
    t = (rng.random(n) < 0.3).astype(np.float32)
    files["bce"] = dict(pred=p, target=t, **dict(zip(("loss", "grad"), run(ref.get_loss("bce"), p, t))))

    for name, arrays in files.items():
        path = os.path.join(OUT, f"loss_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{path}: loss {float(arrays['loss']):.9g}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
