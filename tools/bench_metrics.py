"""Per-call cost of glam_amd.metrics at the shapes of the reference's validation splits: end to end (numpy in, dict out), the kernels
alone (per-dispatch timestamps, glam_amd._lib.kernel_timer), and the equivalent sklearn calls on this host when sklearn is importable
(the reference's metrics.py is sklearn per task plus cal_ci's Python pair loop, restated here as plain loops over the same calls).

    python tools/bench_metrics.py [--reps 20] [--json out.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glam_amd import _lib, metrics as M  # noqa: E402

try:
    from sklearn import metrics as skm
except ImportError:       # the device numbers still stand on their own
    skm = None


def multi_task(rng, n, t, missing):
    y = (rng.random((n, t)) < 0.3).astype(np.int64)
    y[rng.random((n, t)) < missing] = -1
    return y, rng.random((n, t)).astype(np.float32)


def cases(rng):
    y, s = multi_task(rng, 858, 617, 0.7)
    yield "toxcast valid 858 x 617, 70 % missing", "binary_metrics_multi_target_nan", dict(y_true=y, y_score=s)
    y, s = multi_task(rng, 783, 12, 0.15)
    yield "tox21 valid 783 x 12", "binary_metrics_multi_target_nan", dict(y_true=y, y_score=s)
    for n, name in ((1261, "physprop_perturb valid"), (420, "lipophilicity valid"), (10_000, "DTI-sized test set")):
        y = rng.standard_normal(n).astype(np.float32)
        yield f"{name} n = {n}", "regression_metrics", dict(y_true=y, y_pred=(y + rng.standard_normal(n)).astype(np.float32))
    y = (rng.random(204) < 0.5).astype(np.int64)
    yield "bbbp valid n = 204", "binary_metrics", dict(y_true=y, y_score=rng.random(204).astype(np.float32))
    n = 100_000
    y = np.zeros(n, dtype=np.int64)
    y[rng.choice(n, n // 100, replace=False)] = 1
    yield "screening n = 1e5, 1 % actives", "screening_metrics", dict(y_true=y, y_score=rng.random(n).astype(np.float32))


# ---- the sklearn side: the same calls the reference makes ----------------------------------------------------------------------
def _ci_loop(y, f):
    z = s = 0.0
    for i in range(len(y)):
        for j in range(len(y)):
            if y[i] > y[j]:
                z += 1
                u = f[i] - f[j]
                s += 1.0 if u > 0 else 0.5 if u == 0 else 0.0
    return s / z


def sk_call(fn, d):
    if fn == "binary_metrics":
        y, s = d["y_true"], d["y_score"]
        p = (s >= 0.5).astype(int)
        pr, rc, _ = skm.precision_recall_curve(y, s)
        return [skm.roc_auc_score(y, s), skm.auc(rc, pr), skm.accuracy_score(y, p), skm.precision_score(y, p, average='macro'),
                skm.recall_score(y, p, average='macro'), skm.f1_score(y, p, average='macro')]
    if fn == "binary_metrics_multi_target_nan":
        y, s = d["y_true"], d["y_score"]
        p = (s >= 0.5).astype(int)
        out = []
        for i in range(y.shape[1]):
            v = y[:, i] >= 0
            if (y[v, i] == 1).sum() == 0 or (y[v, i] == 0).sum() == 0:
                continue
            out.append((skm.roc_auc_score(y[v, i], s[v, i]), skm.accuracy_score(y[v, i], p[v, i]),
                        skm.precision_score(y[v, i], p[v, i], zero_division=0), skm.recall_score(y[v, i], p[v, i])))
        return out
    if fn == "regression_metrics":
        y, f = d["y_true"], d["y_pred"]
        return [_ci_loop(y, f) if y.size <= 2000 else None, skm.mean_squared_error(y, f), skm.r2_score(y, f)]
    if fn == "screening_metrics":
        y, s = d["y_true"], d["y_score"]
        p = (s > 0.5).astype(int)
        order = np.argsort(-s)
        return [skm.roc_auc_score(y, s), skm.accuracy_score(y, p), skm.precision_score(y, p), skm.recall_score(y, p), order[:5]]
    raise ValueError(fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: no HIP device")
    dev_name = torch.cuda.get_device_name(0)
    rows = []
    for label, fn, d in cases(np.random.default_rng(0)):
        f = getattr(M, fn)
        with contextlib.redirect_stdout(io.StringIO()):
            f(**d)                                        # warm-up: module load, allocator, code objects
            torch.cuda.synchronize()
            e2e = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                f(**d)
                e2e.append(time.perf_counter() - t0)
            with _lib.kernel_timer() as kt:
                f(**d)
            torch.cuda.synchronize()
        rec = kt.records()
        kernel_us = sum(us for _, _, us in rec)
        row = dict(case=label, fn=fn, e2e_ms=1e3 * float(np.median(e2e)), kernel_us=kernel_us,
                   kernels=[(k, g, round(us, 2)) for k, g, us in rec], device=dev_name)
        if skm is not None:
            reps = 1 if fn == "regression_metrics" and d["y_true"].size > 1000 else 3
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                sk_call(fn, d)
                t.append(time.perf_counter() - t0)
            row["sklearn_ms"] = 1e3 * min(t)
            if fn == "regression_metrics" and d["y_true"].size > 2000:
                row["sklearn_note"] = "sklearn parts only; the Python pair loop (cal_ci) is O(n^2) and not timed at this n"
        rows.append(row)
        print(f"{label:40s} e2e {row['e2e_ms']:8.3f} ms   kernels {kernel_us:9.1f} us"
              + (f"   sklearn {row['sklearn_ms']:9.1f} ms" if "sklearn_ms" in row else ""), flush=True)
    print(f"device: {dev_name}; host cpus visible: {os.cpu_count()}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
