"""Writes tests/golden/metrics_*.npz: the reference's evaluation metrics (``src_1gp/metrics.py``, ``multi_class_metrics`` of
``src_2gi_ddi/utils.py``, both over sklearn) on fixed synthetic inputs, the fixtures of tests/test_metrics_host.py and
tests/test_gpu_metrics.py.

    python tools/gen_metrics_golden.py --reference <checkout of the reference project>

Only data is written: per case the inputs, the name of the reference function, its result dict on the inputs as given (``ref``) and on
the same inputs cast to float64 (``ref64``), and how many tasks it skipped (its printed message).  Shapes follow the reference's
validation splits with fewer rows where a file would pass ~0.6 MB.  Deterministic: rerunning reproduces the files."""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")


def load_reference(root):
    sys.path.insert(0, os.path.join(ROOT, "oracle", "pyg_standin"))
    stub = types.ModuleType("dataset")       # metrics.py imports dataset_names only (for auto_metrics)
    stub.dataset_names = {"r": ['esol', 'freesolv', 'lipophilicity', 'physprop_perturb'], "c": [], "a": []}
    sys.modules.setdefault("dataset", stub)
    mods = {}
    for name, rel in (("ref_metrics", "src_1gp/metrics.py"), ("ref_ddi_utils", "src_2gi_ddi/utils.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
        mod = importlib.util.module_from_spec(spec)
        with contextlib.redirect_stdout(io.StringIO()):
            spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["ref_metrics"], mods["ref_ddi_utils"]


def quantise(x, levels):
    return (np.floor(x * levels) / levels).astype(x.dtype)


def multi_task(rng, n, t, missing, tied_every=3):
    y = (rng.random((n, t)) < 0.3).astype(np.int64)
    y[rng.random((n, t)) < missing] = -1
    s = rng.random((n, t)).astype(np.float32)
    s = np.where(y == 1, np.minimum(s + 0.25, 1.0), s).astype(np.float32)
    s[:, ::tied_every] = quantise(s[:, ::tied_every], 8)              # heavily tied tasks
    y[:, 1] = np.where(y[:, 1] >= 0, 0, -1)                            # only negatives: skipped
    y[:, 2] = -1                                                       # all missing: skipped
    y[0, 4], y[1, 4] = 0, 1                                            # both classes ...
    s[:, 4] = (s[:, 4] * 0.4).astype(np.float32)                       # ... and no predicted positive (precision 0.0)
    return y, s


def cases(rng):
    out = {}
    y, s = multi_task(rng, 200, 617, 0.7)
    out["toxcast_like"] = ("binary_metrics_multi_target_nan", dict(y_true=y, y_score=s))
    y, s = multi_task(rng, 783, 12, 0.15, tied_every=4)
    out["tox21_like"] = ("binary_metrics_multi_target_nan", dict(y_true=y, y_score=s))

    y = (rng.random(204) < 0.6).astype(np.int64)
    s = quantise(np.clip(rng.random(204) * 0.8 + 0.2 * y, 0, 1).astype(np.float32), 8)
    out["binary_tied"] = ("binary_metrics", dict(y_true=y, y_score=s))
    y = (rng.random(420) < 0.4).astype(np.float32)
    s = rng.random(420).astype(np.float32)
    out["binary_untied_pred"] = ("binary_metrics", dict(y_true=y, y_score=s, y_pred=(rng.random(420) < 0.5).astype(np.int64)))
    y = (rng.random(150) < 0.5)
    s = (rng.random(150) * 0.45).astype(np.float32)
    out["binary_no_positive_pred"] = ("binary_metrics", dict(y_true=y, y_score=s))

    y = quantise(rng.standard_normal(1261).astype(np.float32), 4)      # tied targets
    f = (y + 0.7 * rng.standard_normal(1261)).astype(np.float32)
    f[::5] = quantise(f[::5], 2)
    out["regression_fp32"] = ("regression_metrics", dict(y_true=y, y_pred=f))
    base = rng.standard_normal(420)
    y = np.repeat(base[:105], 4) + np.tile(np.arange(4) * 1e-12, 105)  # fp64 targets 1e-12 apart: they collide in fp32
    f = y + 0.5 * rng.standard_normal(420)
    out["regression_fp64_collide"] = ("regression_metrics", dict(y_true=y, y_pred=f))

    n = 100_000
    y = np.zeros(n, dtype=np.int64)
    y[rng.choice(n, n // 100, replace=False)] = 1
    rank = np.argsort(np.argsort(rng.random(n) + 0.3 * y, kind="stable"), kind="stable")
    s = (rank / n).astype(np.float32)                                   # distinct in fp32: tie-free
    assert np.unique(s).size == n
    out["screening"] = ("screening_metrics", dict(y_true=y, y_score=s))

    n, c = 1000, 86
    y = rng.integers(0, c, n)
    y[y == 7] = 8                                                       # class 7 is never a label ...
    sc = rng.standard_normal((n, c)).astype(np.float32)
    sc[np.arange(n), y] += 1.5
    sc[::9, 7] = sc[::9].max(axis=1) + 1.0                              # ... but is predicted
    sc[::13, 3] = sc[::13].max(axis=1)                                  # tied maxima: the first one wins
    out["ddi_like"] = ("multi_class_metrics", dict(y_true=y, y_score=sc))
    return out


def run(fn, inputs):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        d = fn(**inputs)
    return {k: float(v) for k, v in d.items()}, buf.getvalue().count("Skipped target")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    ref, ddi = load_reference(args.reference)
    fns = {"multi_class_metrics": ddi.multi_class_metrics}
    for name, (fn_name, inputs) in cases(np.random.default_rng(20261016)).items():
        fn = fns.get(fn_name) or getattr(ref, fn_name)
        res, skipped = run(fn, inputs)
        res64, _ = run(fn, {k: v.astype(np.float64) for k, v in inputs.items()})
        meta = dict(fn=fn_name, ref=res, ref64=res64, skipped=skipped, keys=list(res))
        path = os.path.join(OUT, f"metrics_{name}.npz")
        np.savez_compressed(path, meta=np.array(json.dumps(meta)), **{f"in.{k}": v for k, v in inputs.items()})
        print(f"{path}: {os.path.getsize(path)} bytes, skipped {skipped}, {res}")


if __name__ == "__main__":
    main()
