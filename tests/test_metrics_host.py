"""CPU: the count formulation of glam_amd.metrics against the reference's own results (tests/golden/metrics_*.npz, from
tools/gen_metrics_golden.py), the C ABI's argument checks, and the loud failure without a HIP device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from glam_amd import _lib
from tests import metrics_restated as R
from tests.conftest import ROOT

NAMES = R.fixture_names()


def test_fixture_set_is_complete():
    assert {n[len("metrics_"):] for n in NAMES} >= {"toxcast_like", "tox21_like", "binary_tied", "binary_untied_pred",
                                                    "binary_no_positive_pred", "regression_fp32", "regression_fp64_collide",
                                                    "screening", "ddi_like"}
    for n in NAMES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) < 640 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_count_formulas_reproduce_the_reference(name):
    meta, inputs = R.load_fixture(name)
    got, skipped = R.restate(meta["fn"], inputs)
    got = {k: float(v) for k, v in got.items()}
    R.check_against_reference(got, meta, name)
    assert skipped == meta["skipped"]


def test_fixtures_cover_the_edge_cases():
    meta, inputs = R.load_fixture("metrics_toxcast_like")
    assert inputs["y_true"].shape == (200, 617) and meta["skipped"] >= 2
    y, s = inputs["y_true"], inputs["y_score"]
    v = y[:, 4] >= 0
    assert (y[v, 4] == 1).any() and (y[v, 4] == 0).any() and not (s[v, 4] >= 0.5).any()     # a kept task with no predicted positive
    meta, inputs = R.load_fixture("metrics_regression_fp64_collide")
    y = inputs["y_true"]
    assert y.dtype == np.float64 and np.unique(y).size > np.unique(y.astype(np.float32)).size
    meta, inputs = R.load_fixture("metrics_screening")
    assert inputs["y_true"].size >= 100_000 and np.unique(inputs["y_score"]).size == inputs["y_score"].size
    meta, inputs = R.load_fixture("metrics_ddi_like")
    pred = np.argmax(inputs["y_score"], axis=1)
    assert inputs["y_score"].shape[1] == 86 and np.setdiff1d(pred, inputs["y_true"]).size > 0


def test_restatement_ties_match_the_trapezoid():
    # all scores equal: AUC 1/2, PR-AUC = the positive rate (one trapezoid from (0, 1) to (1, P/n))
    y = np.array([0, 1, 1, 0, 1])
    d = R.binary_metrics(y, np.full(5, 0.3, dtype=np.float32))
    assert d["auc"] == 0.5 and abs(d["prauc"] - (1 + 3 / 5) / 2) < 1e-15


def test_abi_rejects_bad_arguments_without_touching_a_gpu():
    lib = _lib.load()
    E = _lib.GLAM_E_INVALID
    ws = ctypes.c_void_p(16)            # never dereferenced: every call below fails its checks first
    rec = ctypes.c_void_p(16)
    pct = (ctypes.c_double * 5)(0.01, 0, 0, 0, 0)
    assert lib.glam_metrics_workspace_bytes(-1, 1, 0) == 0
    assert lib.glam_metrics_workspace_bytes(2 ** 31, 1, 0) == 0
    assert lib.glam_metrics_workspace_bytes(10, 0, 0) == 0
    assert lib.glam_metrics_workspace_bytes(10, 1, 4097) == 0
    assert lib.glam_metrics_workspace_bytes(10, 3, 0) > 0
    big = 1 << 40
    args = lambda **kw: {**dict(score=ws, label=ws, pred=None, kd=0, ld=0, n=10, t=1, masked=0, mode=1, thr=0.5, alpha=20.0, pct=pct,
                                npct=1, ws=ws, wsb=big, rec=rec), **kw}
    call = lambda a: lib.glam_metrics_binary(a["score"], a["label"], a["pred"], a["kd"], a["ld"], a["n"], a["t"], a["masked"], a["mode"],
                                             a["thr"], a["alpha"], a["pct"], a["npct"], a["ws"], a["wsb"], a["rec"], None)
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(t=0), dict(score=None), dict(label=None), dict(rec=None), dict(ws=None),
                dict(wsb=8), dict(kd=2), dict(ld=-1), dict(mode=3), dict(mode=0), dict(npct=6), dict(pct=None)):
        assert call(args(**bad)) == E, bad
    assert lib.glam_metrics_regression(None, ws, 0, 10, ws, big, rec, None) == E
    assert lib.glam_metrics_regression(ws, ws, 0, -1, ws, big, rec, None) == E
    assert lib.glam_metrics_regression(ws, ws, 0, 2 ** 31, ws, big, rec, None) == E
    assert lib.glam_metrics_regression(ws, ws, 5, 10, ws, big, rec, None) == E
    assert lib.glam_metrics_regression(ws, ws, 1, 10, ws, big, None, None) == E
    assert lib.glam_metrics_regression(ws, ws, 1, 10, ws, 16, rec, None) == E
    for n_class in (0, -3, 4097):
        assert lib.glam_metrics_multiclass(ws, ws, None, 0, 0, 10, n_class, ws, big, rec, None) == E
        assert b"n_class" in lib.glam_last_error()
    assert lib.glam_metrics_multiclass(ws, None, None, 0, 0, 10, 86, ws, big, rec, None) == E
    assert lib.glam_metrics_multiclass(None, ws, None, 0, 0, 10, 86, ws, big, rec, None) == E
    assert lib.glam_metrics_multiclass(ws, ws, None, 0, 0, -2, 86, ws, big, rec, None) == E
    assert lib.glam_metrics_multiclass(ws, ws, None, 0, 0, 10, 86, ws, 64, rec, None) == E


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    for name in ("glam_metrics_workspace_bytes", "glam_metrics_binary", "glam_metrics_regression", "glam_metrics_multiclass"):
        assert name + "(" in header and name in _lib.SIGNATURES
    assert "metrics.hip" in open(os.path.join(ROOT, "glam_amd", "csrc", "Makefile")).read()


def test_no_cpu_fallback(monkeypatch):
    from glam_amd import metrics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    y, s = np.array([0, 1, 1, 0]), np.array([0.1, 0.9, 0.4, 0.3], dtype=np.float32)
    calls = [lambda: metrics.binary_metrics(y, s), lambda: metrics.binary_metrics_multi_target_nan(y[:, None], s[:, None]),
             lambda: metrics.regression_metrics(s, s), lambda: metrics.cal_ci(s, s), lambda: metrics.screening_metrics(y, s),
             lambda: metrics.bedroc_score(y, s), lambda: metrics.enrichment_factor_single(y, s),
             lambda: metrics.multi_class_metrics(y, np.eye(4, dtype=np.float32))]
    for c in calls:
        with pytest.raises(_lib.GlamHipError, match="no CPU fallback"):
            c()


def test_interface_matches_the_reference():
    import inspect
    from glam_amd import metrics
    sig = {n: str(inspect.signature(getattr(metrics, n))) for n in (
        "binary_metrics", "binary_metrics_multi_target_nan", "regression_metrics", "cal_ci", "screening_metrics", "bedroc_score",
        "enrichment_factor_single", "multi_class_metrics", "auto_metrics")}
    assert sig["binary_metrics"] == "(y_true, y_score, y_pred=None, threshod=0.5)"
    assert sig["binary_metrics_multi_target_nan"] == "(y_true, y_score, y_pred=None, nan_fill=-1, threshod=0.5)"
    assert sig["regression_metrics"] == "(y_true, y_pred)" and sig["cal_ci"] == "(y, f)"
    assert sig["screening_metrics"] == "(y_true, y_score, y_pred=None, threshod=0.5)"
    assert sig["bedroc_score"] == "(y_true, y_score, decreasing=True, alpha=20.0)"
    assert sig["enrichment_factor_single"] == "(y_true, y_score, threshold=0.005)"
    assert sig["multi_class_metrics"] == "(y_true, y_score, y_pred=None)"
    assert metrics.auto_metrics("lipophilicity") == ['valr2', 'r2'] and metrics.auto_metrics("tox21") == ['valauc', 'auc']
    for blend in (metrics.blend_binary_classification, metrics.blend_binary_classification_mt):
        assert inspect.signature(blend).parameters["metrics_fn"].default is metrics.binary_metrics
