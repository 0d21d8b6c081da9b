"""GPU: glam_amd.metrics (csrc/metrics.hip) against the reference's results (tests/golden/metrics_*.npz) and, on fresh random cases,
against the count-form restatement of tests/metrics_restated.py; input forms, run-to-run bit equality and the reference's errors."""
import numpy as np
import pytest
import torch

from glam_amd import metrics as M
from tests import metrics_restated as R

pytestmark = pytest.mark.gpu

NAMES = R.fixture_names()


def _call(fn_name, inputs):
    return getattr(M, fn_name)(**inputs)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_matches_the_reference(device, name, capsys):
    meta, inputs = R.load_fixture(name)
    got = _call(meta["fn"], inputs)
    R.check_against_reference(got, meta, name)
    assert capsys.readouterr().out.count("Skipped target") == meta["skipped"]
    # the same call on the inputs cast to float64 (the DTI trainers' labels arrive so)
    got64 = _call(meta["fn"], {k: v.astype(np.float64) for k, v in inputs.items()})
    R.check_against_reference(got64, {**meta, "ref": meta["ref64"]}, name + " (float64)")


def _close(got, want, what, tol=1e-12):
    assert list(got) == list(want), what
    for k in want:
        w = float(want[k])
        t = tol * max(1.0, abs(w)) if k in ("bedroc", "mse", "rmse", "r2") or k.startswith("ef_") else tol
        assert abs(got[k] - w) <= t, f"{what}[{k}]: {got[k]!r} vs {w!r}"


def _labels(rng, n, kind, pos=0.4):
    y = rng.random(n) < pos
    return {"bool": y, "int": y.astype(np.int32), "float": y.astype(np.float32), "f64": y.astype(np.float64)}[kind]


def _scores(rng, n, form, dtype=np.float32):
    s = rng.random(n)
    if form == "q8":
        s = np.floor(s * 8) / 8
    elif form == "equal":
        s = np.full(n, 0.625)
    return s.astype(dtype)


@pytest.mark.parametrize("n,form,lab", [(2, "plain", "int"), (3, "equal", "bool"), (17, "q8", "float"), (255, "plain", "f64"),
                                        (257, "q8", "int"), (1000, "equal", "int"), (4099, "q8", "bool"), (2 ** 17 + 3, "plain", "float"),
                                        (2 ** 17 + 3, "q8", "int")])
def test_binary_random(device, n, form, lab):
    rng = np.random.default_rng(n + len(form))
    y = _labels(rng, n, lab)
    y[0], y[-1] = 0, 1
    s = _scores(rng, n, form)
    _close(M.binary_metrics(y, s), R.binary_metrics(y, s), f"binary n={n} {form}")
    d = M.screening_metrics(y, s)
    _close(d, R.screening_metrics(y, s), f"screening n={n} {form}", tol=1e-11)


def test_single_sample_and_single_class(device):
    with pytest.raises(ValueError):
        M.binary_metrics(np.array([1]), np.array([0.3], dtype=np.float32))
    with pytest.raises(ValueError):
        M.screening_metrics(np.zeros(50, dtype=np.int64), np.linspace(0, 1, 50))
    assert M.enrichment_factor_single(np.array([1]), np.array([0.3])) == pytest.approx(0.0)   # int(1 * 0.005) = 0: no hit


@pytest.mark.parametrize("n,t,missing", [(1, 1, 0.0), (64, 3, 0.5), (858, 617, 0.7), (300, 40, 0.99), (2000, 12, 0.15)])
def test_multi_task_random(device, n, t, missing, capsys):
    rng = np.random.default_rng(n * t)
    y = (rng.random((n, t)) < 0.3).astype(np.int64)
    y[rng.random((n, t)) < missing] = -1
    s = rng.random((n, t)).astype(np.float32)
    s[:, ::2] = np.floor(s[:, ::2] * 8) / 8
    want, skipped = R.binary_metrics_multi_target_nan(y, s)
    if want is None:
        with pytest.raises(ZeroDivisionError):
            M.binary_metrics_multi_target_nan(y, s)
    else:
        _close(M.binary_metrics_multi_target_nan(y, s), want, f"multi {n}x{t}")
    assert capsys.readouterr().out.count("Skipped target") == skipped


@pytest.mark.parametrize("n,form,dtype", [(2, "plain", np.float32), (300, "q8", np.float32), (1261, "plain", np.float64),
                                          (4100, "q8", np.float64)])
def test_regression_random(device, n, form, dtype):
    rng = np.random.default_rng(n)
    y = rng.standard_normal(n).astype(dtype)
    if form == "q8":
        y = np.floor(y * 8) / 8
    y[0], y[-1] = -3.0, 3.0
    f = (y + rng.standard_normal(n)).astype(dtype)
    if form == "q8":
        f = np.floor(f * 4) / 4
    _close(M.regression_metrics(y, f), R.regression_metrics(y, f), f"regression n={n}")


def test_fp64_keys_stay_fp64(device):
    rng = np.random.default_rng(5)
    base = rng.standard_normal(300)
    y = np.repeat(base, 3) + np.tile(np.array([0.0, 1e-12, 2e-12]), 300)         # distinct in fp64, equal in fp32
    f = y + 0.3 * rng.standard_normal(900)
    assert np.unique(y.astype(np.float32)).size < np.unique(y).size
    assert M.cal_ci(y, f) == R.regression_metrics(y, f)["ci"]
    assert M.cal_ci(y, f) != R.regression_metrics(y.astype(np.float32), f.astype(np.float32))["ci"]
    lab = (rng.random(900) < 0.5).astype(np.float64)
    s = np.repeat(rng.random(300), 3) + np.tile(np.array([0.0, 1e-13, 2e-13]), 300)
    _close(M.binary_metrics(lab, s), R.binary_metrics(lab, s), "binary fp64 scores")


@pytest.mark.parametrize("n,c", [(1, 2), (500, 86), (3000, 7), (200, 300)])
def test_multi_class_random(device, n, c):
    rng = np.random.default_rng(n + c)
    y = rng.integers(0, c, n)
    sc = np.floor(rng.random((n, c)) * 4).astype(np.float32)             # many tied maxima: the first one wins
    _close(M.multi_class_metrics(y, sc), R.multi_class_metrics(y, sc), f"multiclass {n}x{c}")
    pred = rng.integers(0, c, n)
    _close(M.multi_class_metrics(y, sc, y_pred=pred), R.multi_class_metrics(y, sc, y_pred=pred), f"multiclass pred {n}x{c}")


def test_input_forms_and_bit_equality(device):
    meta, inputs = R.load_fixture("metrics_toxcast_like")
    y, s = inputs["y_true"], inputs["y_score"]
    a = M.binary_metrics_multi_target_nan(y, s)
    b = M.binary_metrics_multi_target_nan(torch.from_numpy(y), torch.from_numpy(s))
    c = M.binary_metrics_multi_target_nan(torch.from_numpy(y).to(device), torch.from_numpy(s).to(device))
    d = M.binary_metrics_multi_target_nan(y, s)
    assert a == b == c == d
    meta, inputs = R.load_fixture("metrics_screening")
    r = [M.screening_metrics(**inputs), M.screening_metrics(torch.from_numpy(inputs["y_true"]).to(device),
                                                            torch.from_numpy(inputs["y_score"]).to(device))]
    meta, inputs = R.load_fixture("metrics_regression_fp32")
    q = [M.regression_metrics(**inputs), M.regression_metrics(**{k: torch.from_numpy(v) for k, v in inputs.items()})]
    assert r[0] == r[1] and q[0] == q[1]
    for d in (a, r[0], q[0]):
        assert all(type(v) is float for v in d.values())


def test_blends_take_tensors(device):
    rng = np.random.default_rng(3)
    y = torch.from_numpy((rng.random(100) < 0.5).astype(np.int64))
    outs = [(y, (torch.rand(100) > 0.5).long(), torch.rand(100)) for _ in range(3)]
    d = M.blend_binary_classification(outs)
    pl = torch.stack([o[1] for o in outs], 1).mode(1)[0]
    ss = torch.stack([o[2] for o in outs], 1).mean(1)
    _close(d, R.binary_metrics(y.numpy(), ss.numpy(), y_pred=pl.numpy()), "blend")
    yr = torch.randn(50, dtype=torch.float64)
    outs = [(yr, yr + 0.3 * torch.randn(50, dtype=torch.float64)) for _ in range(2)]
    pr = M.blend_regression(outs, return_pred=True)
    _close(M.blend_regression(outs), R.regression_metrics(yr.numpy(), pr.numpy()), "blend regression")


def test_reference_errors(device, capsys):
    y, s = np.array([0, 1, 1, 0]), np.array([0.1, 0.9, 0.4, 0.3], dtype=np.float32)
    with pytest.raises(ValueError):
        M.binary_metrics(np.ones(4), s)                          # one class
    with pytest.raises(ValueError):
        M.binary_metrics(np.array([0, 1, 2, 0]), s)              # not binary
    with pytest.raises(ValueError):
        M.binary_metrics(y, np.array([0.1, np.nan, 0.4, 0.3], dtype=np.float32))
    with pytest.raises(ValueError):
        M.binary_metrics_multi_target_nan(np.array([[0], [1], [3], [-1]]), s[:, None])
    with pytest.raises(ZeroDivisionError):
        M.binary_metrics_multi_target_nan(np.array([[0, -1], [0, 1], [-1, 1], [0, 1]]), np.stack([s, s], 1))
    assert capsys.readouterr().out.count("Skipped target") == 2
    with pytest.raises(ZeroDivisionError):
        M.cal_ci(np.full(5, 2.0), np.arange(5.0))
    with pytest.raises(ZeroDivisionError):
        M.regression_metrics(np.full(5, 2.0), np.arange(5.0))
    with pytest.raises(ValueError):
        M.regression_metrics(np.arange(5.0), np.array([0, 1, np.inf, 3, 4.0]))
    with pytest.raises(Exception, match="n actives == 0"):
        M.enrichment_factor_single(np.array([0, 0, -1, 0]), s)
    with pytest.raises(ValueError):
        M.multi_class_metrics(np.array([0, 1, 5, 2]), np.eye(4, dtype=np.float32))
    # a task skipped by the reference is reported once
    y2 = np.array([[0, 0, 1], [1, 0, 1], [0, 0, 0], [1, -1, 1]])
    M.binary_metrics_multi_target_nan(y2, np.stack([s, s, s], 1))
    assert capsys.readouterr().out.count("Skipped target") == 1
