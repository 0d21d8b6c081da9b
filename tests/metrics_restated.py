"""An independent numpy restatement of the reference's evaluation metrics in the count form of glam_amd.metrics, shared
by tests/test_metrics_host.py and tests/test_gpu_metrics.py.  Per-sample counts come from sorted searches here, not from the pair loop
of the kernels, so the two only agree when the count formulas do.  Ties rank in index order (the stable convention)."""
import json
import os

import numpy as np

from tests.conftest import GOLD

EF_FRACTIONS = (0.001, 0.005, 0.01, 0.02, 0.05)
KEYS = {
    "binary_metrics": ['auc', 'prauc', 'acc', 'precision', 'recall', 'f1'],
    "binary_metrics_multi_target_nan": ['auc', 'acc', 'precision', 'recall'],
    "regression_metrics": ['ci', 'mse', 'rmse', 'r2'],
    "screening_metrics": ['auc', 'acc', 'precision', 'recall', 'bedroc', 'ef_001', 'ef_005', 'ef_01', 'ef_02', 'ef_05'],
    "multi_class_metrics": ['acc', 'precision', 'recall', 'f1'],
}
SUM_KEYS = {'mse', 'rmse', 'r2'}          # fp64 sums, checked with the fp64-twin rule; every other value is a function of integer counts


def load_fixture(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, {k[3:]: z[k] for k in z.files if k.startswith("in.")}


def fixture_names():
    return sorted(f[:-4] for f in os.listdir(GOLD) if f.startswith("metrics_") and f.endswith(".npz"))


def counts(score, pos):
    """Per-sample counts over one task's valid samples: gt_all, gt_pos, eq_all, eq_pos, eq_before."""
    s = np.asarray(score)
    n = s.size
    srt = np.sort(s, kind="stable")
    left, right = np.searchsorted(srt, s, "left"), np.searchsorted(srt, s, "right")
    sp = np.sort(s[pos], kind="stable")
    lp, rp = np.searchsorted(sp, s, "left"), np.searchsorted(sp, s, "right")
    order = np.lexsort((np.arange(n), s))            # ascending score, ties in index order
    eq_before = np.empty(n, dtype=np.int64)
    eq_before[order] = np.arange(n) - left[order]
    return n - right, sp.size - rp, right - left, rp - lp, eq_before


def task_terms(score, label, thr_pred, alpha=20.0, fractions=(), big_n=None):
    """label: 0/1 over the valid samples; thr_pred: 0/1 predictions.  Returns the count-form metrics of one task."""
    pos = label == 1
    P, n = int(pos.sum()), label.size
    N = n - P
    gt_all, gt_pos, eq_all, eq_pos, eq_before = counts(score, pos)
    neg = ~pos
    out = dict(P=P, N=N)
    out["auc"] = (2 * int(gt_pos[neg].sum()) + int(eq_pos[neg].sum())) / (2.0 * P * N) if P and N else None
    rep = (eq_before == 0) & (eq_pos > 0)
    prec_ge = (gt_pos + eq_pos) / (gt_all + eq_all)
    prec_gt = np.where(gt_all > 0, gt_pos / np.maximum(gt_all, 1), 1.0)
    out["prauc"] = float(np.sum((eq_pos / max(P, 1) * (prec_ge + prec_gt) / 2)[rep]))
    rank = 1 + gt_all + eq_before
    out["bedroc_s"] = float(np.sum(np.exp(-alpha * rank[pos] / (big_n or n))))
    out["ef_hits"] = [int((rank[pos] <= int(n * p)).sum()) for p in fractions]
    pr = thr_pred.astype(bool)
    out["tp"], out["fp"] = int((pos & pr).sum()), int((neg & pr).sum())
    out["tn"], out["fn"] = int((neg & ~pr).sum()), int((pos & ~pr).sum())
    return out


def _div(a, b):
    return a / b if b else 0.0


def binary_metrics(y_true, y_score, y_pred=None, threshod=0.5):
    y, s = np.asarray(y_true).reshape(-1).astype(np.float64), np.asarray(y_score).reshape(-1)
    p = (s >= threshod) if y_pred is None else np.asarray(y_pred).reshape(-1)
    t = task_terms(s, y, p)
    tp, fp, tn, fn = t["tp"], t["fp"], t["tn"], t["fn"]
    return {'auc': t["auc"], 'prauc': t["prauc"], 'acc': (tp + tn) / y.size,
            'precision': (_div(tn, tn + fn) + _div(tp, tp + fp)) / 2, 'recall': (_div(tn, tn + fp) + _div(tp, tp + fn)) / 2,
            'f1': (_div(2.0 * tn, 2 * tn + fn + fp) + _div(2.0 * tp, 2 * tp + fp + fn)) / 2}


def binary_metrics_multi_target_nan(y_true, y_score, y_pred=None, threshod=0.5):
    """Returns (dict, skipped tasks)."""
    y, s = np.asarray(y_true).astype(np.float64), np.asarray(y_score)
    p = (s >= threshod) if y_pred is None else np.asarray(y_pred)
    lists, skipped = {k: [] for k in ('auc', 'acc', 'precision', 'recall')}, 0
    for i in range(y.shape[1]):
        v = y[:, i] >= 0
        t = task_terms(s[v, i], y[v, i], p[v, i])
        if not (t["P"] and t["N"]):
            skipped += 1
            continue
        lists['auc'].append(t["auc"])
        lists['acc'].append((t["tp"] + t["tn"]) / int(v.sum()))
        lists['precision'].append(_div(t["tp"], t["tp"] + t["fp"]))
        lists['recall'].append(t["tp"] / t["P"])
    if not lists['auc']:
        return None, skipped           # every task skipped: the reference divides by zero
    return {k: sum(v) / len(v) for k, v in lists.items()}, skipped


def ci_counts(y, f, chunk=2048):
    y, f = np.asarray(y), np.asarray(f)
    pairs = less = equal = 0
    for a in range(0, y.size, chunk):
        lt = y[None, :] < y[a:a + chunk, None]
        pairs += int(lt.sum())
        less += int((lt & (f[None, :] < f[a:a + chunk, None])).sum())
        equal += int((lt & (f[None, :] == f[a:a + chunk, None])).sum())
    return pairs, less, equal


def regression_metrics(y_true, y_pred):
    y, f = np.asarray(y_true).reshape(-1), np.asarray(y_pred).reshape(-1)
    pairs, less, equal = ci_counts(y, f)
    yd, fd = y.astype(np.float64), f.astype(np.float64)
    ss_res = float(np.sum((yd - fd) ** 2))
    ss_tot = float(np.sum((yd - yd.mean()) ** 2))
    mse = ss_res / y.size
    return {'ci': (less + 0.5 * equal) / pairs, 'mse': mse, 'rmse': mse ** 0.5, 'r2': 1.0 - ss_res / ss_tot}


def bedroc_finish(s, n, big_n, alpha=20.0):
    r_a = n / big_n
    rand_sum = r_a * (1 - np.exp(-alpha)) / (np.exp(alpha / big_n) - 1)
    fac = r_a * np.sinh(alpha / 2) / (np.cosh(alpha / 2) - np.cosh(alpha / 2 - alpha * r_a))
    cte = 1 / (1 - np.exp(alpha * (1 - r_a)))
    return float(s * fac / rand_sum + cte)


def screening_metrics(y_true, y_score, y_pred=None, threshod=0.5):
    y, s = np.asarray(y_true).reshape(-1).astype(np.float64), np.asarray(y_score).reshape(-1)
    p = (s > threshod) if y_pred is None else np.asarray(y_pred).reshape(-1)
    t = task_terms(s, y, p, fractions=EF_FRACTIONS)
    tp, fp, tn = t["tp"], t["fp"], t["tn"]
    d = {'auc': t["auc"], 'acc': (tp + tn) / y.size, 'precision': _div(tp, tp + fp), 'recall': tp / t["P"],
         'bedroc': bedroc_finish(t["bedroc_s"], t["P"], y.size)}
    for k, (name, frac) in enumerate(zip(('ef_001', 'ef_005', 'ef_01', 'ef_02', 'ef_05'), EF_FRACTIONS)):
        d[name] = float(t["ef_hits"][k]) / t["P"] / frac
    return d


def multi_class_metrics(y_true, y_score, y_pred=None):
    y = np.asarray(y_true).reshape(-1).astype(np.int64)
    p = np.argmax(np.asarray(y_score), axis=1) if y_pred is None else np.asarray(y_pred).reshape(-1).astype(np.int64)
    labels = np.union1d(y, p)
    prec, rec, f1 = [], [], []
    for c in labels:
        tp, tr, pr = int(((y == c) & (p == c)).sum()), int((y == c).sum()), int((p == c).sum())
        prec.append(_div(tp, pr))
        rec.append(_div(tp, tr))
        f1.append(_div(2.0 * tp, tr + pr))
    return {'acc': float((y == p).mean()), 'precision': float(np.mean(prec)), 'recall': float(np.mean(rec)), 'f1': float(np.mean(f1))}


def restate(fn_name, inputs):
    """The restatement of one fixture call; returns (dict, skipped tasks)."""
    if fn_name == "binary_metrics_multi_target_nan":
        return binary_metrics_multi_target_nan(**inputs)
    return globals()[fn_name](**inputs), 0


def check_against_reference(got, meta, what):
    """Count-form values within 1e-12 of the reference (BEDROC relative); fp64 sums within 8 |ref32 - ref64| + 1e-12 of ref64."""
    assert list(got) == meta["keys"], f"{what}: keys {list(got)} vs {meta['keys']}"
    for k, v in got.items():
        ref, ref64 = meta["ref"][k], meta["ref64"][k]
        assert type(v) is float, f"{what}[{k}]: {type(v)}"
        if k in SUM_KEYS:
            tol = 8 * abs(ref - ref64) + 1e-12
            assert abs(v - ref64) <= tol, f"{what}[{k}]: {v!r} vs ref64 {ref64!r} (tol {tol:.2e})"
        else:
            tol = 1e-12 * max(1.0, abs(ref)) if k in ('bedroc',) or k.startswith('ef_') else 1e-12
            assert abs(v - ref) <= tol, f"{what}[{k}]: {v!r} vs ref {ref!r}"
