"""The evaluation metrics of the reference's trainers (``src_1gp/metrics.py``, ``multi_class_metrics`` of ``src_2gi_ddi/utils.py``),
scored by HIP kernels (``csrc/metrics.hip``) instead of sklearn and ``cal_ci``'s O(n^2) Python loop.

The names, signatures, default arguments, dict keys and key order are the reference's, so a trainer only changes its import
(``from glam_amd.metrics import ...``).  Inputs may be numpy arrays (what the trainers pass), CPU tensors or tensors on the current HIP
device; host inputs are copied to the device once.  Every call is two launches (the pair counts, then a one-block finish) plus the
dtype casts of its inputs, and one read-back of a 256-byte result record; the values come back as Python floats.  There is no CPU
fallback: without a HIP device every call raises ``GlamHipError``.

Scores and regression targets keep their dtype on the device (float32 or float64; integer and bool keys go to float64, half precision
to float32), so fp64 targets that would collide in fp32 stay distinct.  Labels may be int, float or bool.  Conventions that differ from
the reference only where its result is undefined or it does not check:
  - BEDROC and EF rank tied scores in index order (the reference's unstable ``np.argsort`` leaves that order undefined);
  - a label outside {0, 1} ({-1, 0, 1} for ``binary_metrics_multi_target_nan`` and ``enrichment_factor_single``, -1 = missing), a
    non-finite score, or a multi-class label / prediction outside [0, n_class) raises ``ValueError``;
  - at most 2^31 - 2 samples per task (the kernels count in int32)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GlamHipError

_REGRESSION_DATASETS = ['esol', 'freesolv', 'lipophilicity', 'physprop_perturb']     # dataset_names["r"], src_1gp/dataset.py:28
_EF_FRACTIONS = (0.001, 0.005, 0.01, 0.02, 0.05)
_SKIP_MESSAGE = 'Skipped target, cause AUC is only defined when there is at least one positive data.'
_MAX_N = 2 ** 31 - 1


# ---- plumbing ------------------------------------------------------------------------------------------------------------------

def _device():
    if not torch.cuda.is_available():
        raise GlamHipError("glam_amd.metrics runs on an MI355X HIP device only; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(x, dev, what):
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        a = np.asarray(x)
        if a.dtype == object or a.dtype.kind not in "biuf":
            raise ValueError(f"{what}: numeric input expected, got dtype {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.is_cuda:
        _lib.require_device(t)
    else:
        t = t.to(dev, non_blocking=False)
    return t


def _key(t):
    """Scores / targets: float32 and float64 stay; half precision widens to float32, integers and bool to float64 (exact)."""
    if t.dtype in (torch.float32, torch.float64):
        return t.contiguous()
    return t.to(torch.float32 if t.dtype in (torch.float16, torch.bfloat16) else torch.float64).contiguous()


def _label_dtype(*ts):
    wide = any(t is not None and t.dtype in (torch.float64, torch.int64) for t in ts)
    return torch.float64 if wide else torch.float32


def _code(dtype):
    return 1 if dtype == torch.float64 else 0


def _record(rec):
    host = rec.cpu()
    return host[:16].tolist(), host[16:].view(torch.float64).tolist()


def _check_n(n, what):
    if n >= _MAX_N:
        raise ValueError(f"{what}: {n} samples per task; the device counts hold at most 2^31 - 2")


def _binary(y_true, y_score, y_pred, masked, pred_mode, threshold=0.5, alpha=20.0, fractions=(), multi_task=False, negate=False):
    """One call of glam_metrics_binary; returns (int fields, float fields, n rows)."""
    dev = _device()
    lib = _lib.api()
    yt, ys = _to_device(y_true, dev, "y_true"), _to_device(y_score, dev, "y_score")
    yp = _to_device(y_pred, dev, "y_pred") if y_pred is not None else None
    if multi_task:
        if yt.dim() != 2:
            raise IndexError("tuple index out of range")
    else:
        yt, ys = yt.reshape(-1), ys.reshape(-1)
        yp = yp.reshape(-1) if yp is not None else None
    if yt.shape != ys.shape or (yp is not None and yp.shape != yt.shape):
        raise ValueError(f"Found input variables with inconsistent shapes: {tuple(yt.shape)}, {tuple(ys.shape)}"
                         + (f", {tuple(yp.shape)}" if yp is not None else ""))
    n, tasks = (yt.shape[0], yt.shape[1]) if multi_task else (yt.shape[0], 1)
    _check_n(n, "metrics")
    score = _key(ys)
    if negate:
        score = -score
    ldt = _label_dtype(yt, yp)
    label = yt.to(ldt).contiguous()
    pred = yp.to(ldt).contiguous() if yp is not None else None
    ws = torch.empty(max(lib.glam_metrics_workspace_bytes(n, max(tasks, 1), 0), 1), dtype=torch.uint8, device=dev)
    rec = torch.empty(32, dtype=torch.int64, device=dev)
    pct = (ctypes.c_double * 5)(*fractions)
    lib.glam_metrics_binary(_lib.ptr(score), _lib.ptr(label), _lib.ptr(pred), _code(score.dtype), _code(ldt), n, tasks, int(masked),
                            0 if pred is not None else pred_mode, float(threshold), float(alpha), pct, len(fractions), _lib.ptr(ws), ws.numel(),
                            _lib.ptr(rec), _lib.stream())
    iv, dv = _record(rec)
    return iv, dv, n


def _div(a, b):
    """sklearn's zero_division=0 (the default "warn" returns 0.0)."""
    return a / b if b else 0.0


def _single_task(iv, dv, bad_msg="Input contains NaN, infinity or a label outside {0, 1}."):
    if iv[2]:
        raise ValueError(bad_msg)
    if iv[3] == 0 or iv[4] == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")


# ---- the reference's functions -------------------------------------------------------------------------------------------------

def auto_metrics(dataset: str):
    metrics = ['valauc', 'auc']
    if dataset in _REGRESSION_DATASETS + ['physprop_perturb']:
        metrics = ['valr2', 'r2']
    return metrics


def binary_metrics(y_true, y_score, y_pred=None, threshod=0.5):
    """ROC-AUC, PR-AUC, accuracy and macro precision / recall / F1 of one binary task (prediction: score >= threshold)."""
    iv, dv, _ = _binary(y_true, y_score, y_pred, masked=False, pred_mode=1, threshold=threshod)
    _single_task(iv, dv)
    tp, fp, tn, fn = iv[5:9]
    precision = (_div(tn, tn + fn) + _div(tp, tp + fp)) / 2
    recall = (_div(tn, tn + fp) + _div(tp, tp + fn)) / 2
    f1 = (_div(2.0 * tn, 2 * tn + fn + fp) + _div(2.0 * tp, 2 * tp + fp + fn)) / 2
    return {'auc': dv[0], 'prauc': dv[4], 'acc': dv[1], 'precision': precision, 'recall': recall, 'f1': f1}


def binary_metrics_multi_target_nan(y_true, y_score, y_pred=None, nan_fill=-1, threshod=0.5):
    """``(N, T)`` labels (-1 = missing) and scores: per-task AUC, accuracy, precision, recall (binary averaging), meaned over the tasks
    that have both classes; a task without one of them is skipped with the reference's message."""
    iv, dv, _ = _binary(y_true, y_score, y_pred, masked=True, pred_mode=1, threshold=threshod, multi_task=True)
    if iv[2]:
        raise ValueError("Input contains NaN, infinity or a label outside {-1, 0, 1}.")
    for _ in range(iv[1]):
        print(_SKIP_MESSAGE)
    kept = iv[0] if nan_fill == -1 else 0
    if kept == 0:
        raise ZeroDivisionError("division by zero")
    return {'auc': dv[0] / kept, 'acc': dv[1] / kept, 'precision': dv[2] / kept, 'recall': dv[3] / kept}


def _regression(y_true, y_pred):
    dev = _device()
    lib = _lib.api()
    y, f = _to_device(y_true, dev, "y_true").reshape(-1), _to_device(y_pred, dev, "y_pred").reshape(-1)
    if y.shape != f.shape:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{y.numel()}, {f.numel()}]")
    n = y.numel()
    _check_n(n, "regression metrics")
    dt = torch.promote_types(_key(y[:0]).dtype, _key(f[:0]).dtype)
    y, f = y.to(dt).contiguous(), f.to(dt).contiguous()
    ws = torch.empty(max(lib.glam_metrics_workspace_bytes(n, 1, 0), 1), dtype=torch.uint8, device=dev)
    rec = torch.empty(32, dtype=torch.int64, device=dev)
    lib.glam_metrics_regression(_lib.ptr(y), _lib.ptr(f), _code(dt), n, _lib.ptr(ws), ws.numel(), _lib.ptr(rec), _lib.stream())
    iv, dv = _record(rec)
    return iv, dv, n


def _ci(iv):
    pairs, less, equal = iv[0], iv[1], iv[2]
    if pairs == 0:
        raise ZeroDivisionError("float division by zero")
    return (less + 0.5 * equal) / pairs


def cal_ci(y, f):
    """Concordance index: over the pairs with y_i > y_j, the share with f_i > f_j (ties in f count half)."""
    iv, _, _ = _regression(y, f)
    return _ci(iv)


def regression_metrics(y_true, y_pred):
    iv, dv, n = _regression(y_true, y_pred)
    ci = _ci(iv)
    if iv[3]:
        raise ValueError("Input contains NaN or infinity.")
    mse = dv[0] / n
    rmse = mse ** 0.5
    ss_res, ss_tot = dv[0], dv[1]
    r2 = 1.0 - ss_res / ss_tot if ss_tot != 0 else (1.0 if ss_res == 0 else 0.0)
    return {'ci': ci, 'mse': mse, 'rmse': rmse, 'r2': r2}


def _bedroc_finish(s, n, big_n, alpha):
    """The reference's constants (skchem's BEDROC) around the device sum s = sum over the positives of exp(-alpha rank / big_n)."""
    with np.errstate(all="ignore"):
        r_a = np.int64(n) / big_n
        rand_sum = r_a * (1 - np.exp(-alpha)) / (np.exp(alpha / big_n) - 1)
        fac = r_a * np.sinh(alpha / 2) / (np.cosh(alpha / 2) - np.cosh(alpha / 2 - alpha * r_a))
        cte = 1 / (1 - np.exp(alpha * (1 - r_a)))
        return float(np.float64(s) * fac / rand_sum + cte)


def bedroc_score(y_true, y_score, decreasing=True, alpha=20.0):
    """BEDROC of labels in {0, 1} (ties of equal scores in index order)."""
    iv, dv, n = _binary(y_true, y_score, None, masked=False, pred_mode=1, alpha=alpha, negate=not decreasing)
    if iv[2]:
        raise ValueError("Input contains NaN, infinity or a label outside {0, 1}.")
    return _bedroc_finish(dv[5], iv[3], n, alpha)


def _ef(hits, n_actives, fraction):
    if n_actives > 0:
        return float(hits) / np.int64(n_actives) / fraction
    raise Exception('n actives == 0')


def enrichment_factor_single(y_true, y_score, threshold=0.005):
    """Actives among the top int(n * threshold) scores (labels of -1 are missing) over the rate at random."""
    iv, _, _ = _binary(y_true, y_score, None, masked=True, pred_mode=1, fractions=(threshold,))
    if iv[2]:
        raise ValueError("Input contains NaN, infinity or a label outside {-1, 0, 1}.")
    return float(_ef(iv[9], iv[3], threshold))


def screening_metrics(y_true, y_score, y_pred=None, threshod=0.5):
    """AUC, accuracy, precision, recall (prediction: score > threshold), BEDROC (alpha 20) and EF at 0.1 % ... 5 %."""
    iv, dv, n = _binary(y_true, y_score, y_pred, masked=False, pred_mode=2, threshold=threshod, alpha=20.0, fractions=_EF_FRACTIONS)
    _single_task(iv, dv)
    P = iv[3]
    ef = [float(_ef(iv[9 + k], P, p)) for k, p in enumerate(_EF_FRACTIONS)]
    return {'auc': dv[0], 'acc': dv[1], 'precision': dv[2], 'recall': dv[3], 'bedroc': _bedroc_finish(dv[5], P, n, 20.0),
            'ef_001': ef[0], 'ef_005': ef[1], 'ef_01': ef[2], 'ef_02': ef[3], 'ef_05': ef[4], }


def multi_class_metrics(y_true, y_score, y_pred=None):
    """``y_score (N, n_class)``, ``y_true (N,)`` in [0, n_class): accuracy and macro precision / recall / F1 over the classes that occur
    in the labels or the predictions (prediction: the first argmax of each row)."""
    dev = _device()
    lib = _lib.api()
    yt = _to_device(y_true, dev, "y_true").reshape(-1)
    ys = _to_device(y_score, dev, "y_score")
    yp = _to_device(y_pred, dev, "y_pred").reshape(-1) if y_pred is not None else None
    if ys.dim() != 2 or ys.shape[0] != yt.shape[0] or (yp is not None and yp.shape != yt.shape):
        raise ValueError(f"Found input variables with inconsistent shapes: {tuple(yt.shape)}, {tuple(ys.shape)}")
    n, n_class = ys.shape
    _check_n(n, "multi-class metrics")
    if n == 0:
        raise ValueError("Found array with 0 sample(s)")
    score = _key(ys)
    ldt = _label_dtype(yt, yp)
    label = yt.to(ldt).contiguous()
    pred = yp.to(ldt).contiguous() if yp is not None else None
    ws_bytes = lib.glam_metrics_workspace_bytes(n, 1, n_class)
    if ws_bytes == 0:
        raise ValueError(f"multi_class_metrics: {n_class} classes; the device form supports 1 to 4096")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rec = torch.empty(32, dtype=torch.int64, device=dev)
    lib.glam_metrics_multiclass(_lib.ptr(score), _lib.ptr(label), _lib.ptr(pred), _code(score.dtype), _code(ldt), n, n_class,
                                _lib.ptr(ws), ws.numel(), _lib.ptr(rec), _lib.stream())
    iv, dv = _record(rec)
    if iv[2]:
        raise ValueError(f"labels and predictions must be integers in [0, {n_class})")
    seen = iv[1]
    return {'acc': iv[0] / n, 'precision': dv[0] / seen, 'recall': dv[1] / seen, 'f1': dv[2] / seen}


# ---- ensembles: thin torch plumbing over the tensors they receive (src_1gp/metrics.py:171-205) -----------------------------------

def blend_regression(outputs: list, opt='mean', return_pred=False):
    ls, pls = [], []
    for _l, _pl in outputs:
        ls.append(_l)
        pls.append(_pl)
    blendd_l = ls[0]
    blendd_pl = torch.stack(pls, dim=1).mean(dim=1) if opt == 'mean' else None
    if return_pred is True:
        return blendd_pl
    return regression_metrics(blendd_l, y_pred=blendd_pl)


def blend_binary_classification(outputs: list, opt='vote', metrics_fn=binary_metrics):
    ls, pls, ss = [], [], []
    for _l, _pl, _s in outputs:
        ls.append(_l)
        pls.append(_pl)
        ss.append(_s)
    blendd_l = ls[0]
    blendd_pl = torch.stack(pls, dim=1).mode(dim=1)[0] if opt == 'vote' else None
    blendd_ss = torch.stack(ss, dim=1).mean(dim=1)
    return metrics_fn(blendd_l, y_score=blendd_ss, y_pred=blendd_pl)


def blend_binary_classification_mt(outputs: list, opt='vote', metrics_fn=binary_metrics):
    ls, ss = [], []
    for _s, _l in outputs:
        ls.append(_l)
        ss.append(_s)
    blendd_l = ls[0]
    blendd_ss = torch.stack(ss, dim=2).mean(dim=2)
    return metrics_fn(blendd_l, y_score=blendd_ss)
