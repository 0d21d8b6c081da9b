"""The class table (``ops.pair_head_classes``, csrc/pairhead.hip) restated in torch (a helper, not a test module): the factored head's
logits (``pair_head_restated.factored``), then

    cls  = argmax_o logits[..., o]              (torch.argmax: a NaN is the largest, of equal values the smallest index)
    logp = log_softmax(logits)[..., cls]        (the called class's)
    sel  = log_softmax(logits)[..., classes]    (in the order given, duplicates allowed)

in whatever precision the inputs come in.  ``WRONG``: five restatements someone could have written instead; the host test shows that the
comparison sees each of them on inputs built for it."""
import torch

from tests import pair_head_restated as H

WRONG = ("last_on_ties", "softmax_over_selected", "logp_of_class_0", "sel_raw_logits", "nan_smallest")


def from_logits(logits, classes=(), wrong=None):
    """``(cls int64 [R, Cs], logp [R, Cs], sel [R, Cs, S], logits)`` of a ``[R, Cs, out_dim]`` logits table."""
    classes = [int(c) for c in classes]
    n = logits.size(-1)
    if wrong == "last_on_ties":
        cls = n - 1 - torch.argmax(logits.flip(-1), -1)
    else:
        if wrong == "nan_smallest":              # (what a maximum by fmax, which drops a NaN operand, makes of it)
            logits = torch.nan_to_num(logits, nan=torch.finfo(logits.dtype).min)
        cls = torch.argmax(logits, -1)
    logsm = torch.log_softmax(logits, -1)
    index = torch.zeros_like(cls) if wrong == "logp_of_class_0" else cls
    logp = logsm.gather(-1, index.unsqueeze(-1)).squeeze(-1)
    if wrong == "sel_raw_logits":
        sel = logits[..., classes]
    elif wrong == "softmax_over_selected":
        sel = torch.log_softmax(logits[..., classes], -1)
    else:
        sel = logsm[..., classes]
    return cls, logp, sel, logits


def classes(flat_a, flat_b, f, W0, b0, w1, b1, act="none", slope=0.0, classes=(), wrong=None):
    """The four outputs of the class table on the operands of ``pair_head_restated.factored``, in the inputs' dtype."""
    return from_logits(H.factored(flat_a, flat_b, f, W0, b0, w1, b1, act=act, slope=slope), classes, wrong)


def listed(flat_a, flat_b, f, W0, b0, w1, b1, act="none", classes=()):
    """The same from the listed head of the oracle's ``linear_block`` assembly (``pair_head_restated.listed``)."""
    return from_logits(H.listed(flat_a, flat_b, f, W0, b0, w1, b1, act=act), classes)


def with_tie(t, lo, hi, bias=10.0):
    """``t`` (the tuple of ``pair_head_restated.inputs``) with row ``hi`` of ``lin1`` a copy of row ``lo`` and both biases ``bias`` — the two
    classes tie EXACTLY at every pair, far above the others."""
    a, b, f, W0, b0, w1, b1 = [None if x is None else x.clone() for x in t]
    w1[hi] = w1[lo]
    b1[lo] = b1[hi] = bias
    return a, b, f, W0, b0, w1, b1


def with_nan(t, i, j, k=0):
    """``t`` with ``f[i, j, k]`` NaN: every logit of that one pair is NaN."""
    a, b, f, W0, b0, w1, b1 = [None if x is None else x.clone() for x in t]
    f[i, j, k] = float("nan")
    return a, b, f, W0, b0, w1, b1


def with_nan_class(t, o):
    """``t`` with ``b1[o]`` NaN: logit ``o`` of EVERY pair is NaN, the others are numbers."""
    a, b, f, W0, b0, w1, b1 = [None if x is None else x.clone() for x in t]
    b1[o] = float("nan")
    return a, b, f, W0, b0, w1, b1
