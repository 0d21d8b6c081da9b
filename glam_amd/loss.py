"""The loss of the training step, mirroring the reference's ``loss.py`` (``get_loss``, ``src_1gp/loss.py:40-59``).

Every criterion a training loop of the reference's search draws computes its value and un-normalised gradient in ONE HIP launch and
back-propagates with one scale launch (``glam_loss_bwd``); through torch the same is 5-12 small launches per step.

* Elementwise means (``glam_loss_fwd``): ``'mse'`` (``MSELoss``), ``'bcel'`` (``BCEWithLogitsLoss``), ``'mae'`` (``L1Loss``),
  ``'huber'`` / ``'smae'`` (``SmoothL1Loss``), ``'bce'`` (``BCELoss``).  ``MaskedBCEWithLogitsLoss`` (``'bcel_masked'``) is the
  classification trainer's ``criterion(y_score[y_true >= 0], y_true[y_true >= 0])`` (labels of -1 are missing, ``dataset.py:138``)
  without the boolean indexing, which a hipGraph cannot capture.
* The cross-entropy family over logits ``[B, C]`` and int64 labels (``glam_ce_loss_fwd``): ``'ce'`` (``CrossEntropyLoss``, also with
  a class ``weight``: the screening trainer's ``'wce'``, ``src_2gi_dti_scr/trainer.py:265-267``) and ``'focal'`` (``FocalLoss``,
  ``src_1gp/loss.py:3-16``).  Deliberate difference: a label outside ``[0, C)`` that is not ``ignore_index`` makes the loss nan
  where torch raises a device-side assert.

The modules subclass their torch classes and take the HIP route for ``reduction='mean'`` on float32 HIP tensors (CE family: a 2-D
input, int64 class labels, no label smoothing, ``C <= glam_ce_loss_max_classes()``; focal: ``gamma`` 0 or >= 1); every other form
(``reduction='none'``, probability targets, other dtypes, ...) runs the torch parent's ``forward`` unchanged.  ``'wce'`` resolves to
None, as in ``src_2gi_dti_scr/utils.py:89-92`` (the trainer builds it); ``'mtce'``, ``'bcen'``, ``'bceln'``, ``'kl'``, ``'hinge'`` and
``'nll'`` are torch's, as in the reference."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import GlamHipError, f32c, ptr, require_device

_TICKETS: dict = {}     # device index -> persistent u32[544] ticket buffer (zeroed once, re-armed by every launch)
_WS: dict = {}          # device index -> the block partials of a multi-block launch (overwritten by every launch)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _ticket(dev):
    t = _TICKETS.get(dev.index)
    if t is None:
        t = _TICKETS[dev.index] = torch.zeros(544, dtype=torch.int32, device=dev)
    return t


def _workspace(dev, lib):
    ws = _WS.get(dev.index)
    if ws is None:
        ws = torch.empty(lib.glam_loss_workspace_bytes(), dtype=torch.uint8, device=dev)
        if not torch.cuda.is_current_stream_capturing():     # (born in a capture it lives in that graph's pool: not kept)
            _WS[dev.index] = ws
    return ws


def _stream(dev):
    """``hipStream_t`` of torch's current stream on ``dev`` (the raw accessor: ``torch.cuda.current_stream`` costs ~15 us)."""
    if _raw_stream is not None:
        return _raw_stream(dev.index)
    return torch.cuda.current_stream(dev).cuda_stream


class _MeanLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, kind, masked):
        require_device(pred, target)
        if pred.shape != target.shape:
            raise GlamHipError(f"loss: prediction {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
        # classification labels arrive as a LongTensor (src_1gp/dataset.py:139; the reference casts with .float() at the call site,
        # trainer.py:244-245): cast here so that criterion(y_score, y_true) is the drop-in (the mask y >= 0 survives the cast)
        if target.dtype != torch.float32:
            target = target.to(torch.float32)
        p, t = f32c(pred, "prediction"), f32c(target, "target")
        lib, dev, n = _lib.api(), pred.device, pred.numel()
        out = torch.empty(2, dtype=torch.float32, device=dev)             # loss | 1 / count
        grad = torch.empty_like(p)
        ws = _workspace(dev, lib) if n > 1024 else None
        lib.glam_loss_fwd(ptr(p), ptr(t), n, kind, int(masked), out.data_ptr(), out.data_ptr() + 4, ptr(grad), ptr(ws),
                          ws.numel() if ws is not None else 0, ptr(_ticket(dev)) if n > 1024 else None, _stream(dev))
        ctx.save_for_backward(grad, out)
        ctx.shape = pred.shape
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_up):
        return _scale_back(ctx, g_up), None, None, None


def _scale_back(ctx, g_up):
    """d_input = grad * g_up / denominator (``glam_loss_bwd``) from the (grad, [loss | 1 / denominator]) the forward saved."""
    grad, out = ctx.saved_tensors
    lib, dev = _lib.api(), grad.device
    g_up = f32c(g_up.reshape(1), "loss gradient")
    d_pred = torch.empty_like(grad)
    lib.glam_loss_bwd(ptr(grad), out.data_ptr() + 4, ptr(g_up), grad.numel(), ptr(d_pred), _stream(dev))
    return d_pred.view(ctx.shape)


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, weight, ignore_index, focal, alpha, gamma):
        require_device(x, y, weight)
        if x.dim() != 2 or y.dim() != 1 or y.size(0) != x.size(0) or y.dtype != torch.int64:
            raise GlamHipError(f"cross entropy: logits [B, C] and int64 labels [B] expected, got {tuple(x.shape)} and "
                               f"{tuple(y.shape)} {y.dtype}")
        B, C = x.shape
        lib, dev = _lib.api(), x.device
        if B < 1 or not 1 <= C <= _max_classes():
            raise GlamHipError(f"cross entropy: B = {B}, C = {C} outside the kernel's range (B >= 1, 1 <= C <= {_max_classes()})")
        x, y = f32c(x, "logits"), y.contiguous()
        if weight is not None:
            weight = f32c(weight, "class weight")
            if weight.shape != (C,):
                raise GlamHipError(f"cross entropy: weight {tuple(weight.shape)} for {C} classes")
        out = torch.empty(2, dtype=torch.float32, device=dev)             # loss | 1 / denominator
        grad = torch.empty_like(x)
        ws = _workspace(dev, lib)
        lib.glam_ce_loss_fwd(ptr(x), ptr(y), ptr(weight), B, C, int(ignore_index), int(focal), float(alpha), float(gamma),
                             out.data_ptr(), out.data_ptr() + 4, ptr(grad), ptr(ws), ws.numel(), ptr(_ticket(dev)), _stream(dev))
        ctx.save_for_backward(grad, out)
        ctx.shape = x.shape
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_up):
        return _scale_back(ctx, g_up), None, None, None, None, None, None


def mse_loss(pred, target):
    """``F.mse_loss(pred, target)`` (mean)."""
    return _MeanLoss.apply(pred, target, 0, False)


def bce_with_logits(pred, target, masked=False):
    """``F.binary_cross_entropy_with_logits(pred, target)`` (mean); ``masked``: over the elements with ``target >= 0`` only."""
    return _MeanLoss.apply(pred, target, 1, masked)


def l1_loss(pred, target):
    """``F.l1_loss(pred, target)`` (mean)."""
    return _MeanLoss.apply(pred, target, 2, False)


def smooth_l1_loss(pred, target):
    """``F.smooth_l1_loss(pred, target)`` (mean, beta = 1)."""
    return _MeanLoss.apply(pred, target, 3, False)


def bce_loss(pred, target):
    """``F.binary_cross_entropy(pred, target)`` (mean; ``pred`` holds probabilities)."""
    return _MeanLoss.apply(pred, target, 4, False)


def cross_entropy(x, y, weight=None, ignore_index=-100):
    """``F.cross_entropy(x, y, weight, ignore_index=ignore_index)`` (mean) for logits ``[B, C]`` and int64 labels ``[B]``; a label
    outside ``[0, C)`` that is not ``ignore_index`` gives nan."""
    return _CrossEntropy.apply(x, y, weight, ignore_index, 0, 0.0, 0.0)


def focal_loss(x, y, alpha=0.25, gamma=2):
    """The reference's ``FocalLoss(alpha, gamma)(x, y)`` (``src_1gp/loss.py:3-16``): ``(alpha (1 - pt)^gamma ce).mean()`` with the
    unweighted per-row ``ce`` (ignore_index -100) and ``pt = exp(-ce)``; ``gamma`` 0 or >= 1."""
    if not (gamma == 0 or gamma >= 1):
        raise GlamHipError(f"focal_loss: gamma = {gamma}; the HIP route takes gamma = 0 or gamma >= 1")
    return _CrossEntropy.apply(x, y, None, -100, 1, alpha, gamma)


def _f32_hip(*ts):
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


def _elementwise_ok(mod, input, target):
    return (mod.reduction == "mean" and isinstance(input, torch.Tensor) and isinstance(target, torch.Tensor)
            and _f32_hip(input, target) and input.shape == target.shape and 0 < input.numel() < 2 ** 31)


def _max_classes():
    return _lib.api().glam_ce_loss_max_classes()


def _class_logits_ok(input, target):
    """Logits [B, C] on the device with int64 class labels [B] in the kernel's range (anything else: the torch parent)."""
    return (isinstance(input, torch.Tensor) and isinstance(target, torch.Tensor) and _f32_hip(input) and input.dim() == 2
            and target.dtype == torch.int64 and target.is_cuda and target.shape == input.shape[:1] and input.size(0) >= 1
            and 1 <= input.size(1) <= _max_classes() and input.numel() < 2 ** 31)


class MSELoss(torch.nn.Module):
    def forward(self, input, target):
        return mse_loss(input, target)


class BCEWithLogitsLoss(torch.nn.Module):
    def forward(self, input, target):
        return bce_with_logits(input, target)


class MaskedBCEWithLogitsLoss(torch.nn.Module):
    """``criterion(y_score[y_true >= 0], y_true[y_true >= 0].float())`` of ``trainer.py:244-245`` as ``criterion(y_score, y_true)``."""

    def forward(self, input, target):
        return bce_with_logits(input, target, masked=True)


class L1Loss(torch.nn.L1Loss):
    """``nn.L1Loss`` ('mae'); the mean over float32 HIP tensors of one shape on the HIP launch."""

    def forward(self, input, target):
        return l1_loss(input, target) if _elementwise_ok(self, input, target) else super().forward(input, target)


class SmoothL1Loss(torch.nn.SmoothL1Loss):
    """``nn.SmoothL1Loss`` ('huber', 'smae'); the mean with ``beta = 1`` over float32 HIP tensors of one shape on the HIP launch."""

    def forward(self, input, target):
        if self.beta == 1.0 and _elementwise_ok(self, input, target):
            return smooth_l1_loss(input, target)
        return super().forward(input, target)


class BCELoss(torch.nn.BCELoss):
    """``nn.BCELoss`` ('bce', ``TrainerBinary``'s sigmoid + BCELoss); the unweighted mean over float32 HIP tensors on the HIP launch."""

    def forward(self, input, target):
        if self.weight is None and _elementwise_ok(self, input, target):
            return bce_loss(input, target)
        return super().forward(input, target)


class CrossEntropyLoss(torch.nn.CrossEntropyLoss):
    """``nn.CrossEntropyLoss`` ('ce'; with ``weight=train_dataset.weight`` the screening trainer's 'wce'): the mean over logits
    ``[B, C]`` with int64 class labels, optionally class-weighted, with ``ignore_index``, on one HIP launch."""

    def forward(self, input, target):
        w = self.weight
        if (self.reduction == "mean" and self.label_smoothing == 0.0 and _class_logits_ok(input, target)
                and (w is None or (_f32_hip(w) and w.shape == input.shape[1:]))):
            return cross_entropy(input, target, w, self.ignore_index)
        return super().forward(input, target)


class FocalLoss(torch.nn.Module):
    """The reference's ``FocalLoss(alpha=0.25, gamma=2)`` (``src_1gp/loss.py:3-16``), same attributes; logits ``[B, C]`` with int64
    labels and ``gamma`` 0 or >= 1 on one HIP launch, anything else through the reference's formula on torch."""

    def __init__(self, alpha=0.25, gamma=2):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma

    def forward(self, outputs, targets):
        if (self.gamma == 0 or self.gamma >= 1) and _class_logits_ok(outputs, targets):
            return focal_loss(outputs, targets, self.alpha, self.gamma)
        ce_loss = torch.nn.functional.cross_entropy(outputs, targets, reduction='none')
        pt = torch.exp(-ce_loss)
        return (self.alpha * (1 - pt) ** self.gamma * ce_loss).mean()


class MultiTargetCrossEntropy(torch.nn.Module):
    """The reference's ``MultiTargetCrossEntropy`` (``src_1gp/loss.py:19-36``) on torch ops: input ``(N, T, C)``, target ``(N, T)``;
    log-softmax over ``C_dim``, then the NLL mean.  No search path draws it."""

    def __init__(self, C_dim=2):
        super().__init__()
        self.log_softmax = torch.nn.LogSoftmax(dim=C_dim)
        self.nll_loss = torch.nn.NLLLoss()

    def forward(self, input, target):
        assert input.shape[0] == target.shape[0]
        assert input.shape[1] == target.shape[1]
        return self.nll_loss(self.log_softmax(input), target)


def get_loss(loss_str):
    """``loss.py:40-59`` with the same names (and ``'bcel_masked'``); ``'wce'`` is None, as in ``src_2gi_dti_scr/utils.py:89-92``:
    the screening trainer builds ``CrossEntropyLoss(weight=train_dataset.weight)`` itself."""
    if loss_str == 'wce':
        return None
    d = {
        'mse': MSELoss, 'bcel': BCEWithLogitsLoss, 'bcel_masked': MaskedBCEWithLogitsLoss,
        'mae': L1Loss, 'huber': SmoothL1Loss, 'smae': SmoothL1Loss, 'bce': BCELoss, 'ce': CrossEntropyLoss,
        'focal': lambda: FocalLoss(alpha=0.25), 'mtce': MultiTargetCrossEntropy,
        'bcen': lambda: torch.nn.BCELoss(reduction="none"), 'bceln': lambda: torch.nn.BCEWithLogitsLoss(reduction="none"),
        'kl': torch.nn.KLDivLoss, 'hinge': torch.nn.HingeEmbeddingLoss, 'nll': torch.nn.NLLLoss,
    }
    if loss_str not in d:
        raise ValueError('loss not found')
    return d[loss_str]()
