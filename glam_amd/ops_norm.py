"""Column norms over a dense ``[N, C]`` tensor (csrc/colnorm.hip): ``torch.nn.BatchNorm1d`` in training and eval
mode, and PyG's graph LayerNorm with ``batch=None`` (one mean and one standard deviation over the whole tensor).  ``weight`` and
``bias`` are inputs of the autograd functions: a captured step runs the module on proxy leaves (``GraphedCallable._capture``)."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import GlamHipError, f32c, ptr, require_device, stream


def _workspace(lib, N, C, dev):
    """Partials of the two-launch forms: sized by the shape alone, allocated on the input's device at call time (the caching
    allocator keeps a capture's blocks alive)."""
    return torch.empty(max(1, lib.glam_colnorm_workspace_bytes(N, C) // 4), dtype=torch.float32, device=dev)


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, form=0, max_blocks=0):
        require_device(x, weight, bias, running_mean, running_var)
        x, weight, bias = f32c(x, "x"), f32c(weight, "weight"), f32c(bias, "bias")
        if x.dim() != 2 or weight.shape != (x.size(1),) or bias.shape != weight.shape or running_mean.shape != weight.shape \
                or running_var.shape != weight.shape:
            raise GlamHipError(f"batch_norm: x {tuple(x.shape)}, weight {tuple(weight.shape)}, running_mean {tuple(running_mean.shape)}")
        if running_mean.dtype != torch.float32 or running_var.dtype != torch.float32 or not (running_mean.is_contiguous()
                                                                                              and running_var.is_contiguous()):
            raise GlamHipError("batch_norm: the running statistics must be contiguous float32 (they are updated in place)")
        N, C = x.shape
        lib, dev = _lib.api(), x.device
        y = torch.empty_like(x)
        mean, rstd = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
        if training:
            ws = _workspace(lib, N, C, dev)
            lib.glam_batch_norm_fwd(ptr(x), ptr(weight), ptr(bias), ptr(running_mean), ptr(running_var), N, C, float(momentum), float(eps),
                                    ptr(y), ptr(mean), ptr(rstd), ptr(ws), ws.numel() * 4, int(form), int(max_blocks), stream())
        else:
            lib.glam_batch_norm_eval_fwd(ptr(x), ptr(weight), ptr(bias), ptr(running_mean), ptr(running_var), N, C, float(eps), ptr(y),
                                         ptr(mean), ptr(rstd), int(max_blocks), stream())
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.cfg = (not training, int(form), int(max_blocks))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        evalm, form, max_blocks = ctx.cfg
        dy = f32c(dy, "dy")
        N, C = x.shape
        lib, dev = _lib.api(), x.device
        dx, dw, db = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(weight)
        ws = _workspace(lib, N, C, dev)
        lib.glam_batch_norm_bwd(ptr(x), ptr(dy), ptr(weight), ptr(mean), ptr(rstd), N, C, int(evalm), ptr(dx), ptr(dw), ptr(db), ptr(ws),
                                ws.numel() * 4, form, max_blocks, stream())
        return dx, dw, db, None, None, None, None, None, None, None


def batch_norm(x, weight, bias, running_mean, running_var, training, momentum, eps, form=0, max_blocks=0):
    """``torch.nn.functional.batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps)`` on a float32 ``[N, C]``:
    the running statistics are updated in place in training mode (``N >= 2``).  One launch each way for few rows, two for many
    (``form`` / ``max_blocks``: the C ABI's, for tests and measurements)."""
    return _BatchNorm.apply(x, weight, bias, running_mean, running_var, bool(training), momentum, eps, form, max_blocks)


class _LayerNormFlat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, form=0, max_blocks=0):
        require_device(x, weight, bias)
        x, weight, bias = f32c(x, "x"), f32c(weight, "weight"), f32c(bias, "bias")
        if x.dim() != 2 or weight.shape != (x.size(1),) or bias.shape != weight.shape:
            raise GlamHipError(f"layer_norm_flat: x {tuple(x.shape)}, weight {tuple(weight.shape)}, bias {tuple(bias.shape)}")
        N, C = x.shape
        lib, dev = _lib.api(), x.device
        y, stat = torch.empty_like(x), torch.empty(2, dtype=torch.float32, device=dev)
        ws = _workspace(lib, N, C, dev)
        lib.glam_layer_norm_flat_fwd(ptr(x), ptr(weight), ptr(bias), N, C, float(eps), ptr(y), ptr(stat), ptr(ws), ws.numel() * 4, int(form),
                                     int(max_blocks), stream())
        ctx.save_for_backward(x, weight, stat)
        ctx.cfg = (float(eps), int(form), int(max_blocks))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, stat = ctx.saved_tensors
        eps, form, max_blocks = ctx.cfg
        dy = f32c(dy, "dy")
        N, C = x.shape
        lib, dev = _lib.api(), x.device
        dx, dw, db = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(weight)
        ws = _workspace(lib, N, C, dev)
        lib.glam_layer_norm_flat_bwd(ptr(x), ptr(dy), ptr(weight), ptr(stat), N, C, eps, ptr(dx), ptr(dw), ptr(db), ptr(ws), ws.numel() * 4,
                                     form, max_blocks, stream())
        return dx, dw, db, None, None, None


def layer_norm_flat(x, weight, bias, eps=1e-5, form=0, max_blocks=0):
    """PyG's graph ``LayerNorm(C)(x)`` with ``batch=None``: ``x = x - x.mean(); (x / (x.std(unbiased=False) + eps)) * weight + bias``
    on a float32 ``[N, C]`` (``N * C >= 1``; a constant input has no finite gradient, as in torch)."""
    return _LayerNormFlat.apply(x, weight, bias, eps, form, max_blocks)


def column_norm_supported(x):
    """The column-norm kernels serve this input: a float32 ``[N, C]`` on a HIP device, outside autocast, with at least one element."""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.numel() > 0 and not torch.is_autocast_enabled()
