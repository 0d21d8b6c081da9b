"""The optimizers of the training loop that drives the path: ``Adam(self.model.parameters(), lr=args.lr)`` (reference
``src_1gp/trainer.py:49-50``, stepped at ``trainer.py:301``, its learning rate moved by ``ReduceLROnPlateau``, ``trainer.py:55,85``).

``glam_amd.optim.Adam`` is a ``torch.optim.Optimizer`` with ``torch.optim.Adam``'s constructor arguments, ``param_groups`` and
``state_dict`` layout (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter), so schedulers and checkpoints work unchanged.  Its step is
ONE HIP launch over all parameter tensors (``glam_adam_step``: 4 µs where the library's multi-tensor kernel takes 45 µs on a
default-shaped model — 9 workgroups of double-precision arithmetic), and its host side is a cached address table: 36 ``data_ptr()`` reads
per step instead of the library optimizer's per-step list building.  It is always "capturable": the step count lives on the device and
the launch advances it, a learning rate given as a device tensor is read by the launch (``glam_amd.graphs.GraphedTrainStep`` does that).

Differences from ``torch.optim.Adam``, by design: fp32 CUDA/HIP parameters only; no ``amsgrad`` / ``maximize`` / ``differentiable``;
one step count per parameter GROUP (a parameter without a gradient in some step keeps its moments and still sees the group's bias
correction — the library counts per tensor); arithmetic in fp32 with the bias corrections in double (the library's fused kernel works
in double, its single-tensor path in fp32: all three agree to rounding, tested).

``glam_amd.optim.Ranger`` is the reference's other optimizer (``Ranger(model.parameters(), lr=args.lr, k=args.k)``,
``src_1gp/trainer.py:45-48``; the search draws ``'optim': choice(['Adam', 'Ranger'])``): RAdam + Lookahead + gradient centralisation
with ``src_1gp/ranger.py``'s constructor, argument checks, ``param_groups`` keys, attributes and per-parameter state (``step`` /
``exp_avg`` / ``exp_avg_sq`` / ``slow_buffer``).  Its step is ONE HIP launch (``glam_ranger_step``) that reads the step count — and with it
the rectification branch and the Lookahead period — from the device, so ``GraphedTrainStep`` captures it.  Its ``state_dict`` writes
``step`` as a Python int, as the reference does: checkpoints go both ways.  Side effects of the reference kept on purpose: with
``gc_loc=True`` the centralised gradient is left in ``p.grad``; in the un-rectified steps the update direction IS ``exp_avg``, so
``weight_decay`` and late centralisation (``gc_loc=False``) also change ``exp_avg``.  Not kept: the ``radam_buffer`` cache.
Differences from the reference, by design: fp32 contiguous HIP parameters only; one step count per parameter GROUP, as for ``Adam`` (a
parameter without a gradient sits a step out and keeps its buffers, but does not fall behind the group's count: the reference counts
per tensor); the slow weights of every parameter start as a copy of it when the group's first step runs (the reference copies a
parameter at ITS first step with a gradient — the same value unless the parameter was changed by other means in between).

Both share ``_FlatStateOptimizer``: per group, the buffers of all parameters in one flat device allocation each (16-byte aligned views,
adopted from loaded state), a device step counter and ticket, and a host address table refreshed by one list compare per step."""
from __future__ import annotations

import ctypes

import numpy as np
import torch
from torch.optim import optimizer as _topt      # (the module: its global step-hook tables)

from . import _lib
from ._lib import GlamHipError


class _FlatStateOptimizer(torch.optim.Optimizer):
    """The plan / address-table machinery of ``Adam`` and ``Ranger``.  A subclass names its per-parameter buffers (``_BUFFERS``: the
    table columns after {param, grad}) and implements ``_call(lib, group, plan, table, numel, keep)``, the one ABI call of a group."""
    _BUFFERS = ()

    def _init_state(self):
        self._plans = {}          # group index -> _Plan

    def _fresh_buffer(self, name, p):
        """The initial value of buffer ``name`` of a parameter without state (moments: zero)."""
        return None

    class _Plan:
        __slots__ = ("params", "table", "numel", "step", "ticket", "flat", "sub", "sub_key", "gptrs", "pptrs", "row", "row_key")

    def _plan(self, gi, group):
        plan = self._plans.get(gi)
        ps = [p for p in group["params"] if p.requires_grad]
        if plan is not None and len(plan.params) == len(ps) and all(a is b for a, b in zip(plan.params, ps)):
            return plan
        name = type(self).__name__
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise GlamHipError(f"glam_amd.optim.{name}: parameters must be contiguous fp32 tensors on a HIP device")
        dev = ps[0].device
        if any(p.device != dev for p in ps):
            raise GlamHipError(f"glam_amd.optim.{name}: one device per parameter group")
        old = self._plans.get(gi)
        plan = _FlatStateOptimizer._Plan()
        plan.params = ps
        sizes = [(p.numel() + 3) // 4 * 4 for p in ps]                       # every view starts 16-byte aligned
        plan.flat = [torch.zeros(sum(sizes), dtype=torch.float32, device=dev) for _ in self._BUFFERS]
        plan.step = torch.zeros((), dtype=torch.float32, device=dev)
        plan.ticket = torch.zeros(544, dtype=torch.int32, device=dev)      # GLAM_ADAM_TICKET_WORDS: main ticket + 16 sub-counters, 128 B apart
        plan.table = np.zeros((len(ps), 2 + len(self._BUFFERS)), dtype=np.uint64)
        plan.numel = np.array([p.numel() for p in ps], dtype=np.int64)
        plan.sub, plan.sub_key = None, None
        plan.row, plan.row_key = None, None
        plan.gptrs, plan.pptrs = None, None          # gradient / parameter addresses as the table holds them (step(): one list compare)
        off = 0
        for i, (p, n) in enumerate(zip(ps, sizes)):
            views = [f[off:off + p.numel()].view_as(p) for f in plan.flat]
            st = self.state[p]
            adopted = self._BUFFERS[0] in st                                  # (load_state_dict, a re-grouped parameter)
            for b, view in zip(self._BUFFERS, views):
                src = st[b] if adopted and b in st else self._fresh_buffer(b, p)
                if src is not None:
                    view.copy_(src)
            if adopted and (i == 0 or float(st["step"]) > float(plan.step)):
                plan.step.fill_(float(st["step"]))
            for b, view in zip(self._BUFFERS, views):
                st[b] = view
            st["step"] = plan.step
            plan.table[i] = (p.data_ptr(), 0, *[view.data_ptr() for view in views])
            off += n
        del old
        self._plans[gi] = plan
        return plan

    def zero_grad(self, set_to_none: bool = True):
        """``torch.optim.Optimizer.zero_grad``; its default (``set_to_none=True``) as the plain loop it amounts to — the base class's
        goes through a dynamo guard and a profiler scope, 25 us per call where the reference's loop is bound by host time (its batch of
        32: DESIGN.md §7)."""
        if not set_to_none:
            return super().zero_grad(set_to_none=False)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    p.grad = None

    def step(self, closure=None):
        # (torch wraps an optimizer's step in a profiler scope that also runs the step hooks — Optimizer.profile_hook_step, ≈15 us per
        #  call; `step.hooked` below keeps it off this class, and the hooks, when there are any, are run here)
        if self._optimizer_step_pre_hooks or self._optimizer_step_post_hooks or _topt._global_optimizer_pre_hooks or _topt._global_optimizer_post_hooks:
            return _FlatStateOptimizer._hooked_step(self, closure)
        return self._step(closure)

    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.api()
        from . import ops
        ops.parameters_written()         # the launch below writes parameters through raw pointers: no version counter moves
        with torch.no_grad():
            self._launch(lib)
        return loss

    def _launch(self, lib):
        for gi, group in enumerate(self.param_groups):
            if not any(p.requires_grad for p in group["params"]):
                continue
            plan = self._plan(gi, group)
            table, numel = plan.table, plan.numel
            missing = None
            grads = [p.grad for p in plan.params]
            complete = all([g is not None for g in grads])      # (`None in grads` would compare TENSORS with None: a torch call each)
            if complete:
                # the common step: every parameter has a gradient — the addresses against last step's, one list compare each (a loop
                # over numpy elements cost 35 us for the default model's 24 tensors)
                gp, pp = [g.data_ptr() for g in grads], [p.data_ptr() for p in plan.params]
                if gp != plan.gptrs:
                    for i, (g, p) in enumerate(zip(grads, plan.params)):
                        if table[i, 1] != gp[i]:                             # a gradient tensor not seen at this address yet
                            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or g.is_sparse:
                                raise GlamHipError(f"glam_amd.optim.{type(self).__name__}: gradients must be dense contiguous fp32 tensors on the parameter's device")
                            table[i, 1] = gp[i]
                    plan.gptrs = gp
                if pp != plan.pptrs:                                         # `p.data = ...` since the last step
                    for i in range(len(pp)):
                        table[i, 0] = pp[i]
                    plan.pptrs = pp
            else:
                plan.gptrs = plan.pptrs = None
            for i, p in (() if complete else enumerate(plan.params)):
                g = p.grad
                if g is None:
                    missing = missing or []
                    missing.append(i)
                    continue
                ptr = g.data_ptr()
                if table[i, 1] != ptr:                                       # a gradient tensor not seen at this address yet
                    if g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or g.is_sparse:
                        raise GlamHipError(f"glam_amd.optim.{type(self).__name__}: gradients must be dense contiguous fp32 tensors on the parameter's device")
                    table[i, 1] = ptr
                if table[i, 0] != p.data_ptr():                              # `p.data = ...` since the last step
                    table[i, 0] = p.data_ptr()
            if missing:                                                      # parameters without a gradient sit this step out
                if len(missing) == len(plan.params):
                    continue
                keep = np.ones(len(plan.params), dtype=bool)
                keep[missing] = False
                table, numel = np.ascontiguousarray(table[keep]), np.ascontiguousarray(numel[keep])
            self._call(lib, group, plan, table, numel, None if not missing else keep)

    def _lr_arg(self, group):
        """(device learning rate or None, host learning rate) of a group: a one-element fp32 device tensor is read by the launch."""
        lr = group["lr"]
        if torch.is_tensor(lr):
            if lr.is_cuda:
                if lr.dtype != torch.float32 or lr.numel() != 1:
                    raise GlamHipError(f"glam_amd.optim.{type(self).__name__}: a device learning rate must be one fp32 element")
                return lr, 0.0
            return None, float(lr)
        return None, lr

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plans = {}                 # raw device addresses: never carried over by pickling / copying

    def __deepcopy__(self, memo):
        # the plans hold raw addresses of the ORIGINAL moment buffers: a copy rebuilds its own from its (deep-copied) state
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            setattr(new, k, {} if k == "_plans" else copy.deepcopy(v, memo))
        for gi, group in enumerate(new.param_groups):
            if any(p.requires_grad for p in group["params"]) and any(self._BUFFERS[0] in new.state.get(p, {}) for p in group["params"]):
                new._plan(gi, group)
        return new

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # adopt the loaded per-parameter tensors into fresh flat buffers NOW: the base class does not copy tensors that already have the
        # parameter's dtype and device, so until then this optimizer's state aliases the one the dictionary came from
        self._plans.clear()
        for gi, group in enumerate(self.param_groups):
            if any(p.requires_grad for p in group["params"]):
                self._plan(gi, group)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_plans"):
            self._plans.clear()


class Adam(_FlatStateOptimizer):
    _BUFFERS = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 capturable=True, differentiable=False, foreach=None, fused=None):
        if amsgrad or maximize or differentiable:
            raise GlamHipError("glam_amd.optim.Adam: amsgrad / maximize / differentiable are not implemented")
        if not (torch.is_tensor(lr) or lr >= 0.0) or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or eps < 0.0 or weight_decay < 0.0:
            raise ValueError("glam_amd.optim.Adam: invalid hyper-parameters")
        # `capturable` is always true here (device-side step count); the key is kept because GraphedTrainStep and user code look for it
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      capturable=True))
        self._init_state()

    def _call(self, lib, group, plan, table, numel, keep):
        lr_dev, lr = self._lr_arg(group)
        b1, b2 = group["betas"]
        lib.glam_adam_step(table.ctypes.data, numel.ctypes.data, len(numel), plan.step.data_ptr(), plan.ticket.data_ptr(),
                           lr_dev.data_ptr() if lr_dev is not None else None, float(lr), float(b1), float(b2), float(group["eps"]),
                           float(group["weight_decay"]), torch.cuda.current_stream(plan.step.device).cuda_stream)

    def state_dict(self):
        """``torch.optim.Adam``'s layout with a PRIVATE ``step`` per parameter: internally every parameter of a group shares one device
        counter, and a checkpoint that kept the sharing would, loaded into ``torch.optim.Adam`` (capturable / fused), be advanced once
        per parameter per step by ``_foreach_add_``."""
        sd = super().state_dict()
        for st in sd["state"].values():
            if torch.is_tensor(st.get("step")):
                st["step"] = st["step"].detach().clone()
        return sd



class Ranger(_FlatStateOptimizer):
    """``src_1gp/ranger.py``'s Ranger on the device: see the module docstring.  ``alpha``, ``N_sma_threshhold`` and the gradient
    centralisation switches are read from the optimizer's attributes and ``k`` from the group, as the reference reads them."""
    _BUFFERS = ("exp_avg", "exp_avg_sq", "slow_buffer")

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0,
                 use_gc=True, gc_conv_only=False, gc_loc=True, *, capturable=True):
        # the reference's checks and messages (ranger.py:54-61)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f'Invalid slow update rate: {alpha}')
        if not 1 <= k:
            raise ValueError(f'Invalid lookahead steps: {k}')
        if not (torch.is_tensor(lr) or lr > 0):
            raise ValueError(f'Invalid Learning Rate: {lr}')
        if not eps > 0:
            raise ValueError(f'Invalid eps: {eps}')
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0:
            raise ValueError("glam_amd.optim.Ranger: invalid hyper-parameters")
        # `capturable` is always true here (device-side step count), as for Adam
        super().__init__(params, dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                                      weight_decay=weight_decay, capturable=True))
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k
        self.gc_loc = gc_loc
        self.use_gc = use_gc
        self.gc_conv_only = gc_conv_only
        self._init_state()

    def _fresh_buffer(self, name, p):
        return p.detach() if name == "slow_buffer" else None     # Lookahead starts from the parameter as it is before the first update

    def _rows(self, plan):
        """Per tensor the row length of the centralisation (``centralized_gradient``: more than one dimension, or more than three with
        ``gc_conv_only``; a mean over dimensions 1..n per index of dimension 0), 0 for a tensor that is not centralised."""
        key = (bool(self.use_gc), bool(self.gc_conv_only))
        if plan.row_key != key:
            min_dim = 3 if self.gc_conv_only else 1
            plan.row = np.array([p.numel() // p.size(0) if self.use_gc and p.dim() > min_dim and p.size(0) > 0 else 0
                                 for p in plan.params], dtype=np.int64)
            plan.row_key = key
        return plan.row

    def _call(self, lib, group, plan, table, numel, keep):
        lr_dev, lr = self._lr_arg(group)
        row = self._rows(plan)
        if keep is not None:
            row = np.ascontiguousarray(row[keep])
        k = group["k"]
        if int(k) != k or k < 1:
            raise ValueError(f'Invalid lookahead steps: {k}')
        b1, b2 = group["betas"]
        lib.glam_ranger_step(table.ctypes.data, numel.ctypes.data, row.ctypes.data, len(numel), plan.step.data_ptr(), plan.ticket.data_ptr(),
                             lr_dev.data_ptr() if lr_dev is not None else None, float(lr), float(b1), float(b2), float(group["eps"]),
                             float(group["weight_decay"]), float(self.alpha), int(k), float(self.N_sma_threshhold), 1 if self.gc_loc else 0,
                             torch.cuda.current_stream(plan.step.device).cuda_stream)

    def state_dict(self):
        """The reference's layout: ``step`` a Python int per parameter, the buffers copied out of the flat storage (a checkpoint loaded
        into the reference's Ranger on the same device would otherwise step this optimizer's buffers too)."""
        sd = super().state_dict()
        sd["state"] = {k: dict(st) for k, st in sd["state"].items()}      # (the base class hands out this optimizer's own dictionaries)
        counts = {}
        for st in sd["state"].values():
            step = st.get("step")
            if torch.is_tensor(step):
                if id(step) not in counts:
                    counts[id(step)] = int(step.item())
                st["step"] = counts[id(step)]
            for b in self._BUFFERS:
                if torch.is_tensor(st.get(b)):
                    st[b] = st[b].detach().clone()
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:        # a checkpoint of the reference's Ranger has no `capturable` key
            group.setdefault("capturable", True)


# torch wraps `cls.step` in Optimizer.profile_hook_step when the first instance is built — unless the function says it is hooked already:
# the step runs the wrapper itself, and only when a step hook is registered (see there)
_FlatStateOptimizer._hooked_step = torch.optim.Optimizer.profile_hook_step(_FlatStateOptimizer._step)
_FlatStateOptimizer.step.hooked = True
