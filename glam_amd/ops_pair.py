"""Per-pair fusion pools (src_2gi_dti_scr/layer.py:270-283) and their held-once forms: indexed, panel, shared, gathered.

Part of ``glam_amd.ops`` (every public name here is re-exported there: ``from glam_amd import ops; ops.pair_pool(...)``).

The next fusion call is built from the helpers of this file, not from a copy of the call before it: ``host_ints`` validates a host
vector of integers, ``_Staged`` keeps its per-device copies, ``_operands`` checks the two matrices, ``_outputs`` / ``_workspace`` allocate
what a launch writes (``_all_empty``: with no row on one side), ``pair_count`` is "P of whichever index is given", the shared refusals are
``_inference_only`` / ``_require_plan`` / ``_check_sums_slab``, a plan starts from ``_plan_sizes`` / ``_plan_selection`` / ``_first_rows``, and a
Function that hands its inputs back is ``_alias_fwd`` / ``_alias_bwd`` under a wrapper that ends in ``_apply_aliasing``."""
from __future__ import annotations

import ctypes
import dataclasses
import typing

import numpy as np
import torch

from . import _lib
from ._lib import GlamHipError, f32c, ptr, require_device, stream
from .ops_readout import segment_pool


# --------------------------------------------------------------------------------------
# what every call of the family shares
# --------------------------------------------------------------------------------------
def host_ints(v, name, entries, n=None, below=None, on_device=None, wrong=None):
    """``v`` — a host sequence, numpy array or CPU tensor — as a 1-D integer numpy array (empty: ``int64[0]``), or the refusal: a device
    tensor (``GlamHipError``: validating it would be a hidden read-back), a non-integer dtype, another shape than a vector (of ``n``
    entries, if given), an entry below 0 or not below ``below`` (``IndexError``).  ``name`` / ``entries``: what the messages call the
    vector and its shape ("have one entry per pair"); ``on_device`` / ``wrong``: a caller's own text for the device refusal / for every
    other one."""
    if torch.is_tensor(v):
        if v.device.type != "cpu":
            raise GlamHipError(on_device or f"{name} lives on a device: it is validated on the host before the launch, which would be a "
                               "hidden read-back — pass the host sequence / numpy array / CPU tensor it was made from")
        v = v.detach().numpy()
    a = np.asarray(v)
    if a.size == 0:
        a = np.zeros(0, dtype=np.int64)
    if a.dtype.kind not in "iu":
        raise IndexError(wrong or f"{name} must hold integers, got {a.dtype}")
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise IndexError(wrong or f"{name} must {entries}: shape {tuple(a.shape)}" + ("" if n is None else f" for {n} pairs"))
    if a.size and (int(a.min()) < 0 or (below is not None and int(a.max()) >= below)):
        raise IndexError(wrong or f"{name} must lie in [0, {below}): got {int(a.min())} .. {int(a.max())}")
    return a


def _stage_int32(host, device, what):
    """Device copy of a host int32 vector out of pinned memory (only enqueued).  Not inside a hipGraph capture: the copy would be baked
    into the graph and the pinned buffer allocated under it — the eager first visit of a batch makes the copies a capture then finds."""
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise GlamHipError(f"{what} has no copy on {device} yet and a hipGraph capture cannot make one: keep ONE PairIndex across the "
                           "steps (ops.pair_index) and run the first step on it eagerly, as GraphedTrainStep does")
    n = int(host.shape[0])
    staged = torch.empty(max(n, 1), dtype=torch.int32, pin_memory=True)
    staged.numpy()[:n] = host
    return staged.to(device, non_blocking=True)[:n]


class _Staged:
    """Host int32 vectors — one, or two that travel together — and their device copies: ``on(device)`` is the copy (the pair of
    copies), made once per device (ONE copy out of pinned memory, only enqueued) and shared by every launch that reads it."""

    def __init__(self, what, *parts):
        self._what, self._parts = what, parts
        self._dev = {}

    def on(self, device):
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            if len(self._parts) == 1:
                t = _stage_int32(self._parts[0], device, self._what)
            else:
                n = int(self._parts[0].shape[0])
                both = _stage_int32(np.concatenate(self._parts), device, self._what)      # (one copy)
                t = (both[:n], both[n:])
            self._dev[device] = t
        return t


def _operands(who, a, b, spa, spb, na, nb):
    """The two matrices of a fusion call: on the device, 2-D, of one width, ``sp.N`` rows each -> both as contiguous fp32."""
    require_device(a, b)
    if a.dim() != 2 or b.dim() != 2 or a.size(1) != b.size(1) or a.size(0) != spa.N or b.size(0) != spb.N:
        raise GlamHipError(f"{who}: the two sides disagree (width / node count): {na} {tuple(a.shape)} for {spa.N} rows, "
                           f"{nb} {tuple(b.shape)} for {spb.N} rows")
    return f32c(a, na), f32c(b, nb)


def _outputs(shape, dev, arg=True, D=None, ws_bytes=None):
    """What a fusion launch writes: ``out`` fp32 ``[*shape, 2]``, ``arg`` int32 ``[*shape, 2]`` (or None), ``sums`` fp32 ``[*shape, 2, D]``
    (with ``D``: what a backward reads again) and the workspace of ``ws_bytes`` (never an empty one: it has no address)."""
    return (torch.empty(*shape, 2, dtype=torch.float32, device=dev),
            torch.empty(*shape, 2, dtype=torch.int32, device=dev) if arg else None,
            None if D is None else torch.empty(*shape, 2, D, dtype=torch.float32, device=dev),
            None if ws_bytes is None else _workspace(ws_bytes, dev))


def _workspace(nbytes, dev):
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)


def _all_empty(out, arg):          # no row on one side: every pair is empty (and the empty matrix has no address to pass to a launch)
    out.zero_()
    if arg is not None:
        arg.fill_(-1)


def _inference_only(who, tensors, instead):
    """The refusal of a call without a backward when autograd would follow one of ``tensors``; ``instead``: what trains."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise GlamHipError(f"{who} is inference only (no backward): call it under torch.no_grad(); {instead}")


def _require_plan(who, plan, cls, maker):
    if not isinstance(plan, cls):
        raise GlamHipError(f"{who}: plan must come from ops.{maker} (the kernel trusts its table)")


def _check_sums_slab(who, D, dev, sums, slab, per_wave):
    """What a caller may hand a stationary launch: ``sums`` — ``(name, tensor or None, rows)`` each, ``[rows, D]`` on ``dev`` — and a slab."""
    for name, t, rows in sums:
        if t is not None and (t.dim() != 2 or tuple(t.shape) != (rows, D) or t.device != dev):
            raise GlamHipError(f"{who}: {name} must be the [{rows}, {D}] column sums on {dev}, got {tuple(t.shape)} on {t.device}")
    if int(slab) < 0:
        raise GlamHipError(f"{who}: slab must be 0 (choose) or the {per_wave} per wave, got {slab}")


def _plan_sizes(who, sizes_host, nouns):
    """The sizes a plan is built over (``nouns``: what ``who``'s messages call them) as a host int64 vector."""
    return host_ints(sizes_host, "sizes", None, wrong=f"{who}: {nouns} must be a vector of non-negative integers",
                     on_device=f"{who}: {nouns} live on a device: the plan is built on the host — pass their host copy").astype(np.int64)


def _plan_selection(name, entries, selection, Q):
    return np.arange(Q, dtype=np.int32) if selection is None else host_ints(selection, name, entries, below=Q).astype(np.int32)


def _first_rows(sizes, too_many):          # -> (the offsets of the segments' rows, int64 [Q + 1]; N, their last: below 2^31 - 1)
    first = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(sizes, dtype=np.int64)])
    if int(first[-1]) >= 2 ** 31 - 1:
        raise IndexError(too_many)
    return first, int(first[-1])


def _alias_fwd(ctx, out, a_in, b_in, with_identity):
    """What a fusion Function returns.  ``with_identity``: the two inputs come back as outputs — what the caller does with them next
    sends its gradient HERE, into the backward launch of this node."""
    ctx.aliased = bool(with_identity)
    if ctx.aliased:
        ctx.set_materialize_grads(False)
        return out, a_in.view_as(a_in), b_in.view_as(b_in)
    return out


def _alias_bwd(d_out, d_a, d_b, a, b, na, nb, nothing_written=False):
    """The incoming gradients of such a node -> ``(launch, d_out, d_a, d_b)``.  ``launch``: the three are ready for the entry point
    (contiguous fp32; ``d_a`` / ``d_b``, the gradients of the inputs' next use, may be None).  Not ``launch``: ``d_a, d_b`` ARE the
    input gradients — the fusion values were not used (``d_out`` is None: only with the aliases), or the entry point writes nothing
    (``nothing_written``) and the gradients are those of the next use, or zeros."""
    if d_out is None:
        return False, None, d_a, d_b
    d_out = f32c(d_out, "d_out")
    d_a = None if d_a is None else f32c(d_a, f"d_{na} (next use)")
    d_b = None if d_b is None else f32c(d_b, f"d_{nb} (next use)")
    if nothing_written:
        return False, None, torch.zeros_like(a) if d_a is None else d_a, torch.zeros_like(b) if d_b is None else d_b
    return True, d_out, d_a, d_b


def _apply_aliasing(fn, args, a, b, with_identity, add_width=None):
    """``fn.apply(*args)``; ``with_identity``: ``(out, a, b)`` — through the node where its backward launch can take the gradients of
    their next use (both require grad, fp32), the plain inputs appended otherwise.  ``add_width``: ask the library whether that width
    has the adding backward (None: every width of the entry point's table has it)."""
    if not with_identity:
        return fn.apply(*args)
    # (is_cuda: a CPU operand goes on to require_device's refusal in the forward, not to a query of the library)
    if (torch.is_grad_enabled() and a.requires_grad and b.requires_grad and a.is_cuda and a.dtype == torch.float32
            and b.dtype == torch.float32 and (add_width is None or _lib.api().glam_pair_pool_add_supported(add_width) == 1)):
        return fn.apply(*args, True)
    return fn.apply(*args), a, b


# --------------------------------------------------------------------------------------
# one graph per pair and side (csrc/pairpool.hip)
# --------------------------------------------------------------------------------------
class _PairPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mol, pro, msp, psp, with_identity=False):
        mol_in, pro_in = mol, pro
        mol, pro = _operands("pair_pool", mol, pro, msp, psp, "mol_out", "pro_out")
        if msp.B != psp.B:
            raise GlamHipError(f"pair_pool: the two batches disagree (pair count): {msp.B} ligand graphs, {psp.B} protein graphs")
        P, D = msp.B, mol.size(1)
        lib = _lib.api()
        out, arg, sums, ws = _outputs((P,), mol.device, D=D, ws_bytes=lib.glam_pair_pool_workspace_bytes(P, D))
        lib.glam_pair_pool_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), P, D, ptr(out), ptr(arg), ptr(sums), ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(mol, pro, arg, sums)
        ctx.sps = (msp, psp)
        return _alias_fwd(ctx, out, mol_in, pro_in, with_identity)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_ma=None, d_pa=None):
        mol, pro, arg, sums = ctx.saved_tensors
        msp, psp = ctx.sps
        launch, d_out, d_ma, d_pa = _alias_bwd(d_out, d_ma, d_pa, mol, pro, "mol", "pro")
        if not launch:
            return d_ma, d_pa, None, None, None
        d_mol, d_pro = torch.empty_like(mol), torch.empty_like(pro)
        lib = _lib.api()
        if d_ma is not None or d_pa is not None:      # (two entry points: the library's choice)
            lib.glam_pair_pool_bwd_add(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(arg), ptr(sums), ptr(d_out), msp.B, mol.size(1),
                                       ptr(d_ma), ptr(d_pa), ptr(d_mol), ptr(d_pro), stream())
        else:
            lib.glam_pair_pool_bwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(arg), ptr(sums), ptr(d_out), msp.B,
                                   mol.size(1), ptr(d_mol), ptr(d_pro), stream())
        return d_mol, d_pro, None, None, None


def pair_pool(mol_out, pro_out, msp, psp, with_identity=False):
    """``[max, mean]`` of ``mol[seg_i] @ pro[seg_i].T`` per pair -> ``[P, 2]`` (dot_and_global_pool2).  ``with_identity``: returns
    ``(out, mol_out, pro_out)`` with the two matrices handed back through this node where that saves the add launches of their second
    use (the next message step): its gradient is then added inside this node's backward launch."""
    # (add_width: glam_pair_pool_bwd_add exists for the widths the library names)
    return _apply_aliasing(_PairPool, (mol_out, pro_out, msp, psp), mol_out, pro_out, with_identity,
                           add_width=mol_out.size(1) if with_identity else None)


class _PairPool5(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mol, pro, msp, psp):
        require_device(mol, pro)
        mol, pro = f32c(mol, "mol_out"), f32c(pro, "pro_out")
        if msp.B != psp.B or mol.size(1) != pro.size(1) or mol.size(0) != msp.N or pro.size(0) != psp.N:
            raise GlamHipError("pair_pool5: the two batches disagree (pair count / width / node count)")
        P, D = msp.B, mol.size(1)
        out = torch.empty(P, 5, dtype=torch.float32, device=mol.device)
        arg = torch.empty(P, 6, dtype=torch.int32, device=mol.device)
        _lib.api().glam_pair_pool5_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), P, D, ptr(out), ptr(arg), stream())
        ctx.save_for_backward(mol, pro, out, arg)
        ctx.sps = (msp, psp)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        mol, pro, out, arg = ctx.saved_tensors
        msp, psp = ctx.sps
        d_out = f32c(d_out, "d_out")
        d_mol, d_pro = torch.empty_like(mol), torch.empty_like(pro)
        _lib.api().glam_pair_pool5_bwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(out), ptr(arg), ptr(d_out), msp.B,
                                       mol.size(1), ptr(d_mol), ptr(d_pro), stream())
        return d_mol, d_pro, None, None


def pair_pool5(mol_out, pro_out, msp, psp):
    """``[max, mean, median, min, std]`` of ``mol[seg_i] @ pro[seg_i].T`` per pair -> ``[P, 5]`` (dot_and_global_pool5);
    widths that are multiples of 4 up to 128 (``pad_cols`` the operands first: zero columns do not change a score)."""
    return _PairPool5.apply(mol_out, pro_out, msp, psp)


# --------------------------------------------------------------------------------------
# screening: the fusion against proteins that are held once (csrc/pairpool.hip, glam_pair_pool_indexed_fwd)
# --------------------------------------------------------------------------------------
class PairIndex(_Staged):
    """A validated pair -> protein index: ``host`` int32 ``[P]`` (numpy) with every entry in ``[0, Q)``.  ``on(device)`` is its device
    copy, made once per device (out of pinned memory, only enqueued) and shared by every launch that reads it."""

    def __init__(self, host, Q):
        _Staged.__init__(self, "the pair -> protein index", host)
        self.host, self.P, self.Q = host, int(host.shape[0]), int(Q)
        self._by_protein = None

    def by_protein(self):
        """The pairs grouped by protein, for the sums of the training call (``ops.pair_pool_shared`` / ``ops.pair_rows``): ``order`` int32
        ``[P]`` — the stable argsort of the index (the pairs of a protein keep their batch order) — and ``ptr`` int32 ``[Q + 1]``, the
        offsets of the proteins' runs in it.  Built once, on the host; ``.on(device)`` -> their device copies, made once per device."""
        if self._by_protein is None:
            self._by_protein = PairsByProtein(self.host, self.Q)
        return self._by_protein


class PairsByProtein(_Staged):
    """``order`` / ``ptr`` of ``PairIndex.by_protein`` (host, int32 numpy) and their device copies."""

    def __init__(self, host, Q):
        P, Q = int(host.shape[0]), int(Q)
        if P and (int(host.min()) < 0 or int(host.max()) >= Q):
            raise IndexError(f"the pair -> protein index must lie in [0, {Q})")
        self.order = np.argsort(host, kind="stable").astype(np.int32)
        self.ptr = np.zeros(Q + 1, dtype=np.int32)
        np.cumsum(np.bincount(host, minlength=Q)[:Q], out=self.ptr[1:])
        if int(self.ptr[-1]) != P:
            raise IndexError("the pair -> protein index does not sort into its proteins' runs")
        self.P, self.Q = P, Q
        _Staged.__init__(self, "the pair list by protein", self.order, self.ptr)


# --------------------------------------------------------------------------------------
# refillable pair lists: the index and its by-protein lists at fixed device addresses, refilled by one launch (csrc/pairlist.hip)
# --------------------------------------------------------------------------------------
def pair_list_bounds(P, Q, pad=0, name="pro_of_pair"):
    """``(P, Q, pad)`` of a ``PairList`` as ints, or the refusal — host only, before any allocation or copy: ``P >= 1``, ``Q >= 1``, ``pad``
    in ``[0, Q)`` (``ValueError``), and a build the kernel has (``glam_pair_list_supported``: ``P``, ``Q`` <= 65 536 and ``P * Q`` <= 2^26 —
    its work is O(P * Q); ``GlamHipError``)."""
    P, Q, pad = int(P), int(Q), int(pad)
    if P < 1 or Q < 1 or not 0 <= pad < Q:
        raise ValueError(f"a pair list of {name} needs P >= 1 pairs over Q >= 1 segments and its padding segment in [0, Q): got P = {P}, "
                         f"Q = {Q}, pad = {pad}")
    if _lib.load().glam_pair_list_supported(P, Q) != 0:          # (a status: the raw binding hands it back)
        raise GlamHipError(f"a pair list of {P} pairs over {Q} segments is beyond what one launch builds (P, Q <= 65536 and P * Q <= 2^26: "
                           f"the build compares every pair with every segment) — build the lists on the host: ops.pair_index")
    return P, Q, pad


def pair_list_launch(ids, a, col_a, b, col_b, B, y=None, y_out=None):
    """ONE ``glam_pair_list_load`` on the current stream: the lists of ``a`` / ``b`` (``PairList`` or None) from the device columns ``col_a``
    / ``col_b`` through the pair ids ``ids`` (device int32 ``[B]``, None = identity), and ``y_out[:B] = y[ids]``.  Neither list: the label
    gather alone.  Trusted: callers validate on the host first."""
    side = lambda l, c: (None, 0, 0, None, None, None) if l is None else (ptr(c), l.Q, l.pad, ptr(l.idx), ptr(l.order), ptr(l.ptr))   # noqa: E731
    ca, Qa, pa, *outs_a = side(a, col_a)
    cb, Qb, pb, *outs_b = side(b, col_b)
    P = int(B) if a is None and b is None else (a if a is not None else b).P
    rb = 0 if y is None else int(np.prod(y.shape[1:], dtype=np.int64)) * y.element_size()
    _lib.api().glam_pair_list_load(ptr(ids), ca, cb, ptr(y), rb, int(B), P, Qa, Qb, pa, pb, *outs_a, *outs_b, ptr(y_out), stream())


class _FixedLists:
    """``by_protein()`` of a ``PairList``: ``on(device)`` -> its fixed ``(order, ptr)``."""

    def __init__(self, owner):
        self._owner = owner

    def on(self, device):
        self._owner.on(device)
        return self._owner.order, self._owner.ptr


class PairList(PairIndex):
    """A ``PairIndex`` of FIXED CAPACITY that lives on the device: ``idx`` int32 ``[P]``, ``order`` int32 ``[P]`` and ``ptr`` int32 ``[Q + 1]``
    are allocated once and hold whatever the last load put into them (``glam_pair_list_load``, csrc/pairlist.hip: bit for bit the lists
    ``PairsByProtein`` builds on the host), so a training step captured on this object replays for every pair list of a shuffling loop
    (DESIGN.md §4.29).  ``on(device)`` is ``idx``, ``by_protein().on(device)`` is ``(order, ptr)`` — the same tensors every time; another
    device than its own is refused.  ``host`` is None: what builds host tables from an index (``ops.map_plan``, ``matrix_top``) refuses it.
    ``pad``: the segment the slots behind a shorter load point at.  ``name`` / ``over``: as ``pair_index``.  Until the first ``load`` every
    slot points at ``pad``."""

    def __init__(self, P, Q, device, pad=0, name="pro_of_pair", over="proteins"):
        self.P, self.Q, self.pad = pair_list_bounds(P, Q, pad, name)
        self.host, self.name, self.over = None, name, over
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise GlamHipError(f"a PairList lives on an MI355X HIP device (got {self.device}); the host form is ops.pair_index")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # one allocation, every tensor on a 16-byte boundary
        sizes = [self.P, self.P, self.Q + 1, self.P]
        starts = np.concatenate([[0], np.cumsum([(s + 3) & ~3 for s in sizes])])
        self._arena = torch.zeros(int(starts[-1]), dtype=torch.int32, device=self.device)
        self.idx, self.order, self.ptr, self._stage = [self._arena[a:a + s] for a, s in zip(starts[:-1].tolist(), sizes)]
        self._lists = _FixedLists(self)
        self._launched = False
        self._stage.fill_(self.pad)
        self.glam_reload()

    def on(self, device):
        device = torch.device(device)
        if device.type != self.device.type or (device.index is not None and device.index != self.device.index):
            raise GlamHipError(f"this PairList lives on {self.device}, the operands on {device}: a pair list is read where it was loaded")
        return self.idx

    def by_protein(self):
        return self._lists

    def check(self, index):
        """``index`` as the int32 ``[P]`` host vector a load stages — at most ``P`` integers in ``[0, Q)`` (``host_ints``: ``IndexError``; a
        device tensor: ``GlamHipError``), the slots behind them at ``pad`` — host only."""
        a = host_ints(index, self.name, "have one entry per pair", below=self.Q)
        if a.shape[0] > self.P:
            raise IndexError(f"{self.name} must hold at most the {self.P} pairs of this PairList, got {a.shape[0]}")
        full = np.full(self.P, self.pad, dtype=np.int32)
        full[:a.shape[0]] = a
        return full

    def load(self, index, launch=True):
        """Put the pair -> segment index ``index`` (host integers, ``B <= P`` of them, each in ``[0, Q)``) into this list: checked on the
        host (``IndexError`` before anything is enqueued), ONE pinned, non-blocking upload into the fixed staging vector, one launch that
        rewrites ``idx``, ``order`` and ``ptr`` whole.  ``launch=False`` uploads only — for a step that holds the launch itself
        (``glam_reload()`` first in it, as ``GraphedTrainStep`` does for a batch: the ``PaddedBatch`` protocol)."""
        full = self.check(index)
        require_device(self.idx)
        staged = torch.empty(self.P, dtype=torch.int32, pin_memory=True)
        staged.numpy()[...] = full
        self._stage.copy_(staged, non_blocking=True)
        self._launched = False
        if launch:
            self.glam_reload()
            self._launched = True
        return self

    def glam_reload(self):
        """Enqueue the launch for the index now in the staging vector, on the current stream — inside a capture it becomes a node of the
        graph.  Outside a capture a ``load`` that has launched already is not repeated."""
        if self._launched and not torch.cuda.is_current_stream_capturing():
            self._launched = False
            return
        pair_list_launch(None, self, self._stage, None, None, self.P)


def host_index(index, who, instead):
    """``index.host`` of a ``PairIndex``, or the refusal of a ``PairList`` (no host copy) in the words of ``who``; ``instead``: what to pass."""
    if isinstance(index, PairList):
        raise GlamHipError(f"{who} builds its tables on the host and a PairList keeps its index on the device only (reading it would be a "
                           f"hidden read-back): pass {instead}")
    return index.host


def pair_index(pro_of_pair, P, Q, default="identity", name="pro_of_pair", over="proteins"):
    """``PairIndex`` of ``pro_of_pair`` for ``P`` pairs over ``Q`` proteins — host only, before anything is launched (the kernel trusts
    the index; the policy of ``data.resident_table``).  A host sequence, numpy array or CPU tensor of integers of length ``P``;
    ``IndexError`` for a wrong length or an entry outside ``[0, Q)``; a device tensor is refused (validating it would be a hidden
    read-back).  ``None``: ``default="identity"`` pairs ligand i with protein i (needs ``Q == P``), ``default="single"`` pairs every
    ligand with the one protein (needs ``Q == 1``).  ``name`` / ``over``: what the messages call the index and the things it points
    into (``ops.pair_pool_gather`` validates ``idx1`` / ``idx2`` over drugs with the same rules)."""
    P, Q = int(P), int(Q)
    if isinstance(pro_of_pair, PairIndex):
        if pro_of_pair.P != P or pro_of_pair.Q != Q:
            raise IndexError(f"{name} was validated for {pro_of_pair.P} pairs over {pro_of_pair.Q} {over}, not {P} over {Q}")
        return pro_of_pair
    if pro_of_pair is None:
        if default == "identity":
            if Q != P:
                if name != "pro_of_pair":
                    raise IndexError(f"{name}=None takes segment i for pair i: {P} pairs but {Q} {over}")
                raise IndexError(f"pro_of_pair=None pairs ligand i with protein i: {P} ligands but {Q} proteins")
            return PairIndex(np.arange(P, dtype=np.int32), Q)
        if Q != 1:
            raise IndexError(f"pro_of_pair=None screens against the one encoded protein, but the encoding holds {Q}: pass the index")
        return PairIndex(np.zeros(P, dtype=np.int32), Q)
    return PairIndex(host_ints(pro_of_pair, name, "have one entry per pair", n=P, below=Q).astype(np.int32), Q)


def pair_count(idx1, idx2=None, default=None):
    """``P`` of whichever index is given — a ``PairIndex`` or a host vector; ``default`` when neither is."""
    given = idx1 if idx1 is not None else idx2
    return default if given is None else given.P if isinstance(given, PairIndex) else len(given)


def pair_pool_indexed(mol_out, pro_out, msp, psp, pro_of_pair=None, return_argmax=False):
    """``[max, mean]`` of ``mol[seg_i] @ pro[seg_q].T`` with ``q = pro_of_pair[i]`` -> ``[P, 2]``: ``pair_pool`` against proteins that are
    held once (``psp.B`` segments) instead of once per pair.  The max column — and with ``return_argmax`` the ``[P, 2]`` int32 rows of
    the maximum in ``mol_out`` / ``pro_out`` (-1 for an empty pair) — is bit for bit that of ``pair_pool`` on replicated residue rows.
    ``pro_of_pair``: see ``pair_index`` (``None`` = identity).  Inference only: there is no backward (training is ``ops.pair_pool``)."""
    P, Q = msp.B, psp.B
    index = pair_index(pro_of_pair, P, Q)
    _inference_only("pair_pool_indexed", (mol_out, pro_out), "the training route is ops.pair_pool on one protein graph per pair")
    mol, pro = _operands("pair_pool_indexed", mol_out, pro_out, msp, psp, "mol_out", "pro_out")
    D = mol.size(1)
    lib = _lib.api()
    out, arg, _, ws = _outputs((P,), mol.device, arg=return_argmax, ws_bytes=lib.glam_pair_pool_workspace_bytes(P, D))
    lib.glam_pair_pool_indexed_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(index.on(mol.device)), P, Q, D, ptr(out), ptr(arg),
                                   ptr(ws), ws.numel(), stream())
    return (out, arg) if return_argmax else out


# --------------------------------------------------------------------------------------
# panel screening: every ligand against every selected protein, protein-stationary (csrc/pairpanel.hip, glam_pair_pool_panel_fwd)
# --------------------------------------------------------------------------------------
PANEL_CHUNK = 64      # residue rows per chunk (one per lane of the wave that holds them) = kStreamChunk of csrc/pairstream.h


class PanelPlan(_Staged):
    """The work of one panel call over a validated selection: ``sel`` int32 ``[Qs]`` (every entry in ``[0, Q)``) and ``work`` int32
    ``[4 * total_chunks + Qs + 1]`` — per chunk of 64 residue rows, in selection order, ``(j, first row of the chunk in the encoding,
    rows in the chunk, index of its partials in the workspace)``, then ``chunk_ptr[Qs + 1]``, the offsets of the selections' chunk
    runs (``chunks`` / ``chunk_ptr`` are views of it).  Host numpy; ``on(device)`` -> ``(sel, work)`` on the device, made once per
    device (one copy out of pinned memory, only enqueued) and shared by every launch that reads them."""

    def __init__(self, sel, sizes):
        self.sel, self.Qs, self.Q = sel, int(sel.shape[0]), int(sizes.shape[0])
        first, self.N = _first_rows(sizes, "panel_plan: the proteins hold 2^31 residue rows or more")
        n_chunks = (sizes[sel] + PANEL_CHUNK - 1) // PANEL_CHUNK                     # per selection
        chunk_ptr = np.zeros(self.Qs + 1, dtype=np.int64)
        np.cumsum(n_chunks, out=chunk_ptr[1:])
        self.total_chunks = T = int(chunk_ptr[-1])
        if T >= 2 ** 31 - 1:
            raise IndexError("panel_plan: the selection has 2^31 chunks or more")
        j = np.repeat(np.arange(self.Qs, dtype=np.int64), n_chunks)
        c = np.arange(T, dtype=np.int64) - chunk_ptr[j]                              # chunk inside its protein
        table = np.empty((T, 4), dtype=np.int32)
        table[:, 0] = j
        table[:, 1] = first[sel[j]] + PANEL_CHUNK * c
        table[:, 2] = np.minimum(sizes[sel[j]] - PANEL_CHUNK * c, PANEL_CHUNK)
        table[:, 3] = np.arange(T)
        self.work = np.concatenate([table.reshape(-1), chunk_ptr.astype(np.int32)])
        self.chunks, self.chunk_ptr = self.work[:4 * T].reshape(T, 4), self.work[4 * T:]
        _Staged.__init__(self, "the panel's selection and work table", self.sel, self.work)
        self._by_protein, self._row_index = None, {}

    def by_protein(self):
        """The selection grouped by protein, for the protein role of the training call (``ops.pair_pool_panel_shared``): ``order`` int32
        ``[Qs]`` — the stable argsort of ``sel`` (the entries that name a protein keep their order) — and ``ptr`` int32 ``[Q + 1]``, the
        offsets of the proteins' runs in it.  Built once, on the host; ``.on(device)`` -> ``(order, ptr)`` on the device, made once per
        device.  A staged pair of its own: ``plan.on(device)`` stays ``(sel, work)``."""
        if self._by_protein is None:
            self._by_protein = PairsByProtein(self.sel, self.Q)
        return self._by_protein

    def row_index(self, L):
        """The two ``PairIndex`` of the ``L * Qs`` ligand-major rows of a table over ``L`` ligands — row ``l * Qs + j`` is ligand ``l``
        (over ``L``) and protein ``sel[j]`` (over ``Q``) — for ``ops.pair_rows``.  Kept per ``L``: a later step, or a capture, finds the
        same objects and their device copies."""
        L = int(L)
        if L not in self._row_index:
            if L * self.Qs >= 2 ** 31 - 1:
                raise IndexError(f"panel_plan: a table of {L} x {self.Qs} pairs holds 2^31 - 1 rows or more")
            while len(self._row_index) >= 16:
                self._row_index.pop(next(iter(self._row_index)))
            self._row_index[L] = (PairIndex(np.repeat(np.arange(L, dtype=np.int32), self.Qs), L),
                                  PairIndex(np.tile(self.sel, L).astype(np.int32), self.Q))
        return self._row_index[L]


def panel_plan(sizes_host, proteins=None):
    """``PanelPlan`` of the selection ``proteins`` over ``Q = len(sizes_host)`` proteins of ``sizes_host[q]`` residue rows — host only
    (numpy), before anything is launched (the kernel trusts the table; the policy of ``pair_index``).  ``proteins``: ``None`` = all
    ``Q`` in order, or a host sequence / numpy array / CPU tensor of integers in ``[0, Q)``, in any order, duplicates allowed;
    ``IndexError`` for a wrong dtype or an entry outside ``[0, Q)``; a device tensor is refused (validating it would be a hidden
    read-back)."""
    sizes = _plan_sizes("panel_plan", sizes_host, "the proteins' sizes")
    return PanelPlan(_plan_selection("proteins", "be a vector of protein numbers", proteins, int(sizes.shape[0])), sizes)


def pair_pool_panel(mol_out, pro_out, msp, psp, plan, molsum=None, prosum=None, return_argmax=False, slab=0):
    """``[max, mean]`` of ``mol[seg_l] @ pro[seg_q].T`` for EVERY ligand ``l`` and every selected protein ``q = plan.sel[j]`` ->
    ``[L, Qs, 2]``: the panel of ``Qs`` calls of ``pair_pool_indexed`` with ``pro_of_pair = [sel[j]] * L`` from one protein-stationary
    launch (+ a finish launch).  The max column — and with ``return_argmax`` the ``[L, Qs, 2]`` int32 rows of the maximum in ``mol_out``
    / ``pro_out`` (-1 for an empty ligand or protein) — is bit for bit that of those calls; the mean is ``<molsum[l], prosum[q]> /
    (n_l n_q)`` and within the fp64-twin bound.  ``plan``: ``panel_plan`` over the sizes of ``psp``'s segments.  ``molsum`` ``[L, D]``
    / ``prosum`` ``[Q, D]``: the segments' column sums (``segment_pool(x, sp, "sum")``), computed here when missing — a caller that
    keeps the proteins keeps ``prosum`` too.  ``slab``: ligands per wave, 0 = the library chooses.  Widths 1..128.  Inference only:
    there is no backward (training is ``ops.pair_pool`` / ``ops.pair_pool_shared``)."""
    _require_plan("pair_pool_panel", plan, PanelPlan, "panel_plan")
    _inference_only("pair_pool_panel", (mol_out, pro_out, molsum, prosum), "the training routes are ops.pair_pool on one protein graph "
                    "per pair and ops.pair_pool_shared on proteins held once")
    if plan.Q != psp.B or plan.N != psp.N:
        raise GlamHipError(f"pair_pool_panel: the plan was made for {plan.Q} proteins of {plan.N} residue rows, the encoding holds {psp.B} of "
                           f"{psp.N}")
    mol, pro = _operands("pair_pool_panel", mol_out, pro_out, msp, psp, "mol_out", "pro_out")
    D = mol.size(1)
    _check_sums_slab("pair_pool_panel", D, mol.device, (("molsum", molsum, msp.B), ("prosum", prosum, psp.B)), slab, "ligands")
    if _lib.load().glam_pair_pool_panel_supported(D) != 0:          # (a status: the raw binding hands it back)
        raise GlamHipError(f"pair_pool_panel: width {D} is outside the kernel table (1..128)")
    out, arg, _, _ = _panel_fwd(mol, pro, msp, psp, plan, molsum, prosum, slab, return_argmax)
    return (out, arg) if return_argmax else out


def _panel_fwd(mol, pro, msp, psp, plan, molsum, prosum, slab, want_arg):
    """The launches of a panel forward on checked operands -> ``(out, arg, molsum, prosum)``: the column sums that are not given, then
    ``glam_pair_pool_panel_fwd``; with no row on one side the all-empty fill, and ``None`` for the sums (so too for a table of no entry)."""
    L, Q, Qs, D, dev = msp.B, psp.B, plan.Qs, mol.size(1), mol.device
    out, arg, _, _ = _outputs((L, Qs), dev, arg=want_arg)
    if L == 0 or Qs == 0 or msp.N == 0 or psp.N == 0:
        _all_empty(out, arg)
        return out, arg, None, None
    lib = _lib.api()
    molsum = f32c(molsum, "molsum") if molsum is not None else segment_pool(mol, msp, "sum")
    prosum = f32c(prosum, "prosum") if prosum is not None else segment_pool(pro, psp, "sum")
    sel, work = plan.on(dev)
    ws = _workspace(lib.glam_pair_pool_panel_workspace_bytes(plan.total_chunks, L), dev)
    lib.glam_pair_pool_panel_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(work), plan.total_chunks, ptr(sel), Qs, L, Q, D,
                                 ptr(molsum), ptr(prosum), int(slab), ptr(out), ptr(arg), ptr(ws), ws.numel(), stream())
    return out, arg, molsum, prosum


# --------------------------------------------------------------------------------------
# training on a label table: the panel fusion with a backward (csrc/pairpanel.hip forward, csrc/pairpanel_bwd.hip)
# --------------------------------------------------------------------------------------
class _PairPoolPanelShared(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mol, pro, msp, psp, plan, with_identity=False):
        mol_in, pro_in = mol, pro
        mol, pro = _operands("pair_pool_panel_shared", mol, pro, msp, psp, "mol_out", "pro_out")
        sel, _ = plan.on(mol.device)
        order, qptr = plan.by_protein().on(mol.device)
        out, arg, molsum, prosum = _panel_fwd(mol, pro, msp, psp, plan, None, None, 0, True)
        ctx.rows = molsum is not None          # (else an empty table, or only empty pairs: nothing for a backward to read)
        if not ctx.rows:
            molsum, prosum = mol.new_zeros(msp.B, mol.size(1)), pro.new_zeros(psp.B, mol.size(1))
        ctx.save_for_backward(mol, pro, arg, molsum, prosum, sel, order, qptr)
        ctx.sps = (msp, psp)
        return _alias_fwd(ctx, out, mol_in, pro_in, with_identity)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_ma=None, d_pa=None):
        mol, pro, arg, molsum, prosum, sel, order, qptr = ctx.saved_tensors
        msp, psp = ctx.sps
        # (an empty table, or only empty pairs: the entry point writes nothing)
        launch, d_out, d_ma, d_pa = _alias_bwd(d_out, d_ma, d_pa, mol, pro, "mol", "pro", nothing_written=not ctx.rows)
        if not launch:
            return d_ma, d_pa, None, None, None, None
        d_mol, d_pro = torch.empty_like(mol), torch.empty_like(pro)
        _lib.api().glam_pair_pool_panel_bwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(sel), ptr(order), ptr(qptr), ptr(arg),
                                            ptr(d_out), ptr(molsum), ptr(prosum), sel.numel(), msp.B, psp.B, mol.size(1), ptr(d_ma),
                                            ptr(d_pa), ptr(d_mol), ptr(d_pro), stream())
        return d_mol, d_pro, None, None, None, None


def pair_pool_panel_shared(mol_out, pro_out, msp, psp, plan, with_identity=False):
    """``pair_pool_panel`` WITH a backward: ``[max, mean]`` of ``mol[seg_l] @ pro[seg_q].T`` for EVERY ligand ``l`` and every selected
    protein ``q = plan.sel[j]`` -> ``[L, Qs, 2]``, for training on a ligand x protein label table.  The forward is the launches of
    ``pair_pool_panel`` with the argmax kept (bit for bit its output); the column sums of both sides are computed once and kept for the
    backward, ONE launch (``glam_pair_pool_panel_bwd``): a ligand's rows collect the gradients of its ``Qs`` pairs with ``j`` ascending, a
    protein's rows those of every pair that names it in ascending ``l * Qs + j`` — the batch order of the expanded pair list — without
    atomics (two runs are bit-equal); duplicates in the selection add up, a protein the selection does not name gets zeros.  ``plan``:
    ``panel_plan`` over the sizes of ``psp``'s segments — keep ONE across the steps that use it: its device copies are made on the
    first, eager, visit and a hipGraph capture needs them to exist.  Widths 1..128.  ``with_identity``: as ``pair_pool`` — ``(out,
    mol_out, pro_out)`` with the two matrices handed back through the node (both require grad, fp32): its backward launch then adds
    their later gradients itself; the plain triple otherwise."""
    _require_plan("pair_pool_panel_shared", plan, PanelPlan, "panel_plan")
    if plan.Q != psp.B or plan.N != psp.N:
        raise GlamHipError(f"pair_pool_panel_shared: the plan was made for {plan.Q} proteins of {plan.N} residue rows, the operands hold "
                           f"{psp.B} of {psp.N}")
    if mol_out.dim() == 2 and not 1 <= mol_out.size(1) <= 128:
        raise GlamHipError(f"pair_pool_panel_shared: width {mol_out.size(1)} is outside the kernel table (1..128)")
    # (no add_width: glam_pair_pool_panel_bwd adds inside its launch for every width of its table)
    return _apply_aliasing(_PairPoolPanelShared, (mol_out, pro_out, msp, psp, plan), mol_out, pro_out, with_identity)


# --------------------------------------------------------------------------------------
# training against proteins held once: the indexed fusion with a backward (csrc/pairshared.hip)
# --------------------------------------------------------------------------------------
class _PairPoolShared(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mol, pro, msp, psp, index, with_identity=False):
        mol_in, pro_in = mol, pro
        mol, pro = _operands("pair_pool_shared", mol, pro, msp, psp, "mol_out", "pro_out")
        P, Q, D, dev = msp.B, psp.B, mol.size(1), mol.device
        pidx = index.on(dev)
        order, qptr = index.by_protein().on(dev)
        lib = _lib.api()
        out, arg, sums, ws = _outputs((P,), dev, D=D, ws_bytes=lib.glam_pair_pool_workspace_bytes(P, D))
        lib.glam_pair_pool_shared_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(pidx), P, Q, D, ptr(out), ptr(arg), ptr(sums),
                                      ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(mol, pro, arg, sums, pidx, order, qptr)
        ctx.sps = (msp, psp)
        return _alias_fwd(ctx, out, mol_in, pro_in, with_identity)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_ma=None, d_pa=None):
        mol, pro, arg, sums, pidx, order, qptr = ctx.saved_tensors
        msp, psp = ctx.sps
        # (no pair: the entry point writes nothing)
        launch, d_out, d_ma, d_pa = _alias_bwd(d_out, d_ma, d_pa, mol, pro, "mol", "pro", nothing_written=msp.B == 0)
        if not launch:
            return d_ma, d_pa, None, None, None, None
        d_mol, d_pro = torch.empty_like(mol), torch.empty_like(pro)
        _lib.api().glam_pair_pool_shared_bwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(pidx), ptr(order), ptr(qptr), ptr(arg),
                                             ptr(sums), ptr(d_out), msp.B, psp.B, mol.size(1), ptr(d_ma), ptr(d_pa), ptr(d_mol),
                                             ptr(d_pro), stream())
        return d_mol, d_pro, None, None, None, None


def pair_pool_shared(mol_out, pro_out, msp, psp, pro_of_pair=None, with_identity=False):
    """``pair_pool_indexed`` WITH a backward: ``[max, mean]`` of ``mol[seg_i] @ pro[seg_q].T`` with ``q = pro_of_pair[i]`` -> ``[P, 2]``
    against proteins held once (``psp.B`` segments), for training.  The forward is bit for bit ``pair_pool_indexed``; the gradient of a
    protein's residue rows is the sum over every pair that points at it, taken in batch order without atomics (two runs are
    bit-equal); a protein no pair references gets zeros.  ``pro_of_pair``: see ``pair_index`` (``None`` = identity; every ligand against
    the one protein when ``psp.B == 1``).  ``with_identity``:
    as ``pair_pool`` — ``(out, mol_out, pro_out)`` with the two matrices handed back through the node where its backward launch can
    add their later gradients itself (``glam_pair_pool_add_supported``), the plain triple otherwise."""
    P, Q = msp.B, psp.B
    index = pair_index(pro_of_pair, P, Q, default="single" if Q == 1 and P != 1 else "identity")
    # (add_width: the adding form of glam_pair_pool_shared_bwd covers the widths of glam_pair_pool_bwd_add)
    return _apply_aliasing(_PairPoolShared, (mol_out, pro_out, msp, psp, index), mol_out, pro_out, with_identity,
                           add_width=mol_out.size(1) if with_identity else None)


class _PairRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, index):
        pidx = index.on(flat.device)
        order, qptr = index.by_protein().on(flat.device)
        ctx.save_for_backward(order, qptr)
        ctx.dims = (index.P, index.Q, tuple(flat.shape[1:]))
        return flat.index_select(0, pidx)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_rows):
        order, qptr = ctx.saved_tensors
        P, Q, tail = ctx.dims
        d_rows = f32c(d_rows, "d_rows")
        W = int(np.prod(tail, dtype=np.int64))
        if P == 0 or W == 0:
            return torch.zeros((Q,) + tail, dtype=torch.float32, device=d_rows.device), None
        d_flat = torch.empty((Q,) + tail, dtype=torch.float32, device=d_rows.device)
        _lib.api().glam_pair_rows_bwd(ptr(d_rows), ptr(order), ptr(qptr), P, Q, W, ptr(d_flat), stream())
        return d_flat, None


def pair_rows(flat, index):
    """``flat[index]`` -> ``[P, ...]``: the rows of a matrix that holds every protein once, one per pair (``index``: a ``PairIndex`` or
    what ``pair_index`` accepts, over ``flat.size(0)`` rows).  Its backward sums the pairs' rows per protein in batch order
    (``glam_pair_rows_bwd``): ``index_select``'s own backward is an atomic ``index_add``, whose bits change from run to run."""
    if not isinstance(index, PairIndex):
        index = pair_index(index, len(index), flat.size(0))
    elif index.Q != flat.size(0):
        raise IndexError(f"pair_rows: the index was validated over {index.Q} rows, the matrix has {flat.size(0)}")
    require_device(flat)
    if flat.dtype != torch.float32:
        raise GlamHipError(f"pair_rows: expected float32, got {flat.dtype}")
    return _PairRows.apply(flat, index)


# --------------------------------------------------------------------------------------
# drug x drug: the fusion with BOTH sides held once and both indexed (csrc/pairgather.hip, glam_pair_pool_gather_fwd)
# --------------------------------------------------------------------------------------
def pair_pool_gather(x1, x2, sp1, sp2, idx1=None, idx2=None, return_argmax=False):
    """``[max, mean]`` of ``x1[seg_a] @ x2[seg_b].T`` with ``a = idx1[i]``, ``b = idx2[i]`` -> ``[P, 2]``: ``pair_pool`` on two sets of
    small segments that are each held once (``sp1.B`` / ``sp2.B`` of them) — one wave per pair, one launch.  The max column — and with
    ``return_argmax`` the ``[P, 2]`` int32 rows of the maximum in ``x1`` / ``x2`` (-1 for an empty pair) — is bit for bit that of
    ``pair_pool`` on physically gathered rows; the mean is the same bits on every run and within the fp64-twin bound.
    ``idx1`` / ``idx2``: see ``pair_index``; ``None`` = identity on that side (needs ``sp.B == P``); ``P`` is the length of whichever is
    given.  Widths 1..128.  Inference only: there is no backward (training is ``ops.pair_pool`` on one graph per pair and side)."""
    Q1, Q2 = sp1.B, sp2.B
    P = pair_count(idx1, idx2, Q1)
    i1 = None if idx1 is None and Q1 == P else pair_index(idx1, P, Q1, name="idx1", over="segments of x1")
    i2 = None if idx2 is None and Q2 == P else pair_index(idx2, P, Q2, name="idx2", over="segments of x2")
    _inference_only("pair_pool_gather", (x1, x2), "the training route is ops.pair_pool on one graph per pair and side")
    x1, x2 = _operands("pair_pool_gather", x1, x2, sp1, sp2, "x1", "x2")
    D = x1.size(1)
    lib = _lib.api()
    if lib.glam_pair_pool_gather_load_bytes(ptr(x1), ptr(x2), D) == 0:
        raise GlamHipError(f"pair_pool_gather: width {D} is outside the kernel table (1..128)")
    out, arg, _, _ = _outputs((P,), x1.device, arg=return_argmax)
    lib.glam_pair_pool_gather_fwd(ptr(x1), ptr(x2), ptr(sp1.ptr), ptr(sp2.ptr), ptr(None if i1 is None else i1.on(x1.device)),
                                  ptr(None if i2 is None else i2.on(x1.device)), P, Q1, Q2, D, ptr(out), ptr(arg), stream())
    return (out, arg) if return_argmax else out


# --------------------------------------------------------------------------------------
# drug x drug, the whole table: every selected first-side segment against every selected second-side one, second-side-stationary with
# several small segments packed into the 64 lanes of a wave (csrc/pairgrid.hip, glam_pair_pool_grid_fwd)
# --------------------------------------------------------------------------------------
GRID_CHUNK = 64       # second-side rows per chunk (one per lane of the wave that holds them) = kStreamChunk of csrc/pairstream.h


class GridPlan(_Staged):
    """The work of one grid call over a validated column selection: ``sel`` int32 ``[Cs]`` (every entry in ``[0, Q)``) and ``work`` int32
    ``[256 * total_chunks + Cs + 1]``.  The selection is laid out in selection order, greedily: consecutive whole segments share a chunk
    while their rows fit in its 64 lanes; a segment of more than 64 rows closes the running chunk and takes ``ceil(n / 64)`` slices of
    its own (its last slice is not shared); an empty segment takes no lane.  ``work`` holds, per chunk and lane, four int32 —
    ``(row of x2 the lane holds, b: that row inside its segment, n2: rows of that segment, partial: where the lane's best goes)`` with
    ``partial = part_ptr[j] + slice`` for a lane of selection ``j`` and ``-1`` for an idle lane (which holds the row of lane 0 and
    ``b = n2 = 0``); the lanes of one partial are contiguous — then ``part_ptr[Cs + 1]``, the offsets of the selections' partials (one
    per whole segment, ``ceil(n / 64)`` for a sliced one, none for an empty one; ``n_partials`` in all).  ``lanes`` ``[total_chunks, 64,
    4]`` / ``part_ptr`` are views of ``work``; ``fill`` is the mean share of a chunk's lanes that hold a row.  A duplicate of the
    selection gets lanes and partials of its own.  Host numpy; ``on(device)`` -> ``(sel, work)`` on the device, made once per device
    (one copy out of pinned memory, only enqueued) and shared by every launch that reads them."""

    def __init__(self, sel, sizes):
        self.sel, self.Cs, self.Q = sel, int(sel.shape[0]), int(sizes.shape[0])
        first, self.N = _first_rows(sizes, "grid_plan: the segments hold 2^31 rows or more")
        n = sizes[sel]                                                               # rows per selection
        part_ptr = np.zeros(self.Cs + 1, dtype=np.int64)
        np.cumsum((n + GRID_CHUNK - 1) // GRID_CHUNK, out=part_ptr[1:])
        if int(part_ptr[-1]) >= 2 ** 31 - 1 or int(n.sum()) >= 2 ** 31 - 1:
            raise IndexError("grid_plan: the selection has 2^31 rows or partials or more")
        self.n_partials = int(part_ptr[-1])
        # the greedy walk: chunk and first lane of every selection (one pass over the selection; the rows are filled in below, at once)
        chunk, lane0 = np.zeros(self.Cs, dtype=np.int64), np.zeros(self.Cs, dtype=np.int64)
        c = used = 0                                                                 # the running chunk and its lanes in use
        for j, nj in enumerate(n.tolist()):
            if nj == 0:
                continue
            if used and (nj > GRID_CHUNK or used + nj > GRID_CHUNK):                 # does not fit behind (or never shares): close it
                c, used = c + 1, 0
            chunk[j], lane0[j] = c, used
            if nj >= GRID_CHUNK:
                c, used = c + (nj + GRID_CHUNK - 1) // GRID_CHUNK, 0                 # whole slices: nothing shares the last one
            else:
                used += nj
        self.total_chunks = T = c + (1 if used else 0)
        if T * GRID_CHUNK * 4 >= 2 ** 31 - 1:
            raise IndexError("grid_plan: the selection's table has 2^31 entries or more")
        j = np.repeat(np.arange(self.Cs, dtype=np.int64), n)
        k = np.arange(j.shape[0], dtype=np.int64) - (np.cumsum(n) - n)[j]            # row inside its segment
        table = np.zeros((T * GRID_CHUNK, 4), dtype=np.int32)
        table[:, 3] = -1
        at = chunk[j] * GRID_CHUNK + lane0[j] + k                                    # (a sliced segment starts at lane 0 and runs on)
        table[at, 0], table[at, 1], table[at, 2] = first[sel[j]] + k, k, n[j]
        table[at, 3] = part_ptr[j] + k // GRID_CHUNK
        table = table.reshape(T, GRID_CHUNK, 4)
        idle = table[:, :, 3] < 0
        table[:, :, 0] = np.where(idle, table[:, :1, 0], table[:, :, 0])             # an idle lane reads the row of lane 0
        self.fill = float(j.shape[0]) / (T * GRID_CHUNK) if T else 0.0
        self.work = np.concatenate([table.reshape(-1), part_ptr.astype(np.int32)])
        self.lanes, self.part_ptr = self.work[:4 * GRID_CHUNK * T].reshape(T, GRID_CHUNK, 4), self.work[4 * GRID_CHUNK * T:]
        _Staged.__init__(self, "the grid's selection and lane table", self.sel, self.work)


def grid_plan(sizes_host, cols=None):
    """``GridPlan`` of the column selection ``cols`` over ``Q = len(sizes_host)`` segments of ``sizes_host[q]`` rows — host only (numpy),
    before anything is launched (the kernel trusts the table; the policy of ``panel_plan``).  ``cols``: ``None`` = all ``Q`` in order,
    or a host sequence / numpy array / CPU tensor of integers in ``[0, Q)``, in any order, duplicates allowed; ``IndexError`` for a
    wrong dtype or an entry outside ``[0, Q)``; a device tensor is refused (validating it would be a hidden read-back)."""
    sizes = _plan_sizes("grid_plan", sizes_host, "the segments' sizes")
    return GridPlan(_plan_selection("cols", "be a vector of segment numbers", cols, int(sizes.shape[0])), sizes)


def pair_pool_grid(x1, x2, sp1, sp2, plan, rows=None, sum1=None, sum2=None, return_argmax=False, slab=0):
    """``[max, mean]`` of ``x1[seg_a] @ x2[seg_q].T`` for EVERY selected first-side segment ``a = rows[i]`` and every selected second-side
    segment ``q = plan.sel[j]`` -> ``[R, Cs, 2]``: the table of ``R * Cs`` pairs of ``pair_pool_gather`` from one second-side-stationary
    launch (+ a finish launch) in which several small segments share the 64 lanes of a wave.  The max column — and with
    ``return_argmax`` the ``[R, Cs, 2]`` int32 rows of the maximum in ``x1`` / ``x2`` (-1 for an empty segment on either side) — is bit
    for bit that of ``pair_pool_gather`` on those pairs; the mean is ``<sum1[a], sum2[q]> / (n_a n_q)``, within the fp64-twin bound
    (and, for ``rows=None``, the bits of ``pair_pool_panel``).  ``plan``: ``grid_plan`` over the sizes of ``sp2``'s segments.  ``rows``:
    host integers in ``[0, sp1.B)``, any order, duplicates allowed (``pair_index``); ``None`` = all of ``sp1.B`` in order.  ``sum1``
    ``[Q1, D]`` / ``sum2`` ``[Q2, D]``: the segments' column sums (``segment_pool(x, sp, "sum")``), computed here when missing — a
    caller that keeps the segments keeps their sums too.  ``slab``: first-side segments per wave, 0 = the library chooses.  Widths
    1..128.  Inference only: there is no backward (training is ``ops.pair_pool`` / ``ops.pair_pool_gather_shared``)."""
    _require_plan("pair_pool_grid", plan, GridPlan, "grid_plan")
    Q1, Q2, Cs = sp1.B, sp2.B, plan.Cs
    R = pair_count(rows, None, Q1)
    index = None if rows is None else pair_index(rows, R, Q1, name="rows", over="drugs")        # host-side, before the first launch
    _inference_only("pair_pool_grid", (x1, x2, sum1, sum2), "the training routes are ops.pair_pool on one graph per pair and side and "
                    "ops.pair_pool_gather_shared on segments held once")
    if plan.Q != Q2 or plan.N != sp2.N:
        raise GlamHipError(f"pair_pool_grid: the plan was made for {plan.Q} segments of {plan.N} rows, the second side holds {Q2} of {sp2.N}")
    x1, x2 = _operands("pair_pool_grid", x1, x2, sp1, sp2, "x1", "x2")
    D, dev = x1.size(1), x1.device
    _check_sums_slab("pair_pool_grid", D, dev, (("sum1", sum1, Q1), ("sum2", sum2, Q2)), slab, "first-side segments")
    lib = _lib.api()
    if _lib.load().glam_pair_pool_grid_supported(D) != 0:           # (a status: the raw binding hands it back)
        raise GlamHipError(f"pair_pool_grid: width {D} is outside the kernel table (1..128)")
    out, arg, _, _ = _outputs((R, Cs), dev, arg=return_argmax)
    if R and Cs and (sp1.N == 0 or sp2.N == 0):          # no row on one side
        _all_empty(out, arg)
    elif R and Cs:
        sum1 = f32c(sum1, "sum1") if sum1 is not None else segment_pool(x1, sp1, "sum")
        sum2 = f32c(sum2, "sum2") if sum2 is not None else segment_pool(x2, sp2, "sum")
        sel, work = plan.on(dev)
        ws = _workspace(lib.glam_pair_pool_grid_workspace_bytes(plan.n_partials, R), dev)
        lib.glam_pair_pool_grid_fwd(ptr(x1), ptr(x2), ptr(sp1.ptr), ptr(sp2.ptr), ptr(None if index is None else index.on(dev)), R,
                                    ptr(sel), Cs, ptr(work), plan.total_chunks, plan.n_partials, Q1, Q2, D, ptr(sum1), ptr(sum2),
                                    int(slab), ptr(out), ptr(arg), ptr(ws), ws.numel(), stream())
    return (out, arg) if return_argmax else out


# --------------------------------------------------------------------------------------
# training on drugs held once: the gathered fusion with a backward (csrc/pairgather.hip train_fwd, csrc/pairgather_bwd.hip)
# --------------------------------------------------------------------------------------
class _PairPoolGatherShared(torch.autograd.Function):
    """``i1`` / ``i2``: the validated ``PairIndex`` of each side (an identity side too: its by-drug lists are read by the backward);
    ``null1`` / ``null2``: hand the kernels a NULL index on that side (identity)."""

    @staticmethod
    def forward(ctx, x1, x2, sp1, sp2, i1, i2, null1, null2, with_identity=False):
        x1_in, x2_in = x1, x2
        x1, x2 = _operands("pair_pool_gather_shared", x1, x2, sp1, sp2, "x1", "x2")
        P, Q1, Q2, D, dev = i1.P, sp1.B, sp2.B, x1.size(1), x1.device
        # (the table in Python: the training entry points have no query, and their dword form takes every alignment)
        if not 1 <= D <= 128:
            raise GlamHipError(f"pair_pool_gather_shared: width {D} is outside the kernel table (1..128)")
        d1, d2 = i1.on(dev), i2.on(dev)
        order1, lptr1 = i1.by_protein().on(dev)
        order2, lptr2 = i2.by_protein().on(dev)
        out, arg, sums, _ = _outputs((P,), dev, D=D)
        ctx.rows = x1.size(0) > 0 and x2.size(0) > 0
        if ctx.rows:
            _lib.api().glam_pair_pool_gather_train_fwd(ptr(x1), ptr(x2), ptr(sp1.ptr), ptr(sp2.ptr), ptr(None if null1 else d1),
                                                       ptr(None if null2 else d2), P, Q1, Q2, D, ptr(out), ptr(arg), ptr(sums), stream())
        else:                # no row on one side
            _all_empty(out, arg)
        ctx.save_for_backward(x1, x2, arg, sums, d1, d2, order1, lptr1, order2, lptr2)
        ctx.sps, ctx.null, ctx.P = (sp1, sp2), (bool(null1), bool(null2)), P
        return _alias_fwd(ctx, out, x1_in, x2_in, with_identity)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_a1=None, d_a2=None):
        x1, x2, arg, sums, d1, d2, order1, lptr1, order2, lptr2 = ctx.saved_tensors
        sp1, sp2 = ctx.sps
        none = (None,) * 7
        # (no pair, or only empty ones: the entry point writes nothing)
        launch, d_out, d_a1, d_a2 = _alias_bwd(d_out, d_a1, d_a2, x1, x2, "x1", "x2", nothing_written=ctx.P == 0 or not ctx.rows)
        if not launch:
            return (d_a1, d_a2) + none
        d_x1, d_x2 = torch.empty_like(x1), torch.empty_like(x2)
        _lib.api().glam_pair_pool_gather_bwd(ptr(x1), ptr(x2), ptr(sp1.ptr), ptr(sp2.ptr), ptr(None if ctx.null[0] else d1),
                                             ptr(None if ctx.null[1] else d2), ptr(order1), ptr(lptr1), ptr(order2), ptr(lptr2), ptr(arg),
                                             ptr(sums), ptr(d_out), ctx.P, sp1.B, sp2.B, x1.size(1), ptr(d_a1), ptr(d_a2), ptr(d_x1),
                                             ptr(d_x2), stream())
        return (d_x1, d_x2) + none


def pair_pool_gather_shared(x1, x2, sp1, sp2, idx1=None, idx2=None, with_identity=False):
    """``pair_pool_gather`` WITH a backward: ``[max, mean]`` of ``x1[seg_a] @ x2[seg_b].T`` with ``a = idx1[i]``, ``b = idx2[i]`` ->
    ``[P, 2]`` on two sets of small segments that are each held once, for training.  The forward is bit for bit ``pair_pool_gather``; the
    gradient of a segment's rows — on EITHER side — is the sum over every pair that points at it, taken in batch order without atomics
    (two runs are bit-equal, one launch for both sides); a segment no pair references gets zeros.  ``idx1`` / ``idx2``: as
    ``pair_pool_gather`` (``pair_index``; ``None`` = identity on that side, needs ``sp.B == P``); keep ONE ``PairIndex`` per side across
    the steps that use it — its device copies are made on the first, eager, visit and a hipGraph capture needs them to exist.  Widths
    1..128.  ``with_identity``: as ``pair_pool`` — ``(out, x1, x2)`` with the two matrices handed back through the node (both require
    grad, fp32): its backward launch then adds their later gradients itself; the plain triple otherwise."""
    P = pair_count(idx1, idx2, sp1.B)
    i1 = pair_index(idx1, P, sp1.B, name="idx1", over="segments of x1")
    i2 = pair_index(idx2, P, sp2.B, name="idx2", over="segments of x2")
    # (no add_width: glam_pair_pool_gather_bwd adds inside its launch for every width of its table)
    return _apply_aliasing(_PairPoolGatherShared, (x1, x2, sp1, sp2, i1, i2, idx1 is None, idx2 is None), x1, x2, with_identity)


# --------------------------------------------------------------------------------------
# interaction maps: per-row marginals of every pair's score matrix, both sides from one launch (csrc/pairmap.hip, glam_pair_map_fwd)
# --------------------------------------------------------------------------------------
MAP_CHUNK = 64        # owner rows per work item (one per lane of the wave that holds them) = kStreamChunk of csrc/pairstream.h


class MapPlan(_Staged):
    """The work of one map call over two validated indices (``None`` = identity): pair ``i`` is segment ``a = idx1[i]`` of the first side
    against segment ``b = idx2[i]`` of the second.  ``out_ptr1`` / ``out_ptr2`` int32 ``[P + 1]``: the offsets of the pairs' rows in the
    ragged, pair-major outputs of side 1 / side 2 (the cumulative sizes through the indices; ``R1`` / ``R2`` rows in all).  ``work`` int32
    ``[n_items, 4]``: per item ``(a, b, 2 * chunk + side, first output row of the chunk)`` — the owner rows ``64 * chunk .. 64 * chunk + 63``
    of segment ``a`` (side 0) or ``b`` (side 1); every owner row of every pair is in exactly one item, a pair's items are consecutive
    (side 0 first; ``pair_of_item`` int32 ``[n_items]`` names it, host only), and a pair whose partner segment is empty keeps its items:
    the kernel fills their rows.  ``Q1`` / ``Q2`` / ``N1`` /
    ``N2``: the segments and rows the sizes spoke of.  Host numpy; ``on(device)`` -> ``(work, out_ptr1, out_ptr2)`` on the device, made
    once per device (one copy out of pinned memory, only enqueued) and shared by every launch that reads them."""

    def __init__(self, sizes1, sizes2, a, b):
        self.P, self.Q1, self.Q2 = int(a.shape[0]), int(sizes1.shape[0]), int(sizes2.shape[0])
        self.N1, self.N2 = int(sizes1.sum()), int(sizes2.sum())
        n = (sizes1[a], sizes2[b])                                                   # rows per pair and side
        out_ptr = [np.zeros(self.P + 1, dtype=np.int64), np.zeros(self.P + 1, dtype=np.int64)]
        for side in (0, 1):
            np.cumsum(n[side], out=out_ptr[side][1:])
        self.R1, self.R2 = int(out_ptr[0][-1]), int(out_ptr[1][-1])
        n_chunks = [(n[side] + MAP_CHUNK - 1) // MAP_CHUNK for side in (0, 1)]       # per pair
        self.n_items = int(n_chunks[0].sum() + n_chunks[1].sum())
        if max(self.N1, self.N2, self.R1, self.R2, self.n_items) >= 2 ** 31 - 1:
            raise IndexError("map_plan: the segments, the outputs or the work table hold 2^31 rows or more")
        parts = []
        for side in (0, 1):
            first = np.cumsum(n_chunks[side]) - n_chunks[side]
            i = np.repeat(np.arange(self.P, dtype=np.int64), n_chunks[side])
            c = np.arange(i.shape[0], dtype=np.int64) - first[i]                     # chunk inside its segment
            parts.append(np.stack([i, a[i], b[i], 2 * c + side, out_ptr[side][i] + MAP_CHUNK * c], axis=1))
        table = np.concatenate(parts)
        table = table[np.argsort(table[:, 0], kind="stable")]                       # pair-major: a pair's two sides run side by side
        self.pair_of_item = table[:, 0].astype(np.int32)
        self.work = np.ascontiguousarray(table[:, 1:], dtype=np.int32)
        self.out_ptr1, self.out_ptr2 = out_ptr[0].astype(np.int32), out_ptr[1].astype(np.int32)
        _Staged.__init__(self, "the map's work table and output offsets", self.work.reshape(-1),
                         np.concatenate([self.out_ptr1, self.out_ptr2]))

    def on(self, device):
        work, out_ptr = _Staged.on(self, device)
        return work, out_ptr[:self.P + 1], out_ptr[self.P + 1:]


def map_plan(sizes1_host, sizes2_host, idx1=None, idx2=None):
    """``MapPlan`` of the pairs ``(idx1[i], idx2[i])`` over ``Q1 = len(sizes1_host)`` first-side segments of ``sizes1_host[q]`` rows and
    ``Q2 = len(sizes2_host)`` second-side ones — host only (numpy), before anything is launched (the kernel trusts the table; the policy
    of ``pair_index`` / ``grid_plan``).  ``idx1`` / ``idx2``: see ``pair_index`` — host integers, any order, duplicates allowed; ``None`` =
    identity on that side (needs ``Q == P``); ``P`` is the length of whichever is given.  ``IndexError`` for a wrong length or dtype or an
    entry outside the range; a device tensor is refused (validating it would be a hidden read-back)."""
    sizes = [_plan_sizes("map_plan", s, f"the sizes of side {k}") for k, s in ((1, sizes1_host), (2, sizes2_host))]
    Q1, Q2 = int(sizes[0].shape[0]), int(sizes[1].shape[0])
    P = pair_count(idx1, idx2, Q1)
    instead = "the host integers that were loaded into it (or the ops.pair_index of them)"
    a = host_index(pair_index(idx1, P, Q1, name="idx1", over="segments of x1"), "map_plan", instead).astype(np.int64)
    b = host_index(pair_index(idx2, P, Q2, name="idx2", over="segments of x2"), "map_plan", instead).astype(np.int64)
    return MapPlan(sizes[0], sizes[1], a, b)


@dataclasses.dataclass
class PairMap:
    """What ``pair_map`` returns, ragged and pair-major.  Side 1 (``[R1]``, the rows of pair ``i`` at ``out_ptr1[i] : out_ptr1[i + 1]``): per
    row ``r1`` of the pair's first segment ``max1`` = the largest score of the row, ``arg1`` int32 = the row of ``x2`` of the first partner row
    that attains it, ``mean1`` = the mean of the row's scores.  Side 2 (``[R2]``, ``out_ptr2``): the same per row of the second segment, ``arg2``
    a row of ``x1``.  An empty partner: 0, -1, 0.  ``out_ptr1`` / ``out_ptr2``: int32 ``[P + 1]`` on the device."""
    max1: torch.Tensor
    arg1: torch.Tensor
    mean1: torch.Tensor
    max2: torch.Tensor
    arg2: torch.Tensor
    mean2: torch.Tensor
    out_ptr1: torch.Tensor
    out_ptr2: torch.Tensor


def pair_map(x1, x2, sp1, sp2, plan):
    """The two marginals of ``S = x1[seg_a] @ x2[seg_b].T`` for every pair of ``plan`` (``map_plan`` over the sizes of ``sp1``'s and
    ``sp2``'s segments) -> ``PairMap``: per row of the first segment the best partner row and the mean over the partner's rows, per row
    of the second the same the other way — ``S`` is never stored, both sides come from ONE launch.  A score is the fmaf chain of
    ``pair_pool_gather``: the largest ``max1`` (or ``max2``) of a pair is bit for bit its max column, and the first row that holds it
    with its ``arg1`` is its argmax.  Ties go to the smallest partner row.  The means are the same bits on every run and within the
    fp64-twin bound.  Widths 1..128.  Inference only: there is no backward."""
    _require_plan("pair_map", plan, MapPlan, "map_plan")
    _inference_only("pair_map", (x1, x2), "the training route is ops.pair_pool on one graph per pair and side")
    if (plan.Q1, plan.N1, plan.Q2, plan.N2) != (sp1.B, sp1.N, sp2.B, sp2.N):
        raise GlamHipError(f"pair_map: the plan was made for {plan.Q1} segments of {plan.N1} rows against {plan.Q2} of {plan.N2}, the "
                           f"operands hold {sp1.B} of {sp1.N} against {sp2.B} of {sp2.N}")
    x1, x2 = _operands("pair_map", x1, x2, sp1, sp2, "x1", "x2")
    D, dev = x1.size(1), x1.device
    if not 1 <= D <= 128:
        raise GlamHipError(f"pair_map: width {D} is outside the kernel table (1..128)")
    work, out_ptr1, out_ptr2 = plan.on(dev)
    # (never an empty buffer: it has no address, and a call whose owner rows all sit on ONE side still launches — for the fills)
    bufs = [(torch.empty(max(R, 1), dtype=torch.float32, device=dev), torch.empty(max(R, 1), dtype=torch.int32, device=dev),
             torch.empty(max(R, 1), dtype=torch.float32, device=dev)) for R in (plan.R1, plan.R2)]
    sides = [tuple(t[:R] for t in side) for side, R in zip(bufs, (plan.R1, plan.R2))]
    if plan.n_items and (sp1.N == 0 or sp2.N == 0):      # no row on one side: every partner is empty
        for mx, arg, mean in sides:
            _all_empty(mx, arg)
            mean.zero_()
    elif plan.n_items:
        _lib.api().glam_pair_map_fwd(ptr(x1), ptr(x2), ptr(sp1.ptr), ptr(sp2.ptr), ptr(work), plan.n_items, D,
                                     *[ptr(t) for side in bufs for t in side], stream())
    return PairMap(*sides[0], *sides[1], out_ptr1, out_ptr2)


# --------------------------------------------------------------------------------------
# the head over a table: both linear layers without the [pairs, e_dim] hidden matrix (csrc/pairhead.hip, glam_pair_head_fwd)
# --------------------------------------------------------------------------------------
_HEAD_ACTS = {"none": 0, "relu": 1, "leaky": 2}
HEAD_MAX_OUT, HEAD_MAX_F = 8, 16          # = kHeadMaxOut / kHeadMaxF of csrc/pairhead.hip


def _weight_bias(lin, name, who="pair_head"):
    """``(weight, bias)`` of ``lin`` — a ``torch.nn.Linear`` or the pair of tensors itself."""
    if isinstance(lin, torch.nn.Linear):
        return lin.weight, lin.bias
    if isinstance(lin, (tuple, list)) and len(lin) == 2 and all(torch.is_tensor(t) for t in lin):
        return lin[0], lin[1]
    raise GlamHipError(f"{who}: {name} must be a torch.nn.Linear with a bias or its (weight, bias) tensors, got {type(lin).__name__}")


def _rows_view(t, name):
    """A 2-D fp32 matrix whose rows are contiguous, as it is (a ``[n, C]`` view of padded rows keeps its leading dimension), else its
    contiguous copy."""
    if t.dtype != torch.float32:
        raise GlamHipError(f"{name}: expected float32, got {t.dtype}")
    return t if t.stride(1) == 1 and t.stride(0) >= t.size(1) else t.contiguous()


def _head_operands(who, flat_a, flat_b, f, lin0, lin1, act, slope, out_lo, out_hi, host_checks=None):
    """The argument checks the table heads share (``pair_head``, ``pair_head_classes``), in one order and with one wording -> ``(lead, held,
    R, Cs, e_dim, out_dim)``: the 18 leading arguments of both entry points and the tensors they point into (kept by the caller until
    its launch is enqueued).  ``host_checks(out_dim)`` runs before anything needs a device."""
    w0, b0 = _weight_bias(lin0, "lin0", who)
    w1, b1 = _weight_bias(lin1, "lin1", who)
    if b0 is None or b1 is None:
        raise GlamHipError(f"{who}: both linear layers must have a bias")
    if host_checks is not None and w1.dim() == 2:
        host_checks(w1.size(0))
    given = (flat_a, flat_b, f, w0, b0, w1, b1)
    _inference_only(who, given, "the head that trains is the listed one — head=\"rows\" of score_matrix / screen_panel, and model(...) / "
                    "forward_shared for the training calls")
    require_device(*given)
    if act not in _HEAD_ACTS:
        raise GlamHipError(f"{who}: act = {act!r} is not one of 'none', 'relu', 'leaky'")
    if flat_a.dim() != 2 or flat_b.dim() != 2 or flat_a.size(1) != flat_b.size(1) or flat_a.size(1) < 1:
        raise GlamHipError(f"{who}: the two sides disagree (width): flat_a {tuple(flat_a.shape)}, flat_b {tuple(flat_b.shape)}")
    R, Cs, hid = flat_a.size(0), flat_b.size(0), flat_a.size(1)
    if f is not None and (f.dim() != 3 or tuple(f.shape[:2]) != (R, Cs)):
        raise GlamHipError(f"{who}: f must be [{R}, {Cs}, F] (or None for F = 0), got {tuple(f.shape)}")
    F = 0 if f is None else f.size(2)
    if w0.dim() != 2 or w0.size(1) != 2 * hid + F or tuple(b0.shape) != (w0.size(0),) or w0.size(0) < 1:
        raise GlamHipError(f"{who}: lin0 must map 2 * {hid} + {F} = {2 * hid + F} columns and carry one bias per output, got weight "
                           f"{tuple(w0.shape)}, bias {tuple(b0.shape)}")
    e_dim = w0.size(0)
    if w1.dim() != 2 or w1.size(1) != e_dim or tuple(b1.shape) != (w1.size(0),):
        raise GlamHipError(f"{who}: lin1 must map the {e_dim} outputs of lin0 and carry one bias per output, got weight "
                           f"{tuple(w1.shape)}, bias {tuple(b1.shape)}")
    out_dim = w1.size(0)
    if not out_lo <= out_dim <= out_hi:
        raise GlamHipError(f"{who}: out_dim = {out_dim} is outside {out_lo}..{out_hi} (head=\"rows\" takes any)")
    if F > HEAD_MAX_F:
        raise GlamHipError(f"{who}: F = {F} fusion columns are outside 0..{HEAD_MAX_F} (head=\"rows\" takes any)")
    if R * Cs >= 2 ** 31 - 1:
        raise GlamHipError(f"{who}: a table of {R} x {Cs} pairs holds 2^31 - 1 entries or more: score it in blocks of rows")
    a, b = _rows_view(flat_a, "flat_a"), _rows_view(flat_b, "flat_b")
    w0 = _rows_view(w0, "lin0.weight")
    w1, b0, b1 = f32c(w1, "lin1.weight"), f32c(b0, "lin0.bias"), f32c(b1, "lin1.bias")
    f = None if F == 0 else f32c(f, "f")
    lead = (ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(f), R, Cs, hid, F, ptr(w0), w0.stride(0), ptr(b0), e_dim, ptr(w1), ptr(b1), out_dim,
            _HEAD_ACTS[act], float(slope))
    return lead, (a, b, f, w0, b0, w1, b1), R, Cs, e_dim, out_dim


def pair_head(flat_a, flat_b, f, lin0, lin1, act="none", slope=0.0):
    """``lin1(act(lin0(cat[flat_a[i], flat_b[j], f[i, j]])))`` for EVERY ``i`` and ``j`` -> ``[R, Cs, out_dim]``: the two linear layers of a pair
    model's head over a table, without the ``[R * Cs, 2 hid + F]`` input rows and the ``[R * Cs, e_dim]`` hidden matrix — the first layer
    separates into ``A[i] + B[j] + Wf f[i, j]`` and only the ``F`` fusion columns are per pair (two launches: ``k_pair_head_side``,
    ``k_pair_head``).  ``flat_a`` ``[R, hid]`` / ``flat_b`` ``[Cs, hid]``: as they are, views of padded rows included; ``f`` ``[R, Cs, F]`` or
    ``None`` for ``F = 0``; ``lin0`` / ``lin1``: the two ``torch.nn.Linear`` (``2 hid + F -> e_dim -> out_dim``) or their ``(weight, bias)``;
    ``act``: ``"none"``, ``"relu"`` or ``"leaky"`` with ``slope`` (an ``RReLU`` in ``eval()`` is a leaky of its mean slope).  An entry is
    one fixed chain of its own ``(flat_a[i], flat_b[j], f[i, j])``: the same bits whatever the rest of the table is.  ``out_dim`` in 1..8,
    ``F`` in 0..16, ``R * Cs < 2^31 - 1``.  Inference only: there is no backward (a head that trains is the listed one: ``head="rows"`` of
    the table calls, ``model(...)`` / ``forward_shared`` for training)."""
    lead, _held, R, Cs, e_dim, out_dim = _head_operands("pair_head", flat_a, flat_b, f, lin0, lin1, act, slope, 1, HEAD_MAX_OUT)
    out = torch.empty(R, Cs, out_dim, dtype=torch.float32, device=flat_a.device)
    if R and Cs:
        lib = _lib.api()
        ws = _workspace(lib.glam_pair_head_workspace_bytes(R, Cs, e_dim), out.device)
        lib.glam_pair_head_fwd(*lead, ptr(ws), ws.numel(), ptr(out), stream())
    return out


# --------------------------------------------------------------------------------------
# the class table: called class, its log-probability and selected log-probabilities, for any out_dim (glam_pair_head_classes_fwd)
# --------------------------------------------------------------------------------------
HEAD_CLASS_TILE, HEAD_MAX_CLASSES, HEAD_MAX_SEL = 16, 1024, 8          # = kClassTile / kHeadMaxClasses / kMaxSel of csrc/pairhead.hip


class ClassTable(typing.NamedTuple):
    """``cls`` int32 ``[R, Cs]``: the called class (``torch.argmax`` of the logits); ``logp`` ``[R, Cs]``: its log-softmax; ``sel``
    ``[R, Cs, S]``: the log-softmax of the ``S`` selected classes, in the order given; ``logits`` ``[R, Cs, out_dim]`` or ``None``."""
    cls: torch.Tensor
    logp: torch.Tensor
    sel: torch.Tensor
    logits: typing.Optional[torch.Tensor]


def class_selection(classes, out_dim, who="pair_head_classes"):
    """``classes`` as a list of host ints in ``[0, out_dim)``, at most ``HEAD_MAX_SEL`` of them (duplicates allowed, order kept), or the
    refusal."""
    sel = host_ints(classes, "classes", "be a vector of class indices", below=out_dim,
                    on_device=f"{who}: classes lives on a device: it is a host sequence of at most {HEAD_MAX_SEL} class indices")
    if sel.shape[0] > HEAD_MAX_SEL:
        raise GlamHipError(f"{who}: {sel.shape[0]} selected classes, the kernel catches at most {HEAD_MAX_SEL} per call (return_logits / "
                           "logits=True hands out all of them)")
    return [int(c) for c in sel]


def pair_head_classes(flat_a, flat_b, f, lin0, lin1, act="none", slope=0.0, classes=(), logits=False):
    """The head of ``pair_head`` read as a classifier, for ANY ``out_dim`` in 2..1 024 -> ``ClassTable(cls, logp, sel, logits)``: per pair
    the called class (``torch.argmax`` of the logits: a NaN is the largest, of equal logits the smallest index), its log-softmax, and the
    log-softmax of the classes ``classes`` names (host ints in ``[0, out_dim)``, at most 8, duplicates allowed, order kept) — from the side
    launch and ONE ``k_pair_head_classes``, which walks the classes in tiles of ``HEAD_CLASS_TILE`` and keeps a running maximum and sum:
    neither the ``[R * Cs, e_dim]`` hidden matrix nor, unless ``logits=True`` asks for it, the ``[R, Cs, out_dim]`` table exists.  A logit
    is ``pair_head``'s chain bit for bit; an entry's four results are one fixed sequence of its own ``(flat_a[i], flat_b[j], f[i, j])``.
    ``logp`` / ``sel`` are NaN where a logit is NaN (``torch.log_softmax``).  Arguments, checks and limits otherwise as ``pair_head``
    (``F`` in 0..16, ``R * Cs < 2^31 - 1``, inference only, empty tables without a launch)."""
    who = "pair_head_classes"
    chosen = []
    lead, _held, R, Cs, e_dim, out_dim = _head_operands(
        who, flat_a, flat_b, f, lin0, lin1, act, slope, 2, HEAD_MAX_CLASSES, lambda n: chosen.extend(class_selection(classes, n, who)))
    dev = flat_a.device
    S = len(chosen)
    cls = torch.empty(R, Cs, dtype=torch.int32, device=dev)
    logp = torch.empty(R, Cs, dtype=torch.float32, device=dev)
    sel = torch.empty(R, Cs, S, dtype=torch.float32, device=dev)
    table = torch.empty(R, Cs, out_dim, dtype=torch.float32, device=dev) if logits else None
    if R and Cs:
        lib = _lib.api()
        ws = _workspace(lib.glam_pair_head_classes_workspace_bytes(R, Cs, e_dim, out_dim), dev)
        lib.glam_pair_head_classes_fwd(*lead, (ctypes.c_int * max(S, 1))(*chosen), S, ptr(ws), ws.numel(), ptr(cls), ptr(logp),
                                       ptr(sel) if S else None, ptr(table), stream())
    return ClassTable(cls, logp, sel, table)
