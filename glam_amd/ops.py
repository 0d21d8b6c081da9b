"""Functional ops over ``libglam_hip.so`` with autograd (host side of the C ABI).

Every function launches hand-written gfx950 kernels on torch's *current* HIP stream; PyTorch
only supplies device memory, the stream and the autograd tape.  There is no CPU path.

``GraphIndex`` is the CSR staging of one ``edge_index`` (by target for the forward gather, by
source — the transpose — for the backward scatter); it is cached per ``edge_index`` tensor
because the reference re-uses one edge list for every message step (``src_1gp/model.py:53-54``)
and its train loader does not shuffle (``src_1gp/trainer.py:37-38``).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import math
import os
import weakref

import torch

from . import _lib
from ._lib import GlamHipError, check, f32c, ptr, require_device, stream     # noqa: F401  (check: for callers of the raw binding, as ops.check)
from ._memo import TensorMemo


# --------------------------------------------------------------------------------------
# CSR staging
# --------------------------------------------------------------------------------------
# --------------------------------------------------------------------------------------
# id validation of foreign batches
# --------------------------------------------------------------------------------------
# Tensors collated by glam_amd.data carry trust marks and are never read back.  Anything else (a PyG ``Batch``, hand-built
# tensors) has its node / graph ids range-checked ON THE DEVICE while the CSR / ptr is built (bad entries are dropped there: no
# out-of-bounds access either way); what remains is when the host learns about a raised flag:
#   "sync"      (default) read the flag back at once: IndexError at the call that staged the tensor, like torch's own index checks
#               on CPU — one host sync per NEW tensor (cached afterwards);
#   "deferred"  copy the flag to pinned host memory asynchronously and raise at the next staging call, at ``check_pending()`` or at
#               the end of ``Architecture.forward`` once the copy has landed — no host sync on the step (CUDA's own convention for
#               device-side errors: reported late, never lost as long as the program keeps calling into the library);
#   "off"       never look (the reference on a GPU: a device-side assert or silent garbage).
VALIDATE = os.environ.get("GLAM_VALIDATE", "sync")
_PENDING: collections.deque = collections.deque()
_PINNED_FLAGS: list = []


def _check_flag(err, message):
    if VALIDATE == "off":
        return
    if VALIDATE == "deferred" and not torch.cuda.is_current_stream_capturing():
        host = _PINNED_FLAGS.pop() if _PINNED_FLAGS else torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(err, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _PENDING.append((ev, host, message))
        return
    if int(err.item()) != 0:
        raise IndexError(message)


def poll_checks(block=False):
    """Raise the IndexError of a deferred id check whose flag has come back (``block``: wait for all of them)."""
    while _PENDING:
        ev, host, message = _PENDING[0]
        if block:
            ev.synchronize()
        elif not ev.query():
            return
        _PENDING.popleft()
        bad = int(host[0]) != 0
        _PINNED_FLAGS.append(host)
        if bad:
            raise IndexError(message + " (deferred check, GLAM_VALIDATE=deferred: raised after the call that staged the tensor)")


def check_pending():
    """Wait for every outstanding deferred id check and raise if one failed."""
    poll_checks(block=True)


class GraphIndex:
    """CSR-by-target ``(rowptr, src, eid)`` and CSR-by-source ``(colptr, dst, eid_t)`` of an
    int64 ``edge_index[2,E]`` over ``N`` nodes (PyG flow source_to_target: row 0 = source j,
    row 1 = target i).  int32, device resident, stable inside every segment."""

    def __init__(self, edge_index, num_nodes, validate=True):
        require_device(edge_index)
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise GlamHipError(f"edge_index must be int64 [2,E], got {edge_index.dtype} {tuple(edge_index.shape)}")
        ei = edge_index if edge_index.is_contiguous() else edge_index.contiguous()
        self.N, self.E = int(num_nodes), int(ei.size(1))
        self.device = ei.device
        lib = _lib.api()
        dev = ei.device
        i32 = dict(dtype=torch.int32, device=dev)
        self.rowptr = torch.empty(self.N + 1, **i32)
        self.src = torch.empty(self.E, **i32)
        self.eid = torch.empty(self.E, **i32)
        # a WEAK reference: the index lives in a cache keyed on this tensor, and holding the tensor here would keep both
        # alive for ever (a loader that builds new batch objects every step leaked one CSR per step)
        self._ei_ref = weakref.ref(ei)
        self._t = None
        self._ell = False              # False: not built yet; None: in-degree > 4 somewhere; else (ell_src, ell_eid)
        self._ell_t = False            # the same by source (out-degree), for the pipelined backward B2
        self._err = torch.zeros(1, **i32)
        ws = torch.empty(lib.glam_csr_workspace_bytes(self.N, self.E), dtype=torch.uint8, device=dev)
        lib.glam_csr_build(ptr(ei), self.N, self.E, 0, ptr(self.rowptr), ptr(self.src), ptr(self.eid), ptr(self._err), ptr(ws), ws.numel(), stream())
        # tensors built by glam_amd.data's collation carry a trust mark — the tensor's version counter at marking time: ids valid by
        # construction (checked once on the host when the dataset was packed) and not written since: no read-back, so a loop over
        # fresh batches has no host sync per step
        poll_checks()
        if validate and getattr(edge_index, "_glam_trusted", None) != edge_index._version:   # same failure class as torch's index_select on CPU
            _check_flag(self._err, f"edge_index holds node ids outside [0, {self.N})")

    @classmethod
    def from_parts(cls, edge_index, num_nodes, rowptr, src, eid, by_source, ell, ell_t):
        """The index of ``edge_index`` from tensors that ALREADY hold it (``glam_amd.data.DeviceDataset.collate`` writes them in the
        launch that writes ``edge_index``): nothing is launched, nothing is read back.  ``by_source = (colptr, dst, eid_t)``; ``ell`` /
        ``ell_t``: the ``[N, 4]`` pair, or ``None`` for an edge list without that form — both arrive resolved, never ``False``."""
        gi = cls.__new__(cls)
        gi.N, gi.E, gi.device = int(num_nodes), int(edge_index.size(1)), edge_index.device
        gi.rowptr, gi.src, gi.eid = rowptr, src, eid
        gi._ei_ref = weakref.ref(edge_index)
        gi._t = tuple(by_source)
        gi._ell = None if ell is None else tuple(ell)
        gi._ell_t = None if ell_t is None else tuple(ell_t)
        gi._err = None             # (the flag of the builds: there are none left to run)
        return gi

    # the pipelined forward pays off once xw + aggr (2 * N * H * Cp * 4 bytes) no longer fit the 256 MiB LLC (measured crossover:
    # B = 8 192 -> 0.59 general vs 0.55 pipelined; B = 16 384 -> 0.44-0.48 vs 0.56-0.64 of the HBM peak); ELL_MIN_NODES overrides
    ELL_MIN_NODES = -1          # (>= 0: a node count from which the ELL form is wanted regardless of the LLC)
    LLC_BYTES = 256 << 20

    @classmethod
    def wants_ell(cls, N, H, Cp):
        return N >= cls.ELL_MIN_NODES if cls.ELL_MIN_NODES >= 0 else 2 * N * H * Cp * 4 > cls.LLC_BYTES

    def ell(self):
        """``(ell_src, ell_eid)`` int32 ``[N, 4]`` index records of the software-pipelined forward aggregate (``glam_ell_build``),
        or ``None`` when some node has more than 4 incoming edges (one host sync, once per edge list — molecular graphs never
        do; protein contact maps always do and keep the general kernel).  While a stream capture is running the answer must
        already be known (a read-back would invalidate the capture): unknown then means ``None``, the general kernels."""
        if self._ell is False and torch.cuda.is_current_stream_capturing():
            return None
        if self._ell is False:
            self._ell = None
            if self.N > 0:
                lib = _lib.api()
                i32 = dict(dtype=torch.int32, device=self.device)
                es, ee, ovf = torch.empty(self.N, 4, **i32), torch.empty(self.N, 4, **i32), torch.zeros(1, **i32)
                lib.glam_ell_build(ptr(self.rowptr), ptr(self.src), ptr(self.eid), self.N, ptr(es), ptr(ee), ptr(ovf), stream())
                if int(ovf.item()) == 0:
                    self._ell = (es, ee)
        return self._ell

    def ell_t(self):
        """``(ell_dst, ell_eid_t)`` int32 ``[N, 4]``: the ELL records BY SOURCE of the software-pipelined backward B2 (``glam_ell_build`` on
        the CSR transpose), or ``None`` when some node has more than 4 outgoing edges (one host sync, once per edge list; inside a
        stream capture an answer not known yet is ``None``)."""
        if self._ell_t is False and torch.cuda.is_current_stream_capturing():
            return None
        if self._ell_t is False:
            self._ell_t = None
            if self.N > 0:
                lib = _lib.api()
                colptr, dst, eid_t = self.transpose()
                i32 = dict(dtype=torch.int32, device=self.device)
                es, ee, ovf = torch.empty(self.N, 4, **i32), torch.empty(self.N, 4, **i32), torch.zeros(1, **i32)
                lib.glam_ell_build(ptr(colptr), ptr(dst), ptr(eid_t), self.N, ptr(es), ptr(ee), ptr(ovf), stream())
                if int(ovf.item()) == 0:
                    self._ell_t = (es, ee)
        return self._ell_t

    def transpose(self):
        """CSR by source (built on first backward)."""
        if self._t is None:
            lib = _lib.api()
            i32 = dict(dtype=torch.int32, device=self.device)
            colptr, dst, eid_t = torch.empty(self.N + 1, **i32), torch.empty(self.E, **i32), torch.empty(self.E, **i32)
            ws = torch.empty(lib.glam_csr_workspace_bytes(self.N, self.E), dtype=torch.uint8, device=self.device)
            ei = self._ei_ref()
            if ei is None:     # the caller dropped edge_index before the first backward: the by-target CSR holds the same edges
                # Only the first rowptr[N] entries of src / eid were written: edges with bad ids were dropped (VALIDATE = "deferred" /
                # "off" lets such an index live).  Those entries go to a spare column and their edges come back as -1, which the build
                # below drops again — no read of an unwritten entry, no host sync, and the same tables as from the tensor itself.
                pos = torch.arange(self.E, device=self.device)
                live = pos < self.rowptr[-1]
                dst64 = torch.searchsorted(self.rowptr[1:].long(), pos, right=True)      # the segment that position pos lies in
                slot = torch.where(live, self.eid.long(), self.E)
                ei = torch.full((2, self.E + 1), -1, dtype=torch.int64, device=self.device)
                ei[0, slot] = torch.where(live, self.src.long(), -1)
                ei[1, slot] = torch.where(live, dst64, -1)
                ei = ei[:, :self.E].contiguous()
            lib.glam_csr_build(ptr(ei), self.N, self.E, 1, ptr(colptr), ptr(dst), ptr(eid_t), ptr(self._err), ptr(ws), ws.numel(), stream())
            self._t = (colptr, dst, eid_t)
        return self._t


# Whole-layer route for molecular graphs (ELL form, one-hot bond features of width 4): "auto" = the warp-specialised kernels
# (csrc/triplet_ws.hip, csrc/triplet_ws_b1.hip) wherever they exist, at every batch size; "0" = the general kernels (A/B knob of the
# tests: the two routes are pinned to each other).
WS_ROUTE = os.environ.get("GLAM_WS_ROUTE", "auto")


# --------------------------------------------------------------------------------------
# per-forward reuse of staged weights
# --------------------------------------------------------------------------------------
class _WeightScope:
    """Weight re-layouts (GEMM images, the TripletMessage staging buffer) made during ONE model forward, and the
    transposed images made by its backward.  A MessageBlock is applied ``message_steps`` times per forward with the same
    parameters (src_1gp/model.py:53-54), so each re-layout is built once per pass instead of once per application.  The
    scope only lives for one forward (and is kept alive by the autograd nodes for the matching backward): parameters cannot
    change inside it, so nothing can go stale.

    Three operations on the two tables (``table``: "fwd" / "bwd"; a value sits next to its ``owner``, so an ``id(owner)`` in the key stays
    unique) are the whole interface: ``lookup``, ``store``, ``build`` (``scope_build``: the scope may be None).  What is filed under which
    key is written down ONCE: a ``k_ts_gemm`` weight image by the constructor of its ``ImageSpec`` (``lin_image`` ...), which serves the
    op's lazy build (``scoped_image``) and ``prestage`` alike; any other entry that several sites touch by its key constructor
    (``triplet_key`` ...).  A new kind of entry adds a constructor, not a string at each site."""

    def __init__(self):
        self.fwd, self.bwd = {}, {}

    def lookup(self, table, key, owner):      # None: nothing there, or another object under the same key (a reused ``id()``)
        hit = (self.fwd if table == "fwd" else self.bwd).get(key)
        return hit[1] if hit is not None and hit[0] is owner else None

    def store(self, table, key, owner, value):
        (self.fwd if table == "fwd" else self.bwd)[key] = (owner, value)

    def build(self, table, key, owner, build_fn):      # ``build_fn()`` once per (table, key, owner)
        val = self.lookup(table, key, owner)
        if val is None:
            val = build_fn()
            self.store(table, key, owner, val)
        return val


_SCOPE = None


@contextlib.contextmanager
def weight_scope():
    """``with ops.weight_scope():`` around a model forward (``glam_amd.model.Architecture`` does it)."""
    global _SCOPE
    prev, _SCOPE = _SCOPE, _WeightScope()
    scope = _SCOPE
    try:
        yield
    finally:
        _SCOPE = prev
        # The forward table is only read while the forward runs.  Some of its entries carry autograd history that leads back
        # to nodes holding this scope (for their backward images): dropping the table here leaves no reference cycle, so the
        # pass's activations are released when its backward finishes, not whenever Python's cycle collector next runs (a
        # collection in the middle of a later hipGraph capture brings the capture down).
        scope.fwd.clear()


def scope_build(scope, table, key, owner, build_fn):      # ``scope.build`` for a scope that may be None: ``build_fn()`` every time
    return build_fn() if scope is None else scope.build(table, key, owner, build_fn)


def scoped_weights(key, owner, build):
    """Derived weights (pure functions of parameters: pads, stacks, small matmuls) built once per model forward when a
    ``weight_scope`` is active; their autograd subgraph is then also shared by the applications of the block."""
    return scope_build(_SCOPE, "fwd", key, owner, build)


# ---- k_ts_gemm weight images: ONE description per image, for the lazy build of its op (scoped_image) and for prestage ------------
# ``glam_ts_gemm_make_image(W, ldw, transW, K, M, img)`` into an image of ``glam_ts_gemm_image_bytes(Kimg, M)`` bytes, filed in the scope's
# ``table`` under ``key`` / ``owner``.  ``Kimg > K``: a zero-padded input's linear (15 -> 16 rows), filled from the unpadded weight.
ImageSpec = collections.namedtuple("ImageSpec", "table key owner W ldw transW K M Kimg")


class _ImageKind(collections.namedtuple("_ImageKind", "table name transposed")):
    """One kind of weight image: its scope table, the name in its key and whether it holds ``W`` as stored (``[K, M]``) or the transpose
    of the stored ``[M, K]`` matrix.  Calling it gives the ``ImageSpec`` of one matrix ``W`` (default: the owner itself)."""

    def entry(self, owner):      # (table, key, owner): where the image of ``owner`` is filed
        return self.table, (self.name, id(owner)), owner

    def __call__(self, owner, Kimg=None, W=None):
        W = owner if W is None else W
        K, M = W.shape[::-1] if self.transposed else W.shape
        return ImageSpec(*self.entry(owner), W, W.stride(0), int(self.transposed), K, M, K if Kimg is None else Kimg)


# an nn.Linear weight [M, Kw] for an input of Kimg (default: Kw) columns, and its input-gradient product dy[N, M] @ w
lin_image, lin_dx_image = _ImageKind("fwd", "lin", True), _ImageKind("bwd", "lin", False)
# the [K, M]-stored operand of _MatmulTall, and dy[N, M] @ w^T
tall_image, tall_dx_image = _ImageKind("fwd", "tall-fwd", False), _ImageKind("bwd", "tall-dx", True)
# _TripletLayerWide (owner wn; W: the views Wcat[Cp, HC + 8] / Ws_p[HC, Cp] of its plain staging): x @ Wcat, aggr @ Ws_p, d_out @ Ws_p^T, [d_xw | d_a] @ Wcat^T
wide_node_image, wide_upd_image = _ImageKind("fwd", "wide-img-node", False), _ImageKind("fwd", "wide-img-upd", False)
wide_dagg_image, wide_dx_image = _ImageKind("bwd", "wide-img-dagg", True), _ImageKind("bwd", "wide-img-dx", True)


def scoped_image(scope, kind, owner, Kimg=None, W=None):
    """The image ``kind(owner, Kimg, W)``, built on first use and filed in ``scope`` (None: built every time); a hit builds no spec."""
    img = None if scope is None else scope.lookup(kind.table, (kind.name, id(owner)), owner)
    if img is None:
        lib, spec = _lib.api(), kind(owner, Kimg, W() if callable(W) else W)      # (a callable W: built on a miss only)
        img = torch.empty(lib.glam_ts_gemm_image_bytes(spec.Kimg, spec.M) // 4, dtype=torch.float32, device=spec.W.device)
        lib.glam_ts_gemm_make_image(ptr(spec.W), spec.ldw, spec.transW, spec.K, spec.M, ptr(img), stream())
        if scope is not None:
            scope.store(*kind.entry(owner), img)
    return img


# ---- keys of the other entries that several sites touch (the owner is the first tensor): the staged images of a TripletMessage (plain:
# the wide layer's staging), the flag that the pass applied it on the ELL route, the pre-split images of a GRU's gate matrices (a
# gru_pre_buffer: [2, bytes], forward | backward), the gate-padded images of the fp32 fused GRU step, the padded GRU parameters of an odd width
def triplet_key(wn, we, att, wsc, bias, plain=False): return ("triplet-plain" if plain else "triplet", id(wn), id(we), id(att), id(wsc), id(bias))
def triplet_ell_key(wn): return ("triplet-ell", id(wn))
def gru_pre_key(w_ih, w_hh): return ("gru-pre", id(w_ih), id(w_hh))
def gru_pre_buffer(w_ih): return torch.empty(2, _lib.api().glam_gru_ws_pre_bytes(), dtype=torch.uint8, device=w_ih.device)
def gru_fused_key(w_ih, w_hh): return ("gru-fused", id(w_ih), id(w_hh))
def gru_pad_key(w_ih, w_hh, b_ih, b_hh): return ("gru-pad", id(w_ih), id(w_hh), id(b_ih), id(b_hh))


def prestage(triplet=None, images=(), gru_pre=()):
    """The derived weights of a model pass in ONE launch (``glam_prestage``) instead of one per module at its first use: the staged
    images of a TripletMessage (``triplet = (wn, we, att, wsc, bias, H, Dp)``) and up to six ``k_ts_gemm`` weight images
    (``images``: ``ImageSpec``s, or plain tuples of their fields, from the constructors that the ops build their images with lazily).
    The entries are put into the active ``weight_scope`` exactly as the lazy builders would put them, so an op whose route differs
    from the caller's guess just builds its own as before.  Returns the
    number of entries built (0: no scope, switched off, or everything already there).  ``gru_pre``: ``(w_ih, w_hh, C)`` per GRU whose
    warp-specialised step wants its pre-split images (``glam_gru_ws_make_pre``; four of the six jobs of a launch)."""
    scope = _SCOPE
    if scope is None or not PRESTAGE:
        return 0
    lib = _lib.api()
    args_t = [None] * 5 + [0] * 5 + [None]
    built = 0
    on_device = lambda *ts: all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts)
    if triplet is not None and not CACHED_STAGING:
        wn, we, att, wsc, bias, H, Dp = triplet
        key = triplet_key(wn, we, att, wsc, bias)
        if on_device(wn, we, att, wsc, bias) and scope.lookup("fwd", key, wn) is None:
            C, De = wn.size(0), we.size(0)
            Cp = (C + 3) // 4 * 4
            buf = torch.empty(lib.glam_triplet_staged_floats(H, Cp, Dp), dtype=torch.float32, device=wn.device)
            args_t = [ptr(wn), ptr(we), ptr(att), ptr(wsc), ptr(bias), C, H, De, Cp, Dp, ptr(buf)]
            scope.store("fwd", key, wn, buf)
            built += 1
    jobs = []
    for table, key, owner, W, ldw, transW, K, M, Kimg in images:
        if scope.lookup(table, key, owner) is not None or not on_device(W) or len(jobs) == 6:
            continue
        img = torch.empty(lib.glam_ts_gemm_image_bytes(Kimg, M) // 4, dtype=torch.float32, device=W.device)
        jobs.append((W, (ldw, transW, K, M), img))
        scope.store(table, key, owner, img)
        built += 1
    for w_ih, w_hh, C in gru_pre:
        key = gru_pre_key(w_ih, w_hh)
        if scope.lookup("fwd", key, w_ih) is not None or not on_device(w_ih, w_hh) or len(jobs) + 4 > 6:
            continue
        buf = gru_pre_buffer(w_ih)
        jobs += [(w_ih, (C, 2, C, 0), buf[0]), (w_hh, (C, 2, C, 1), buf[0]), (w_ih, (C, 3, C, 0), buf[1]), (w_hh, (C, 3, C, 1), buf[1])]
        scope.store("fwd", key, w_ih, buf)
        built += 1
    if built == 0:
        return 0
    n = len(jobs)
    wp = (ctypes.c_void_p * max(n, 1))(*[ptr(j[0]) for j in jobs])
    ip = (ctypes.c_void_p * max(n, 1))(*[ptr(j[2]) for j in jobs])
    dims = (ctypes.c_int32 * (4 * max(n, 1)))(*[v for j in jobs for v in j[1]])
    lib.glam_prestage(*args_t, n, wp, dims, ip, stream())
    return built


class _PadGroup(torch.autograd.Function):
    """Zero-padded copies of several parameters of one module in ONE launch (``glam_pad_group``); the backward slices all their
    gradients in one launch too.  ``specs[t] = (d0, d1, d2, p1, p2)``: tensor t viewed as ``[d0, d1, d2]`` becomes ``[d0, p1, p2]``."""

    @staticmethod
    def forward(ctx, specs, *params):
        require_device(*params)
        params = [f32c(p, "parameter") for p in params]
        dev = params[0].device
        outs = [torch.empty(d0 * p1 * p2, dtype=torch.float32, device=dev) for d0, _, _, p1, p2 in specs]
        _pad_group_launch(params, outs, specs, 0)
        ctx.specs, ctx.shapes, ctx.dev = specs, [p.shape for p in params], dev
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *d_outs):
        specs = ctx.specs
        grads = [torch.empty(d0 * d1 * d2, dtype=torch.float32, device=ctx.dev) for d0, d1, d2, _, _ in specs]
        _pad_group_launch([None if g is None else f32c(g, "d_padded") for g in d_outs], grads, specs, 1)
        return (None,) + tuple(g.view(sh) for g, sh in zip(grads, ctx.shapes))


def _pad_group_launch(src, dst, specs, backward):
    n = len(specs)
    vp = ctypes.c_void_p * n
    dims = (ctypes.c_int32 * (5 * n))(*[v for sp in specs for v in sp])
    _lib.api().glam_pad_group(n, vp(*[None if t is None else t.data_ptr() for t in src]), vp(*[t.data_ptr() for t in dst]), dims, backward, stream())


class _CatCols(torch.autograd.Function):
    """``torch.cat(tensors, dim=1)`` of up to eight [R, C_t] matrices whose backward hands every input a CONTIGUOUS gradient from ONE
    launch (``glam_pad_group`` in its slicing direction, the column block of tensor t read as a "padded" [1, R, total] tensor that
    starts at its first column) — autograd's own CatBackward returns strided views, and every consumer that needs rows of C_t floats
    (the readout linears, the pair pools of the two-tower models: src_2gi_dti_scr/model.py:60-75) then copies its piece with a launch
    of its own."""

    @staticmethod
    def forward(ctx, *ts):
        ctx.widths = [t.size(1) for t in ts]
        ctx.set_materialize_grads(False)
        return torch.cat(ts, dim=1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * len(ctx.widths)
        g = f32c(g, "d_cat")
        R, total = g.shape
        outs = [torch.empty(R, c, dtype=torch.float32, device=g.device) if need else None for c, need in zip(ctx.widths, ctx.needs_input_grad)]
        src, dst, specs, off = [], [], [], 0
        for c, o in zip(ctx.widths, outs):
            if o is not None and R > 0 and c > 0:
                src.append(g.view(-1)[off:]); dst.append(o); specs.append((1, R, c, R, total))
            off += c
        if specs:
            _pad_group_launch(src, dst, specs, 1)
        return tuple(outs)


def cat_cols(tensors):
    """``torch.cat(tensors, dim=-1)``; for 2-D fp32 device matrices (at most eight) with contiguous gradients from one launch (_CatCols)."""
    ts = list(tensors)
    if (1 < len(ts) <= 8 and all(t.dim() == 2 and t.is_cuda and t.dtype == torch.float32 and t.size(0) == ts[0].size(0) for t in ts)
            and torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
        return _CatCols.apply(*ts)
    return torch.cat(ts, dim=-1)


def pad_group(items):
    """``items = [(tensor, (d0, d1, d2), (p1, p2), out_shape), ...]`` (at most 8, one module's parameters): the zero-padded
    re-layouts of all of them from one launch, gradients back through one launch."""
    specs = tuple((d0, d1, d2, p1, p2) for _, (d0, d1, d2), (p1, p2), _ in items)
    outs = _PadGroup.apply(specs, *[t for t, _, _, _ in items])
    return tuple(o.view(sh) for o, (_, _, _, sh) in zip(outs, items))


# ---- zero-padded column layout of odd-width features (hid_dim 15 / 30 / 45 / 90: C % 4 != 0) ----------------------
# The kernels work on rows of Cp = ceil4(C) floats.  An op that produced a padded [N, Cp] tensor whose pad columns are
# zero hands the caller the [N, C] VIEW of it (slice_cols) and remembers the padded tensor; when that view comes back as
# the input of the next op (conv -> GRU -> next message step), pad_cols returns the padded tensor itself instead of
# copying: the per-step pad / slice glue of the odd widths disappears without changing any module interface.
_PADDED = TensorMemo("ptr")      # the padded tensors themselves (TensorMemo.referent): no value goes with them


def slice_cols(x_p, C):
    """``x_p[:, :C]`` of a padded tensor whose columns ``C..`` are zero (the caller guarantees it)."""
    if x_p.size(1) == C:
        return x_p
    _PADDED.put(x_p, True)
    v = x_p[:, :C]
    v._glam_padded = x_p      # the view keeps its padded tensor alive (a view of a VIEW — the skip-connection alias of _TripletLayer —
    return v                  # only references the root storage owner: the registered object would die with the caller's local)


def padded_base(x):
    """The registered zero-padded tensor that ``x[N, C]`` is the untouched view of, or None."""
    base = _PADDED.referent(x) if x.dim() == 2 else None
    if base is not None and base.size(0) == x.size(0) and base.size(1) > x.size(1) and \
            x.stride() == (base.size(1), 1) and base.data_ptr() == x.data_ptr() and base.dtype == x.dtype:
        return base
    return None


def pad_cols(x, Cp):
    """``x[N, C]`` zero-padded to ``Cp`` columns: the registered padded tensor when ``x`` is its untouched view, else one
    ``F.pad`` per tensor and model pass."""
    if x.size(1) == Cp:
        return x
    base = padded_base(x)
    if base is not None and base.size(1) == Cp:
        return base
    C = x.size(1)
    if not x.requires_grad and x.grad_fn is None:
        # a DATA tensor (e.g. the atom features x[N, 15] of a cached loader batch): padded once per tensor, not once per pass
        padded = _PAD_DATA.get(x)
        if padded is None or padded.size(1) != Cp:
            padded = torch.nn.functional.pad(x, (0, Cp - C))
            _PAD_DATA.put(x, padded)
        return padded
    return scoped_weights(("pad-cols", id(x), Cp), x, lambda: torch.nn.functional.pad(x, (0, Cp - C)))


_PAD_DATA = TensorMemo("id")      # data tensor -> its zero-padded copy


_GI_CACHE = TensorMemo("id")      # edge_index -> (num_nodes, GraphIndex)


def graph_index(edge_index, num_nodes):
    """Cached ``GraphIndex`` for this very tensor object (dropped when the tensor dies or is
    modified in place)."""
    hit = _GI_CACHE.get(edge_index)
    if hit is not None and hit[0] == int(num_nodes):
        return hit[1]
    gi = GraphIndex(edge_index, num_nodes)
    _GI_CACHE.put(edge_index, (int(num_nodes), gi))
    return gi


class SegmentPtr:
    """``ptr[B+1]`` (int32) of a sorted ``batch`` vector; ``num_graphs`` optional — when absent it
    is read back from ``batch[-1]`` exactly like PyG's ``int(batch.max()) + 1`` (one host sync)."""

    def __init__(self, batch, num_graphs=None, validate=True):
        require_device(batch)
        if batch.dtype != torch.int64 or batch.dim() != 1:
            raise GlamHipError("batch must be an int64 vector")
        self.N = int(batch.numel())
        if num_graphs is None:
            num_graphs = int(batch[-1].item()) + 1 if self.N > 0 else 0
        self.B = int(num_graphs)
        if self.B < 0 or self.B >= 2 ** 31 - 1:      # an unchecked batch[-1] (negative / huge id) must not size the ptr buffer
            raise IndexError(f"batch must be non-decreasing with ids in [0, num_graphs) (num_graphs = {self.B})")
        self.ptr = torch.empty(self.B + 1, dtype=torch.int32, device=batch.device)
        err = torch.zeros(1, dtype=torch.int32, device=batch.device)
        _lib.api().glam_batch_ptr(ptr(batch.contiguous()), self.N, self.B, ptr(self.ptr), ptr(err), stream())
        poll_checks()
        if validate and getattr(batch, "_glam_trusted", None) != batch._version:
            _check_flag(err, "batch must be non-decreasing with ids in [0, num_graphs)")

    @classmethod
    def from_parts(cls, ptr32, num_nodes, num_graphs):
        """The segment pointer from an int32 ``ptr[B+1]`` that already exists (``DeviceDataset.collate``): no launch, no read-back."""
        sp = cls.__new__(cls)
        sp.N, sp.B, sp.ptr = int(num_nodes), int(num_graphs), ptr32
        return sp


_SP_CACHE = TensorMemo("id")      # batch vector -> SegmentPtr


def segment_ptr(batch, num_graphs=None):
    sp = _SP_CACHE.get(batch)
    if sp is None or not (num_graphs is None or sp.B == int(num_graphs)):
        sp = SegmentPtr(batch, num_graphs)
        _SP_CACHE.put(batch, sp)
    return sp


# --------------------------------------------------------------------------------------
# fused gather / attention softmax / scatter-add  (TripletMessage, TripletMessageLight)
# --------------------------------------------------------------------------------------
class _TripletAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xw, a_ij, edge_attr, w_edge, M, gi, H, Cp, De, emul, slope):
        require_device(xw, a_ij, edge_attr, w_edge, M)
        xw, a_ij, edge_attr, M = f32c(xw, "xw"), f32c(a_ij, "a_ij"), f32c(edge_attr, "edge_attr"), f32c(M, "M")
        w_edge = f32c(w_edge, "w_edge") if emul else None
        N, E = gi.N, gi.E
        if xw.shape != (N, H * Cp) or a_ij.shape != (N, 8) or edge_attr.shape != (E, De) or M.shape != (De, 4):
            raise GlamHipError(f"triplet_aggregate: shape mismatch xw={tuple(xw.shape)} a_ij={tuple(a_ij.shape)} "
                               f"edge_attr={tuple(edge_attr.shape)} M={tuple(M.shape)} for N={N} E={E} H={H} Cp={Cp} De={De}")
        aggr = torch.empty(N, H * Cp, dtype=torch.float32, device=xw.device)
        stats = torch.empty(N, 8, dtype=torch.float32, device=xw.device)
        lib = _lib.api()
        # Batches whose working set leaves the 256 MiB LLC: the software-pipelined kernel (bit-identical; 0.56 vs 0.44 of the HBM
        # peak at B = 16 384).  Below that the general kernel's three waves per SIMD win (9.4 vs 10.4 us at B = 1 024).
        ell = gi.ell() if (emul and GraphIndex.wants_ell(N, H, Cp) and lib.glam_triplet_fwd_ell_supported(H, Cp, De)) else None
        if ell is not None:
            lib.glam_triplet_fwd_ell(ptr(xw), ptr(a_ij), ptr(edge_attr), ptr(w_edge), ptr(M), ptr(ell[0]), ptr(ell[1]), N, E, H, Cp, De,
                                     float(slope), int(rows_are_one_hot(edge_attr)), ptr(aggr), ptr(stats), 0, stream())
        else:
            lib.glam_triplet_fwd(ptr(xw), ptr(a_ij), ptr(edge_attr), ptr(w_edge), ptr(M), ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid), N, E, H, Cp, De,
                                 int(emul), float(slope), ptr(aggr), ptr(stats), stream())
        ctx.save_for_backward(xw, a_ij, edge_attr, w_edge, M, aggr, stats)
        ctx.gi, ctx.dims = gi, (H, Cp, De, int(emul), float(slope))
        return aggr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_aggr):
        xw, a_ij, edge_attr, w_edge, M, aggr, stats = ctx.saved_tensors
        gi = ctx.gi
        H, Cp, De, emul, slope = ctx.dims
        N, E = gi.N, gi.E
        lib = _lib.api()
        d_aggr = f32c(d_aggr, "d_aggr")
        colptr, dst, eid_t = gi.transpose()
        dev = xw.device
        d_xw = torch.empty_like(xw)
        d_a_ij = torch.empty_like(a_ij)
        d_w_edge = torch.empty_like(w_edge) if emul else None
        d_M = torch.empty_like(M)
        d_ea = torch.zeros_like(edge_attr) if ctx.needs_input_grad[2] else None
        ws = torch.empty(lib.glam_triplet_bwd_workspace_bytes(N, E, H, Cp, De), dtype=torch.uint8, device=dev)
        lib.glam_triplet_bwd(ptr(xw), ptr(a_ij), ptr(edge_attr), ptr(w_edge), ptr(M), ptr(aggr), ptr(stats), ptr(d_aggr), ptr(gi.rowptr), ptr(gi.src),
                             ptr(gi.eid), ptr(colptr), ptr(dst), ptr(eid_t), N, E, H, Cp, De, emul, slope, ptr(d_xw), ptr(d_a_ij), ptr(d_w_edge),
                             ptr(d_M), ptr(d_ea), ptr(ws), ws.numel(), stream())
        return d_xw, d_a_ij, d_ea, d_w_edge, d_M, None, None, None, None, None, None


def triplet_aggregate(xw, a_ij, edge_attr, w_edge, M, gi, heads, Cp, slope=0.2):
    """``aggr[N, H*Cp]`` of TripletMessage (see ``glam_triplet_fwd`` in include/glam_hip.h)."""
    return _TripletAggregate.apply(xw, a_ij, edge_attr, w_edge, M, gi, heads, Cp, edge_attr.size(1), True, slope)


def light_aggregate(xw, a_ij, edge_attr, M, gi, Cp, slope=0.2):
    """``aggr[N, Cp]`` of TripletMessageLight (single head, message ``alpha * x_j``)."""
    return _TripletAggregate.apply(xw, a_ij, edge_attr, None, M, gi, 1, Cp, edge_attr.size(1), False, slope)


def _triplet_shapes(wn, we, att, H):
    """The layout of a TripletMessage's flat parameter gradients: its five parameters in parameter order."""
    C = wn.size(0)
    return (wn.shape, we.shape, att.shape, (H * C, C), (C,))


def fused_layer_supported(C, heads, De):
    """Shapes covered by the dense MFMA kernels behind ``glam_triplet_layer_*`` (C <= 60 at 3 heads)."""
    Cp = (C + 3) // 4 * 4
    return heads * Cp + 8 <= 192 and Cp <= 64 and De <= 8 and 1 <= heads <= 4


# ---- gradient carry of a block's parameters ---------------------------------------------------------------------------
# A MessageBlock applies the SAME parameters message_steps times per forward (src_1gp/model.py:53-54), so autograd would sum
# message_steps gradients per parameter tensor: 17 small add kernels per training step of the default model.  Inside a
# weight_scope the parameters instead enter the graph once, through a `_ParamBundle` node whose output (an uninitialised
# flat tensor — only its GRADIENT matters) is threaded through the applications as an extra input / output: application k's
# backward receives the gradients accumulated by the later applications, adds its own flat gradient buffer (one add), and
# hands the sum on; the bundle's backward splits the total into per-parameter views.  Works for .backward() and
# autograd.grad alike; outside a scope (or without grad) the ops return per-parameter gradients as before.
GRAD_CARRY = True            # (module switches like this one are attributes, not environment variables: the tests flip them in place)


def _flat_views(flat, shapes):
    """Consecutive views of ``flat`` with the given shapes: the pieces of a flat gradient buffer, in memory order."""
    return [t.view(s) for t, s in zip(flat.split([math.prod(s) for s in shapes]), shapes)]


def _flat_grads(shapes, device):
    """An uninitialised flat fp32 gradient buffer laid out as ``shapes`` and its views (``_flat_views``)."""
    flat = torch.empty(sum(math.prod(s) for s in shapes), dtype=torch.float32, device=device)
    return flat, _flat_views(flat, shapes)


class _ParamBundle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, shapes, order, *params):
        ctx.shapes, ctx.order = shapes, order
        return torch.empty(sum(math.prod(s) for s in shapes), dtype=torch.float32, device=params[0].device)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_flat):
        views = _flat_views(d_flat, ctx.shapes)
        return (None, None) + tuple(views[i] for i in ctx.order)


class _Carry:
    """One application's end of the gradient carry of a block's parameters ``params`` under the scope key ``key``.  ``shapes``: the
    pieces of the flat gradient buffer in memory order; ``order[i]``: the piece that holds the gradient of ``params[i]`` (default:
    parameter order).  ``tensor`` is the carry to hand to the node, None when there is no scope, gradients are off or no parameter
    requires one; ``first`` marks the block's first application of the pass, whose backward runs LAST."""

    def __init__(self, key, params, shapes, order=None):
        self.key, self.owner, self.scope = key, params[0], _SCOPE
        prev = self.scope.lookup("fwd", key, self.owner) if self.scope is not None else None
        self.first = prev is None
        self.tensor = None
        if self.scope is not None and GRAD_CARRY and torch.is_grad_enabled() and any(p.requires_grad for p in params):
            order = tuple(range(len(params))) if order is None else order
            self.tensor = _ParamBundle.apply(shapes, order, *params) if self.first else prev

    def store(self, carry):
        """The node's carry output, for the block's next application."""
        if carry is not None:
            self.scope.store("fwd", self.key, self.owner, carry)


def _carried(flat, d_carry, summed=False):
    """What a node hands back through the carry: its flat parameter gradients plus those of the later applications (``d_carry``),
    unless the reduction of its weight-gradient product already added them (``summed``)."""
    return flat if (summed or d_carry is None) else flat.add_(d_carry)


# ---- parked weight-gradient operand sets ---------------------------------------------------------------------------------
# With GRU_WGRAD_BATCH the weight gradients of ALL applications of a block come from one product over their operands: every
# application but the first parks its operand set in the scope and hands the carry on untouched; the first one (its backward runs
# last: everything later in the forward depends on its outputs) multiplies the parked sets together, three per launch, chaining each
# launch's result into the next as its addend.  3 weight-gradient launches + 3 reductions -> 1 + 1 per training step at message_steps = 3.
_WGRAD_BATCH_MIN_ROWS = 512     # (a wave's row range must fit into one operand set: glam_wgrad_gemm_pair_split_seg)


def _parks(scope, N):
    """True when a carried node of ``N`` rows parks its weight-gradient operands (``_park``) instead of multiplying them itself."""
    return scope is not None and GRU_WGRAD_BATCH and N >= _WGRAD_BATCH_MIN_ROWS


def _park(scope, kind, owner, first, operands, compat=None):
    """Parks ``operands`` (unless None) with the sets of the block's other applications.  Returns None on every application but the
    first: the caller returns its pass-through gradients.  On the first one it returns all parked sets as the groups to launch: at
    most three sets each, of one ``compat`` key, in parking order.  The list is emptied before anything is launched: a set left
    behind by an interrupted backward would be counted again by a retried one (``retain_graph=True``)."""
    parked = scope.build("bwd", ("parked", kind, id(owner)), owner, list)
    if operands is not None:
        parked.append((compat, operands))
    if not first:
        return None
    sets = list(parked)
    parked.clear()
    groups = []
    while sets:
        grp = [s for s in sets if s[0] == sets[0][0]][:3]
        sets = [s for s in sets if all(s is not g for g in grp)]
        groups.append([s[1] for s in grp])
    return groups


# ---- staged parameter images across passes -------------------------------------------------------------------------------
# The weight re-layout of a TripletMessage (k_stage_params: four GEMM images, W_edge, M, bias) depends on the parameters only.  By
# default it is rebuilt in every pass (every model forward inside a weight_scope): always right, also when a captured optimizer
# launch rewrites the parameters between replays, which no host-side bookkeeping can see.  ``with ops.cached_staging():`` is the
# caller's statement that parameters are written only through torch (in-place ops bump the version counter; ``.data`` swaps change
# the address) and NOT by kernels replayed from a graph that also holds this forward: the images are then kept until a parameter's
# (address, version) changes — a forward-backward step whose parameters stand still (bench.py's configs[1] step: no optimizer in it)
# starts at the node GEMM.
# Writers the host cannot see through (address, version counter) — ``glam_amd.optim.Adam`` updates parameters through raw device
# pointers — announce themselves by bumping PARAM_EPOCH, which is part of every entry's stamp.
CACHED_STAGING = False
_STAGED: dict = {}
PARAM_EPOCH = 0


def parameters_written():
    """Tell the staging cache that parameters were (or will be, by a launch just enqueued) written outside torch's version counting."""
    global PARAM_EPOCH
    PARAM_EPOCH += 1


@contextlib.contextmanager
def cached_staging(on=True):
    global CACHED_STAGING
    prev, CACHED_STAGING = CACHED_STAGING, bool(on)
    try:
        yield
    finally:
        CACHED_STAGING = prev


def _staged_cached(kind, params, build):
    key = (kind,) + tuple(id(p) for p in params)
    stamp = (PARAM_EPOCH,) + tuple((p.data_ptr(), p._version) for p in params)
    hit = _STAGED.get(key)
    if hit is not None and hit[0] == stamp and all(r() is p for r, p in zip(hit[1], params)):
        return hit[2]
    val = build()
    if torch.cuda.is_current_stream_capturing():
        # built inside a capture: the buffer lives in the graph's pool and is only filled when the graph is replayed — an eager pass
        # before that would read uninitialised images, so it is never published to the cache
        return val
    try:
        refs = tuple(weakref.ref(p, lambda _r, k=key, c=_STAGED: c.pop(k, None)) for p in params)
    except TypeError:
        return val
    _STAGED[key] = (stamp, refs, val)
    return val


def _ws_route(lib, N, H, Cp, Dp, ea_p):
    """The warp-specialised kernels cover this layer call (shape table in the library + one-hot rows: one cached read-back per tensor)."""
    return WS_ROUTE != "0" and N > 0 and lib.glam_triplet_layer_ws_supported(H, Cp, Dp, 1) == 1 and rows_are_one_hot(ea_p)


class _TripletLayer(torch.autograd.Function):
    """Whole TripletMessage layer: parameter staging, node GEMM (+ separable attention columns), fused
    gather/softmax/scatter-add, update GEMM — and the hand-written backward of all of it."""

    @staticmethod
    def forward(ctx, x_p, ea_p, wn, we, att, wsc, bias, gi, H, slope, carry=None, with_identity=False, first_app=True, no_backward=False):
        """Returns ``out`` — or the tuple ``(out[, x_p itself][, carry])``.  ``with_identity``: the layer's input comes back as a second
        output, the skip connection of a MessageBlock (src_1gp/layer.py:253-265: ``x`` feeds the conv AND ``x + identity``): both gradient
        paths then arrive at THIS node and the d_x product's epilogue sums them (glam_triplet_layer_bwd_params_ell_add) instead of
        autograd launching an add per block application."""
        require_device(x_p, ea_p, wn, we, att, wsc, bias)
        x_in = x_p
        x_p, ea_p = f32c(x_p, "x"), f32c(ea_p, "edge_attr")
        wn, we, att, wsc, bias = (f32c(t, n) for t, n in ((wn, "weight_node"), (we, "weight_edge"),
                                                           (att, "weight_triplet_att"), (wsc, "weight_scale"), (bias, "bias")))
        C, De = wn.size(0), we.size(0)
        N, Cp = x_p.shape
        Dp = ea_p.size(1)
        if gi.N != N or ea_p.size(0) != gi.E or wn.shape != (C, H * C) or wsc.shape != (H * C, C) or Cp != (C + 3) // 4 * 4:
            raise GlamHipError("triplet_layer: shape mismatch")
        lib, dev = _lib.api(), x_p.device
        HC = H * Cp
        f = dict(dtype=torch.float32, device=dev)
        ctx.carried = carry is not None
        ctx.aliased = bool(with_identity)
        ctx.first_app = bool(first_app)
        ctx.scope = _SCOPE
        ctx.set_materialize_grads(False)     # the carry of the block's LAST application has no gradient yet: None, not a zero fill
        def build():
            buf = torch.empty(lib.glam_triplet_staged_floats(H, Cp, Dp), **f)
            lib.glam_triplet_stage_params(ptr(wn), ptr(we), ptr(att), ptr(wsc), ptr(bias), C, H, De, Cp, Dp, ptr(buf), stream())
            return buf

        # the same conv is applied message_steps times per model forward: one staging per pass (see _WeightScope); with
        # ops.cached_staging() the staged images additionally survive from pass to pass until a parameter is written
        staged = _staged_cached(("triplet", H, Cp, Dp), (wn, we, att, wsc, bias), build) if CACHED_STAGING else \
            scoped_weights(triplet_key(wn, we, att, wsc, bias), wn, build)
        out = torch.empty(N, Cp, **f)
        # molecular graphs with one-hot bond features take the warp-specialised kernels at every size (13.6 vs 16.8 us at B = 1 024,
        # 136 vs 256 us at B = 16 384 against the general fused kernel); everything else the general kernels
        ell = gi.ell() if _ws_route(lib, N, H, Cp, Dp, ea_p) else None
        # the node product may exist already: the previous application's GRU step wrote it with these very rows (ops.NODE_IN_GRU)
        given = take_node_product(x_p, staged) if ell is not None else None
        xw, a_ij = given if given is not None else (torch.empty(N, HC, **f), torch.empty(N, 8, **f))
        if ell is not None and _SCOPE is not None:
            _SCOPE.store("fwd", triplet_ell_key(wn), wn, True)
        # no backward will come (torch.no_grad(): the evaluation passes of src_1gp/trainer.py:306-327): the inference forward, which keeps
        # neither `aggr` nor `stats` (two thirds of what the launch writes)
        # (`no_backward` comes from the caller: inside forward() autograd is off and needs_input_grad ignores torch.no_grad())
        infer = INFER_FWD and no_backward and (ell is not None or bool(lib.glam_triplet_layer_infer_supported(H, Cp, Dp)))
        aggr, stats = (None, None) if infer else (torch.empty(N, HC, **f), torch.empty(N, 8, **f))
        if ell is not None:
            lib.glam_triplet_layer_fwd_ell(None if given is not None else ptr(x_p), ptr(ea_p), ptr(staged), ptr(ell[0]), ptr(ell[1]), 1, N,
                                           gi.E, H, Cp, Dp, float(slope), ptr(xw), ptr(a_ij), ptr(aggr), ptr(stats), ptr(out), stream())
        else:
            lib.glam_triplet_layer_fwd(ptr(x_p), ptr(ea_p), ptr(staged), ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid), N, gi.E, H, Cp, Dp, float(slope),
                                       ptr(xw), ptr(a_ij), ptr(aggr), ptr(stats), ptr(out), stream())
        if not infer:
            ctx.save_for_backward(x_p, ea_p, wn, we, att, staged, xw, a_ij, aggr, stats)
        ctx.gi, ctx.dims = gi, (C, H, De, Cp, Dp, float(slope))
        res = (out,) + ((x_in.view_as(x_in),) if ctx.aliased else ()) + ((carry.view(-1),) if ctx.carried else ())
        return res if len(res) > 1 else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, *more):
        d_alias = more[0] if ctx.aliased else None
        d_carry = more[-1] if ctx.carried else None
        x_p, ea_p, wn, we, att, staged, xw, a_ij, aggr, stats = ctx.saved_tensors
        C, H, De, Cp, Dp, slope = ctx.dims
        gi, scope = ctx.gi, ctx.scope
        N, E = gi.N, gi.E
        lib, dev = _lib.api(), x_p.device
        groups = None
        if d_out is None:
            # the layer's output was not used: only the skip connection / the carry pass through — on the first application together
            # with the parameter gradients of the sets that the later applications parked (below: without a set of its own)
            groups = _park(scope, "triplet", wn, True, None) if (scope is not None and ctx.first_app) else None
            if not groups:
                return (d_alias,) + (None,) * 9 + (d_carry, None, None, None)
            d_x, d_ea = d_alias, None
        else:
            d_out = f32c(d_out, "d_out")
            colptr, dst, eid_t = gi.transpose()
            d_x = torch.empty_like(x_p)
            d_ea = torch.zeros_like(ea_p) if ctx.needs_input_grad[1] else None
            ws = torch.empty(lib.glam_triplet_layer_bwd_workspace_bytes(N, E, H, Cp, Dp), dtype=torch.uint8, device=dev)
            # molecular graphs with one-hot bond features: B1 and B2 + d_x warp-specialised over the ELL records of both directions
            ell_t = gi.ell_t() if (d_ea is None and _ws_route(lib, N, H, Cp, Dp, ea_p)) else None
            ell_f = gi.ell() if ell_t is not None else None          # (by target: what the forward used)
            if ctx.carried and d_ea is None and _parks(scope, N):
                # The parameter gradients of ALL applications of the layer from one launch pair (see _park): every application runs the
                # DATA half of its backward (d_x) and parks its operands — its workspace holds d_xw, d_a and the block partials of
                # d_W_edge / d_M —; the first application runs both weight-gradient products over the parked sets and k_param_grads ONCE
                # (glam_triplet_layer_param_grads_sets).  3 x (k_wgrad + k_param_grads) -> 1 + 1 per training step at message_steps = 3.
                in_kernel = d_alias is not None and ell_t is not None and _lib.route_enabled("x3")   # (warp-specialised route only)
                addend = f32c(d_alias, "d_identity") if in_kernel else None
                info = (ctypes.c_int64 * 4)()
                lib.glam_triplet_layer_bwd_data_ell(ptr(x_p), ptr(ea_p), ptr(staged), ptr(xw), ptr(a_ij), ptr(aggr), ptr(stats), ptr(d_out),
                                                    ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid), ptr(colptr), ptr(dst), ptr(eid_t), N, E, C, H, De,
                                                    Cp, Dp, slope, ptr(d_x), ptr(ell_f[0]) if ell_f else None, ptr(ell_f[1]) if ell_f else None,
                                                    ptr(ell_t[0]) if ell_t else None, ptr(ell_t[1]) if ell_t else None, 1 if ell_t else 0,
                                                    None, ptr(ws), ws.numel(), ptr(addend), info, stream())
                if d_alias is not None and not in_kernel:
                    d_x = d_x.add_(d_alias)
                groups = _park(scope, "triplet", wn, ctx.first_app, (ws, tuple(info), x_p, aggr, d_out))
                if groups is None:
                    return d_x, d_ea, None, None, None, None, None, None, None, None, d_carry, None, None, None
        shapes = _triplet_shapes(wn, we, att, H)
        if groups is not None:
            # both weight-gradient products + k_param_grads over each group of parked operand sets, chained through the gradient carry
            carry = f32c(d_carry, "d_carry") if d_carry is not None else None
            vp = ctypes.c_void_p
            for grp in groups:
                n = len(grp)
                out, o = _flat_grads(shapes, dev)
                c = _flat_views(carry, shapes) if carry is not None else (None,) * 5
                ws2 = torch.empty(2 * lib.glam_wgrad_workspace_bytes(), dtype=torch.uint8, device=dev)
                infos = (ctypes.c_int64 * (4 * n))(*[v for t in grp for v in t[1]])
                arr = lambda i: (vp * n)(*[t[i].data_ptr() for t in grp])
                lib.glam_triplet_layer_param_grads_sets(n, arr(0), infos, arr(2), arr(3), arr(4), N, C, H, De, Cp, Dp, ptr(wn), ptr(we),
                                                        ptr(att), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(o[4]), ptr(c[0]), ptr(c[1]),
                                                        ptr(c[2]), ptr(c[3]), ptr(c[4]), ptr(ws2), ws2.numel(), stream())
                carry = out
            return d_x, d_ea, None, None, None, None, None, None, None, None, carry, None, None, None
        # the five parameter gradients are consecutive views of ONE buffer (parameter order), so a data-parallel
        # step can all-reduce them as a single bucket without a gather copy (parallel.flat_view)
        flatg, (d_wn, d_we, d_att, d_wsc, d_bias) = _flat_grads(shapes, dev)
        have_carry = ctx.carried and d_carry is not None and N > 0
        if have_carry or ell_t is not None:
            # the gradient accumulated by the later applications of the block is summed by k_param_grads itself
            c_wn, c_we, c_att, c_wsc, c_bias = _flat_views(f32c(d_carry, "d_carry"), shapes) if have_carry else (None,) * 5
            # the skip connection's gradient joins d_x in the epilogue of the d_x product (warp-specialised route)
            in_kernel = d_alias is not None and ell_t is not None and _lib.route_enabled("x3")     # (a 3 x bf16 consumer option)
            addend = f32c(d_alias, "d_identity") if in_kernel else None
            lib.glam_triplet_layer_bwd_params_ell_add(ptr(x_p), ptr(ea_p), ptr(staged), ptr(xw), ptr(a_ij), ptr(aggr), ptr(stats), ptr(d_out),
                                                      ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid), ptr(colptr), ptr(dst), ptr(eid_t), N, E, C, H, De, Cp,
                                                      Dp, slope, ptr(wn), ptr(we), ptr(att), ptr(d_x), ptr(d_wn), ptr(d_we), ptr(d_att), ptr(d_wsc),
                                                      ptr(d_bias), ptr(c_wn), ptr(c_we), ptr(c_att), ptr(c_wsc), ptr(c_bias),
                                                      ptr(ell_f[0]) if ell_f else None, ptr(ell_f[1]) if ell_f else None,
                                                      ptr(ell_t[0]) if ell_t else None, ptr(ell_t[1]) if ell_t else None, 1 if ell_t else 0,
                                                      ptr(d_ea), ptr(ws), ws.numel(), ptr(addend), stream())
            if d_alias is not None and not in_kernel:
                d_x = d_x.add_(d_alias)
            if ctx.carried:
                return d_x, d_ea, None, None, None, None, None, None, None, None, _carried(flatg, d_carry, have_carry), None, None, None
            return d_x, d_ea, d_wn, d_we, d_att, d_wsc, d_bias, None, None, None, None, None, None, None
        lib.glam_triplet_layer_bwd_params(ptr(x_p), ptr(ea_p), ptr(staged), ptr(xw), ptr(a_ij), ptr(aggr), ptr(stats), ptr(d_out), ptr(gi.rowptr),
                                          ptr(gi.src), ptr(gi.eid), ptr(colptr), ptr(dst), ptr(eid_t), N, E, C, H, De, Cp, Dp, slope, ptr(wn),
                                          ptr(we), ptr(att), ptr(d_x), ptr(d_wn), ptr(d_we), ptr(d_att), ptr(d_wsc), ptr(d_bias), ptr(d_ea), ptr(ws),
                                          ws.numel(), stream())
        if d_alias is not None:
            d_x = d_x.add_(d_alias)
        if ctx.carried:
            return d_x, d_ea, None, None, None, None, None, None, None, None, _carried(flatg, d_carry), None, None, None
        return d_x, d_ea, d_wn, d_we, d_att, d_wsc, d_bias, None, None, None, None, None, None, None


# The layer through the torch-extension operator (torch.ops.glam.triplet_layer: C++ autograd node, no ctypes marshalling, no Python
# autograd.Function) is the route for EAGERLY issued steps, which are bound by host time: full-model step issued eagerly 1.21 vs 1.48 ms
# at B = 32, 1.32 vs 1.55 ms at B = 1 024.  The Python node keeps the per-pass weight staging and the gradient carry of a weight_scope,
# which a captured hipGraph replays for free.  GLAM_TORCH_EXT: "auto" (default) = the operator while nothing is being captured and the
# batch is cache resident, "1" / "0" = always / never.  Both routes give
# the same numbers bit for bit (tested), so an eager first visit and a captured second one stay on one trajectory.
_ext_env = os.environ.get("GLAM_TORCH_EXT", "auto")
USE_TORCH_EXT = True if _ext_env == "1" else False if _ext_env == "0" else "auto"
_EXT_OK = None


def _want_torch_ext(N, H, Cp):
    global _EXT_OK
    if USE_TORCH_EXT is False or N <= 0 or CACHED_STAGING:     # (the C++ node stages per call)
        return False
    if USE_TORCH_EXT == "auto":
        if torch.cuda.is_current_stream_capturing() or GraphIndex.wants_ell(N, H, Cp):
            return False
        if _EXT_OK is None and os.environ.get("GLAM_HIP_LIB"):
            _EXT_OK = False            # the shim is linked against the in-tree libglam_hip.so, not against a substituted build
        if _EXT_OK is None:
            try:
                from . import torch_ext
                torch_ext.load()
                _EXT_OK = True
            except Exception:          # noqa: BLE001 - the shim is optional in auto mode: the Python node is the same HIP path
                _EXT_OK = False
        return _EXT_OK
    return True


def triplet_layer(x_p, ea_p, weight_node, weight_edge, att, weight_scale, bias, gi, heads, slope=0.2, with_identity=False):
    """``TripletMessage.forward`` (src_1gp/layer.py:36-61) in padded widths: ``x_p[N,Cp] -> out[N,Cp]``.  ``with_identity``: returns
    ``(out, identity)`` where ``identity`` is ``x_p`` handed back through the layer's autograd node (see _TripletLayer.forward) — or
    plain ``x_p`` on the routes that have nothing to gain from it."""
    if with_identity and not (torch.is_grad_enabled() and x_p.requires_grad) or _want_torch_ext(gi.N, heads, x_p.size(1)) and with_identity:
        return triplet_layer(x_p, ea_p, weight_node, weight_edge, att, weight_scale, bias, gi, heads, slope), x_p
    if _want_torch_ext(gi.N, heads, x_p.size(1)):
        from . import torch_ext
        # the one-time read-backs of the ELL routes happen on an eager visit (a later CAPTURED visit of the same batch finds them
        # cached); with them the C++ node launches the same warp-specialised kernels as the Python node: one trajectory, bit for bit
        ell_f = ell_b = None
        onehot = False
        if _ws_route(_lib.api(), gi.N, heads, x_p.size(1), ea_p.size(1), ea_p):
            onehot = True
            ell_f = gi.ell()
            if torch.is_grad_enabled():
                ell_b = gi.ell_t()
        # same checks, same exception type as the Python node (the operator's own TORCH_CHECKs would raise RuntimeError)
        require_device(x_p, ea_p, weight_node, weight_edge, att, weight_scale, bias)
        C = weight_node.size(0)
        if (x_p.dim() != 2 or ea_p.dim() != 2 or gi.N != x_p.size(0) or ea_p.size(0) != gi.E or weight_node.shape != (C, heads * C)
                or weight_scale.shape != (heads * C, C) or x_p.size(1) != (C + 3) // 4 * 4):
            raise GlamHipError("triplet_layer: shape mismatch")
        t_ptr = gi.transpose() if torch.is_grad_enabled() else (gi.rowptr, gi.src, gi.eid)     # any int32 tensors when no backward follows
        return torch_ext.load().triplet_layer(f32c(x_p, "x"), f32c(ea_p, "edge_attr"), weight_node, weight_edge, att, weight_scale, bias,
                                              gi.rowptr, gi.src, gi.eid, t_ptr[0], t_ptr[1], t_ptr[2], heads, float(slope),
                                              ell_f[0] if ell_f else None, ell_f[1] if ell_f else None,
                                              ell_b[0] if ell_b else None, ell_b[1] if ell_b else None, onehot)
    params = (weight_node, weight_edge, att, weight_scale, bias)
    carry = _Carry(("carry-triplet", id(weight_node)), params, _triplet_shapes(weight_node, weight_edge, att, heads))
    if carry.tensor is None:
        # no backward can follow (torch.no_grad(), or nothing that requires a gradient): the inference forward
        no_backward = not (torch.is_grad_enabled() and any(t.requires_grad for t in (x_p, ea_p) + params))
        return _TripletLayer.apply(x_p, ea_p, weight_node, weight_edge, att, weight_scale, bias, gi, heads, slope, None, with_identity, True, no_backward)
    # the parameters still enter as inputs (the kernels read them, and the scope's staging cache is keyed on them), but this
    # node returns no gradient for them: it flows through `carry`
    res = _TripletLayer.apply(x_p, ea_p, weight_node, weight_edge, att, weight_scale, bias, gi, heads, slope, carry.tensor, with_identity, carry.first)
    carry.store(res[-1])
    return (res[0], res[1]) if with_identity else res[0]


class _TripletLayerWide(torch.autograd.Function):
    """TripletMessage for widths beyond the fused kernels' table (H*Cp + 8 > 192; hid_dim_alpha = 6 of glam.py:60) as ONE
    autograd node: ``k_stage_plain`` -> library GEMMs for the data-side products -> the aggregate kernels -> ``k_wgrad``
    for both N-deep weight gradients (written straight into the ``dstaged`` layout) -> ``k_stage_params_bwd``.
    No per-parameter torch glue on either pass."""

    @staticmethod
    def forward(ctx, x_p, ea_p, wn, we, att, wsc, bias, gi, H, slope, carry=None, first_app=True):
        require_device(x_p, ea_p, wn, we, att, wsc, bias)
        ctx.first_app = bool(first_app)
        x_p, ea_p = f32c(x_p, "x"), f32c(ea_p, "edge_attr")
        wn, we, att, wsc, bias = (f32c(t, n) for t, n in ((wn, "weight_node"), (we, "weight_edge"),
                                                           (att, "weight_triplet_att"), (wsc, "weight_scale"), (bias, "bias")))
        C, De = wn.size(0), we.size(0)
        N, Cp = x_p.shape
        Dp = ea_p.size(1)
        HC = H * Cp
        if gi.N != N or ea_p.size(0) != gi.E or wn.shape != (C, H * C) or wsc.shape != (H * C, C) or Cp != (C + 3) // 4 * 4:
            raise GlamHipError("triplet_layer_wide: shape mismatch")
        ctx.carried = carry is not None      # gradient carry of the block's parameters (see _Carry)
        if ctx.carried:
            ctx.set_materialize_grads(False)
        lib, dev = _lib.api(), x_p.device
        f = dict(dtype=torch.float32, device=dev)

        def build():
            buf = torch.empty(lib.glam_triplet_plain_floats(H, Cp, Dp), **f)
            lib.glam_triplet_stage_plain(ptr(wn), ptr(we), ptr(att), ptr(wsc), ptr(bias), C, H, De, Cp, Dp, ptr(buf), stream())
            return buf

        scope = ctx.scope = _SCOPE
        plain = scope_build(scope, "fwd", triplet_key(wn, we, att, wsc, bias, plain=True), wn, build)
        Wcat, Ws_p, We_p, M, bias_p = _plain_views(plain, H, Cp, Dp)
        xw, a_ij = torch.empty(N, HC, **f), torch.empty(N, 8, **f)
        aggr, stats, out = torch.empty(N, HC, **f), torch.empty(N, 8, **f), torch.empty(N, Cp, **f)
        mfma, tall = _wide_gemms_supported(H, Cp), _wide_tall_supported(H, Cp)
        st = stream()
        if scope is not None and any(ctx.needs_input_grad):
            # the four GEMM images of the pass (two for the forward, two for the backward) from one launch instead of four
            prestage(None, ([wide_node_image(wn, W=Wcat), wide_dagg_image(wn, W=Ws_p)] if mfma else []) +
                     ([wide_upd_image(wn, W=Ws_p), wide_dx_image(wn, W=Wcat)] if tall else []))
        if mfma:     # the 120 KB-image k_ts_gemm variant: xw and a_ij in one launch
            img1 = scoped_image(scope, wide_node_image, wn, W=Wcat)
            lib.glam_ts_gemm(ptr(x_p), Cp, Cp, None, 0, 0, ptr(img1), None, ptr(xw), HC, HC, ptr(a_ij), 8, 8, N, st)
        else:
            torch.matmul(x_p, Wcat[:, :HC], out=xw)                        # layer.py:37
            torch.matmul(x_p, Wcat[:, HC:], out=a_ij)                      # separable attention scalars a_i | a_j
        lib.glam_triplet_fwd(ptr(xw), ptr(a_ij), ptr(ea_p), ptr(We_p), ptr(M), ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid),
                             N, gi.E, H, Cp, Dp, 1, float(slope), ptr(aggr), ptr(stats), st)
        if tall:      # layer.py:57-61, 276 -> 92: the long-reduction 3 x bf16 kernel (tall_x3.hip)
            img2 = scoped_image(scope, wide_upd_image, wn, W=Ws_p)
            lib.glam_ts_gemm(ptr(aggr), HC, HC, None, 0, 0, ptr(img2), ptr(bias_p), ptr(out), Cp, Cp, None, 0, 0, N, st)
        else:
            torch.addmm(bias_p, aggr, Ws_p, out=out)
        ctx.save_for_backward(x_p, ea_p, wn, we, att, plain, xw, a_ij, aggr, stats)
        ctx.gi, ctx.dims = gi, (C, H, De, Cp, Dp, float(slope))
        return (out, carry.view(-1)) if ctx.carried else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_carry=None):
        if d_out is None:                    # the layer's output was not used: only the carry (if any) passes through
            return (None,) * 10 + (d_carry, None)
        x_p, ea_p, wn, we, att, plain, xw, a_ij, aggr, stats = ctx.saved_tensors
        C, H, De, Cp, Dp, slope = ctx.dims
        gi = ctx.gi
        N, E, HC = gi.N, gi.E, H * Cp
        lib, dev = _lib.api(), x_p.device
        f = dict(dtype=torch.float32, device=dev)
        d_out = f32c(d_out, "d_out")
        if N == 0:        # an empty batch: every gradient is zero
            z = lambda t: torch.zeros_like(t)
            if ctx.carried:
                return (torch.zeros_like(x_p), torch.zeros_like(ea_p) if ctx.needs_input_grad[1] else None) + (None,) * 8 + (d_carry, None)
            return (torch.zeros_like(x_p), torch.zeros_like(ea_p) if ctx.needs_input_grad[1] else None, z(wn), z(we), z(att),
                    torch.zeros(H * C, C, **f), torch.zeros(C, **f), None, None, None, None, None)
        Wcat, Ws_p, We_p, M, _ = _plain_views(plain, H, Cp, Dp)
        colptr, dst, eid_t = gi.transpose()
        # dstaged: d_Wcat[Cp, HC+8] | d_WsB[HC+1, Cp] | d_We_p[Dp, HC] | d_M[Dp, 4]   (include/glam_hip.h)
        o_wsb = Cp * (HC + 8)
        o_we = (o_wsb + (HC + 1) * Cp + 3) // 4 * 4
        o_m = o_we + Dp * HC
        dstaged = torch.empty(lib.glam_triplet_dstaged_floats(H, Cp, Dp), **f)
        mfma = _wide_gemms_supported(H, Cp)
        scope = ctx.scope
        if mfma:
            img3 = scoped_image(scope, wide_dagg_image, wn, W=Ws_p)
            d_aggr = torch.empty(N, HC, **f)
            lib.glam_ts_gemm(ptr(d_out), Cp, Cp, None, 0, 0, ptr(img3), None, ptr(d_aggr), HC, HC, None, 0, 0, N, stream())
        else:
            d_aggr = torch.matmul(d_out, Ws_p.t())
        d_xw, d_a = torch.empty(N, HC, **f), torch.empty(N, 8, **f)
        d_ea = torch.zeros_like(ea_p) if ctx.needs_input_grad[1] else None
        ws = torch.empty(lib.glam_triplet_bwd_workspace_bytes(N, E, H, Cp, Dp), dtype=torch.uint8, device=dev)
        lib.glam_triplet_bwd(ptr(xw), ptr(a_ij), ptr(ea_p), ptr(We_p), ptr(M), ptr(aggr), ptr(stats), ptr(d_aggr), ptr(gi.rowptr), ptr(gi.src),
                             ptr(gi.eid), ptr(colptr), ptr(dst), ptr(eid_t), N, E, H, Cp, Dp, 1, slope, ptr(d_xw), ptr(d_a), ptr(dstaged[o_we:]),
                             ptr(dstaged[o_m:]), ptr(d_ea), ptr(ws), ws.numel(), stream())
        if _wide_tall_supported(H, Cp):      # d_x = [d_xw | d_a] @ Wcat^T: both sources in one launch
            img4 = scoped_image(scope, wide_dx_image, wn, W=Wcat)
            d_x = torch.empty(N, Cp, **f)
            lib.glam_ts_gemm(ptr(d_xw), HC, HC, ptr(d_a), 8, 8, ptr(img4), None, ptr(d_x), Cp, Cp, None, 0, 0, N, stream())
        else:
            d_x = torch.matmul(d_xw, Wcat[:, :HC].t())
            d_x.addmm_(d_a, Wcat[:, HC:].t())
        if ctx.carried and Cp <= 128 and _parks(scope, N):
            # the parameter gradients of ALL applications of the layer from one set of launches (see _park): every application parks
            # its operands (and its small d_W_edge / d_M sums); the first one runs both N-deep products over the parked sets
            # (glam_wgrad_gemm_sets2) and the chain rule (k_stage_params_bwd is linear in dstaged) ONCE
            groups = _park(scope, "wide", wn, ctx.first_app, (aggr, d_out, d_xw, d_a, x_p, dstaged))
            if groups is None:
                return d_x, d_ea, None, None, None, None, None, None, None, None, d_carry, None
            vp = ctypes.c_void_p
            small = dstaged[o_we:]                       # d_We_p | d_M: sums over the applications (its own set is parked last)
            for t in [t for grp in groups for t in grp][:-1]:
                small.add_(t[5][o_we:])
            for g, grp in enumerate(groups):
                n = len(grp)
                arr = lambda i: (vp * n)(*[t[i].data_ptr() for t in grp])
                wws = torch.empty(lib.glam_wgrad_workspace_bytes(), dtype=torch.uint8, device=dev)
                lib.glam_wgrad_gemm_sets2(n, arr(0), HC, HC, None, 0, 0, 1, arr(1), Cp, Cp, N, ptr(dstaged[o_wsb:]), Cp, 1,
                                          None if g == 0 else ptr(dstaged[o_wsb:]), ptr(wws), wws.numel(), stream())
                wws2 = torch.empty(lib.glam_wgrad_workspace_bytes(), dtype=torch.uint8, device=dev)
                lib.glam_wgrad_gemm_sets2(n, arr(2), HC, HC, arr(3), 8, 8, 0, arr(4), Cp, Cp, N, ptr(dstaged), 1, HC + 8,
                                          None if g == 0 else ptr(dstaged), ptr(wws2), wws2.numel(), stream())
        else:
            wws = torch.empty(lib.glam_wgrad_workspace_bytes(), dtype=torch.uint8, device=dev)
            # d_WsB = [aggr | 1]^T d_out ;  d_Wcat = x^T [d_xw | d_a], computed as ([d_xw | d_a]^T x)^T
            lib.glam_wgrad_gemm(ptr(aggr), HC, HC, None, 0, 0, 1, ptr(d_out), Cp, Cp, 0, N, ptr(dstaged[o_wsb:]), Cp, 1,
                                ptr(wws), wws.numel(), stream())
            lib.glam_wgrad_gemm(ptr(d_xw), HC, HC, ptr(d_a), 8, 8, 0, ptr(x_p), Cp, Cp, 0, N, ptr(dstaged), 1, HC + 8,
                                ptr(wws), wws.numel(), stream())
        flatg, (d_wn, d_we, d_att, d_wsc, d_bias) = _flat_grads(_triplet_shapes(wn, we, att, H), dev)
        lib.glam_triplet_stage_params_bwd(ptr(wn), ptr(we), ptr(att), ptr(dstaged), C, H, De, Cp, Dp, ptr(d_wn), ptr(d_we),
                                          ptr(d_att), ptr(d_wsc), ptr(d_bias), stream())
        if ctx.carried:       # one add of the flat buffer per application instead of five per-parameter accumulations
            return d_x, d_ea, None, None, None, None, None, None, None, None, _carried(flatg, d_carry), None
        return d_x, d_ea, d_wn, d_we, d_att, d_wsc, d_bias, None, None, None, None, None


def _wide_gemms_supported(H, Cp):
    return Cp <= 96 and H * Cp + 8 <= 320


def _wide_tall_supported(H, Cp):
    """The long-reduction products of the wide layer (H Cp (+ 8) -> Cp) inside tall_x3.hip's table (K <= 288, M <= 96)."""
    return _wide_gemms_supported(H, Cp) and H * Cp + 8 <= 288


def _plain_views(plain, H, Cp, Dp):
    HC = H * Cp
    n1, n2, n3, n4 = Cp * (HC + 8), HC * Cp, Dp * HC, Dp * 4
    return (plain[:n1].view(Cp, HC + 8), plain[n1:n1 + n2].view(HC, Cp), plain[n1 + n2:n1 + n2 + n3].view(Dp, HC),
            plain[n1 + n2 + n3:n1 + n2 + n3 + n4].view(Dp, 4), plain[n1 + n2 + n3 + n4:])


def wide_layer_supported(C, heads, De):
    """Widths the one-node wide path covers (k_wgrad: up to 320 + 128 columns): C <= 100 at 3 heads."""
    Cp = (C + 3) // 4 * 4
    return heads * Cp + 8 <= 320 and Cp <= 128 and De <= 8 and 1 <= heads <= 4


def triplet_layer_wide(x_p, ea_p, weight_node, weight_edge, att, weight_scale, bias, gi, heads, slope=0.2):
    params = (weight_node, weight_edge, att, weight_scale, bias)
    carry = _Carry(("carry-triplet-wide", id(weight_node)), params, _triplet_shapes(weight_node, weight_edge, att, heads))
    if carry.tensor is None:
        return _TripletLayerWide.apply(x_p, ea_p, weight_node, weight_edge, att, weight_scale, bias, gi, heads, slope)
    out, carry_out = _TripletLayerWide.apply(x_p, ea_p, weight_node, weight_edge, att, weight_scale, bias, gi, heads, slope, carry.tensor, carry.first)
    carry.store(carry_out)
    return out


# --------------------------------------------------------------------------------------
# device-side random stream of the training-mode layers (RReLU slopes, Dropout masks): csrc/rng.h
# --------------------------------------------------------------------------------------
_RNG_STATE: dict = {}
RNG_STATE_WORDS = 288          # include/glam_hip.h: GLAM_RNG_STATE_WORDS


def rng_state(device):
    """``int64[288]`` on ``device``: [0] Philox seed, [1] stream offset (advanced by every RNG-consuming launch, on the device), [16] and
    [32 + 16 s] tickets (include/glam_hip.h: GLAM_RNG_STATE_WORDS).
    Created on first use from ``torch.initial_seed()`` — so the reference's ``seed_torch`` (``utils.py:22-28``) also fixes this
    stream — and OUTSIDE any hipGraph capture (``GraphedTrainStep`` runs the first visit of a batch eagerly)."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    st = _RNG_STATE.get(key)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            raise GlamHipError("the RNG state must exist before a hipGraph capture: run one eager training-mode forward first "
                               "(or call glam_amd.ops.manual_seed)")
        st = _RNG_STATE[key] = torch.tensor([torch.initial_seed() & (2 ** 63 - 1)] + [0] * (RNG_STATE_WORDS - 1), dtype=torch.int64, device=device)
    return st


def manual_seed(seed, device=None):
    """Restart the device-side stream of RReLU / Dropout numbers at ``(seed, offset 0)``."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = rng_state(device)
    st.copy_(torch.tensor([int(seed) & (2 ** 63 - 1)] + [0] * (RNG_STATE_WORDS - 1), dtype=torch.int64))
    return st


# A tail kernel that also wrote Dropout(p)(out) — the input of the NEXT message step's conv (layer.py:255-259) — registers the
# pair here; the block's dropout call on that very tensor then returns the twin instead of launching a kernel.
_DROPPED = TensorMemo("ptr")      # out -> (out_drop, p)


def register_dropped(out, out_drop, p):
    _DROPPED.put(out, (out_drop, float(p)))


def take_dropped(x, p):
    hit = _DROPPED.get(x)
    if hit is not None and hit[1] == float(p):
        return _DROPPED.take(x)[0]
    return None


_ONEHOT_CACHE = TensorMemo("id")      # tensor -> whether its rows are one-hot


def rows_are_one_hot(t):
    """True iff every row of ``t`` is one-hot (one host sync, cached per tensor object like the CSR staging).  Inside a stream capture an
    answer that is not cached yet is ``False`` (no read-back there): the contraction path is always correct."""
    ok = _ONEHOT_CACHE.get(t)
    if ok is not None:
        return ok
    mark = getattr(t, "_glam_onehot", None)      # (flag, tensor version) known from the host side (data.PackedDataset): no read-back
    if not (mark is not None and mark[1] == t._version) and t.is_cuda and torch.cuda.is_current_stream_capturing():
        return False
    ok = bool(mark[0]) if (mark is not None and mark[1] == t._version) else \
        (bool((((t == 0) | (t == 1)).all() & (t.sum(dim=1) == 1).all()).item()) if t.numel() else True)
    _ONEHOT_CACHE.put(t, ok)
    return ok


# ---- knobs of the dense / readout operators (glam_amd/ops_dense.py, ops_readout.py read them through this module) ----
GEMM_PAIR = True     # A/B knob: the GRU's two products per direction in one launch
# Gate GEMMs + gate math + tail of the forward GRU step in ONE launch (glam_gru_fused_fwd, bit-identical to the pair launch + tail
# kernel, tested).  Its work item is coarse (a 16-row tile x both products x all three gates) and its epilogue runs at the chip's write
# bandwidth, so it pays once a wave has several tiles to pipeline: model step at B = 8 192 3.90 vs 4.08 ms, B = 1 024 0.807 vs 0.814 ms,
# B = 32 0.384 vs 0.370 ms (the 96 KB of weight images per block dominate).  "auto": from GRU_FUSED_MIN_NODES nodes on.
GRU_FUSED = "auto"
GRU_FUSED_MIN_NODES = 16384
# The same step warp-specialised on the bf16 matrix cores in 3 x bf16 form (glam_gru_ws_fwd: fp32 accuracy, different roundings than the
# fp32 launches above; 24 <= C <= 64): the default where it applies.
GRU_WS = "1"
# MessageBlock's skip connection handed through the conv's autograd node (the d_x product's epilogue sums both gradient paths): A/B switch
SKIP_THROUGH_CONV = True
# the weight gradients of all applications of a block from one product over their parked operand sets (see _park): A/B switch
GRU_WGRAD_BATCH = True
# the warp-specialised GRU step on pre-split operand fragments of its gate matrices (glam_gru_ws_make_pre) instead of splitting the plain
# images in every block's prologue: A/B switch (GLAM_GRU_PRE=0)
GRU_PRE = os.environ.get("GLAM_GRU_PRE", "1") != "0"
# the warp-specialised GRU step keeps THE GATES [r | z | n | gh_n] (4C floats per row) for its backward instead of both pre-activation
# matrices (6C), and the backward writes ONE gate-gradient matrix [N, 4C] instead of d_gi and d_gh (they share two of three blocks):
# A/B switch (GLAM_GRU_GATES=0)
GRU_GATES = os.environ.get("GLAM_GRU_GATES", "1") != "0"
# a MessageBlock that is applied again (src_1gp/model.py:53-54) has the GRU step of one application write the node product
# x @ [W_node | Wa] of the next (block.hip: k_gru_fwd_ws + node; glam_gru_ws_fwd_pre_node), whose TripletMessage then starts at its
# aggregate launch: A/B switch (GLAM_NODE_IN_GRU=0)
NODE_IN_GRU = os.environ.get("GLAM_NODE_IN_GRU", "1") != "0"
# the training-mode RReLU of a LinearBlock (and the dropped twin behind it) in the epilogue of its product where that runs on k_tall_x3
# (the input embeddings) instead of a launch of its own: A/B switch (GLAM_RRELU_IN_GEMM=0)
RRELU_IN_GEMM = os.environ.get("GLAM_RRELU_IN_GEMM", "1") != "0"
# the output head applies the training-mode RReLU of the layer in front of it and its own Dropout to the elements it reads
# (glam_linear_narrow_act_*): no activated matrix, no dropped twin, two launches less each way: A/B switch (GLAM_HEAD_ACT=0)
HEAD_ACT_FUSED = os.environ.get("GLAM_HEAD_ACT", "1") != "0"
# ... while a launch saved outweighs the matrix and vector work the node product adds to the GRU step's four SIMDs (A/B on one box,
# model step: B = 32 -3.5 %, 1 024 -1.5 %, 2 048 -1.2 %, 4 096 +0.6 %, 8 192 +1.0 %)
NODE_IN_GRU_MAX_ROWS = 65536
_FEEDS_ITSELF = False


@contextlib.contextmanager
def block_feeds_itself(on=True):
    """The caller's statement that the output of the MessageBlock applications inside goes into the SAME block again (model.py:53-54:
    all but the last of the message_steps applications)."""
    global _FEEDS_ITSELF
    prev, _FEEDS_ITSELF = _FEEDS_ITSELF, bool(on)
    try:
        yield
    finally:
        _FEEDS_ITSELF = prev


_NODE_PRODUCTS = TensorMemo("ptr")      # rows -> (rows.shape, staged, xw, a_ij)


def register_node_product(rows, staged, xw, a_ij):
    """``xw | a_ij = rows @ [W_node | Wa]`` of the layer whose staged images are ``staged`` exist already (the GRU step that wrote ``rows``
    wrote them): ``_TripletLayer`` takes them when exactly these rows arrive with exactly these images."""
    _NODE_PRODUCTS.put(rows, (tuple(rows.shape), staged, xw, a_ij))


def take_node_product(x, staged):
    hit = _NODE_PRODUCTS.get(x, same_object=False)      # the consumer may hold another tensor object over the same rows
    if hit is None or hit[0] != tuple(x.shape) or not x.is_contiguous() or hit[1] is not staged or not NODE_IN_GRU:
        return None
    return _NODE_PRODUCTS.take(x, same_object=False)[2:]


def first_node_spec(conv, N, edge_index, edge_attr):
    """``(staged, H * Cp)`` when the TripletMessage ``conv`` will take the node product of its FIRST input from the launch that writes that
    input (the input embedding: ``linear_relu`` / ``linear_rrelu`` with ``node=``): its staged images exist already (``prestage``), and the
    call will run on the warp-specialised route (one-hot bond features, an ELL form of the edge list).  Else None."""
    if not (NODE_IN_GRU and _SCOPE is not None and not CACHED_STAGING and N > 0):
        return None
    C, H, De = conv.node_channels, conv.heads, conv.edge_channels
    if C % 4 or De != 4 or not (1 <= H <= 4 and fused_layer_supported(C, H, De)) or H * C + 8 <= 64 or N > NODE_IN_GRU_MAX_ROWS or _want_torch_ext(N, H, C):
        return None
    wn = conv.weight_node
    staged = _SCOPE.lookup("fwd", triplet_key(wn, conv.weight_edge, conv.weight_triplet_att, conv.weight_scale, conv.bias), wn)
    if staged is None or edge_attr is None or edge_attr.dim() != 2 or edge_attr.size(1) != De or edge_attr.dtype != torch.float32:
        return None
    if not _ws_route(_lib.api(), N, H, C, De, edge_attr) or graph_index(edge_index, N).ell() is None:
        return None
    return staged, H * C


def next_node_spec(conv, N):
    """``(staged, H * Cp)`` when the TripletMessage ``conv`` — applied a moment ago inside the active weight scope — will take its next
    input's node product from the GRU step (warp-specialised route, unpadded width), else None."""
    if not (NODE_IN_GRU and _FEEDS_ITSELF and _SCOPE is not None and not CACHED_STAGING and GRU_PRE and GRU_WS == "1"):
        return None
    C, H, De = conv.node_channels, conv.heads, conv.edge_channels
    if C % 4 or not (1 <= H <= 4 and fused_layer_supported(C, H, De)) or H * C + 8 <= 64 or N > NODE_IN_GRU_MAX_ROWS or _want_torch_ext(N, H, C):
        return None
    wn = conv.weight_node
    staged = _SCOPE.lookup("fwd", triplet_key(wn, conv.weight_edge, conv.weight_triplet_att, conv.weight_scale, conv.bias), wn)
    if staged is None or _SCOPE.lookup("fwd", triplet_ell_key(wn), wn) is None:
        return None
    return staged, H * C
# the readout MLP's products of few tiles split k across blocks (glam_linear_dense_*_ws; matters at the reference's batch of 32): A/B switch
DENSE_SPLITK = os.environ.get("GLAM_DENSE_SPLITK", "1") != "0"
# PairNorm + the Dropout behind it from one launch each way (glam_graph_norm_drop_*): A/B switch
NORM_DROP = True
# the derived weights of a model pass from one launch (glam_prestage) instead of one per module: A/B switch
PRESTAGE = True
# the readout MLP's linear on csrc/dense_x3.hip (0: the GEMM library + separate activation / mask / column-sum launches): A/B switch
DENSE_LINEAR = True
# _BatchNorm and the batch-less _LayerNorm on csrc/colnorm.hip (False: torch.nn.BatchNorm1d / the elementwise torch expression): A/B switch
COLUMN_NORM = True
# the backward of a ReLU fused into a linear, inside that linear's weight-gradient product (glam_wgrad_gemm_split_relu) where the product
# is the gradient's only consumer: A/B switch (False: an elementwise launch in front of the product)
RELU_IN_WGRAD = True
# a TripletMessage forward that no backward can follow (torch.no_grad()) stores neither aggr nor stats: A/B switch
INFER_FWD = os.environ.get("GLAM_INFER_FWD", "1") != "0"


# ---- the dense, readout, pair-fusion and column-norm operator families live in their own modules; their names are part of this namespace ----
from . import ops_dense as _ops_dense, ops_norm as _ops_norm, ops_pair as _ops_pair, ops_readout as _ops_readout     # noqa: E402  (they read this module's state at call time)

for _m in (_ops_dense, _ops_readout, _ops_pair, _ops_norm):
    for _k, _v in vars(_m).items():
        if not _k.startswith("__") and _k != "_o" and _k not in globals():
            globals()[_k] = _v
del _m, _k, _v
