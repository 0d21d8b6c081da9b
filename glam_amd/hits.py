"""Screening hit lists: per query (a cached protein), the best ``k`` candidates of a stream of score batches, kept on the device
(``csrc/hits.hip``: ``glam_hits_reset`` / ``glam_hits_merge``).

A screening campaign does not want the ``[L, Qs, out_dim]`` scores of every batch; it wants the best ``k`` ligands per target of a
library far longer than any batch.  ``HitList`` holds ``Qs x k`` (score, id) pairs however long the library is; ``update`` merges one
batch into them with two HIP launches, no read-back and no ATen kernel, so a loop of ``screen_panel`` + ``update`` stays as free of
host synchronisation as ``screen_panel`` itself (``ArchitectureDTI.screen_top`` is that loop).

The order — ONE total order, and the lists are exact under it: better score first (larger with ``largest``, smaller without; ``-0.0``
and ``+0.0`` are equal), equal scores by ascending id, NaN scores after every number (among themselves by ascending id), unfilled slots
(score NaN, id -1) last.  The stored scores are the candidates' own bits."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import GlamHipError, ptr, require_device, stream
from .ops_pair import _stage_int32

MAX_ID = 2 ** 31 - 1      # ids are int32


def check_k(k, who="HitList"):
    """``k`` as an int the kernels have a list for (1..1024, ``glam_hits_supported``), or ``GlamHipError``."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise GlamHipError(f"{who}: k must be an integer, got {k!r}")
    if _lib.load().glam_hits_supported(int(k)) != 0:          # (a status: the raw binding hands it back)
        raise GlamHipError(f"{who}: k = {k} is outside the kernels' lists (1..1024)")
    return int(k)


def update_plan(scores, ids, task, queries, offered):
    """What ``HitList.update`` settles on the host before anything is launched — for a list of ``queries`` columns that was offered
    ``offered`` candidates so far: ``(L, offset, ld_row, ld_col, ids)`` with ``scores.data_ptr() + 4 * offset`` the score of candidate 0
    for query 0, the two strides in elements, and ``ids`` an int32 numpy vector (host ids), the device tensor as given, or ``None``.
    Refusals (``GlamHipError`` unless said): ``scores`` not a float32 tensor or of another shape than ``[L, queries]`` / ``[L, queries,
    out_dim]`` (with one query also ``[L]`` / ``[L, out_dim]``); ``task`` outside the task columns; ``ids`` of the wrong dtype, shape or
    count, or with an entry outside ``[0, 2^31 - 1]`` (host ids: ``IndexError``, as ``ops.host_ints``); default ids that would pass
    ``2^31 - 1``.  Touches no device: a device ``ids`` is checked by dtype and shape only."""
    if not torch.is_tensor(scores) or scores.dtype != torch.float32:
        raise GlamHipError(f"HitList.update: scores must be a float32 tensor, got {scores.dtype if torch.is_tensor(scores) else type(scores).__name__}")
    if isinstance(task, bool) or not isinstance(task, (int, np.integer)):
        raise GlamHipError(f"HitList.update: task must be an integer, got {task!r}")
    shape, st = tuple(scores.shape), scores.stride()
    if queries == 1 and scores.dim() in (1, 2):                # [L] or [L, out_dim]
        L, ld_row, ld_col = shape[0], st[0], 0
        tasks, ld_task = (1, 0) if scores.dim() == 1 else (shape[1], st[1])
    elif scores.dim() in (2, 3) and shape[1] == queries:       # [L, Qs] or [L, Qs, out_dim]
        L, ld_row, ld_col = shape[0], st[0], st[1]
        tasks, ld_task = (1, 0) if scores.dim() == 2 else (shape[2], st[2])
    else:
        raise GlamHipError(f"HitList.update: scores must be [L, {queries}] or [L, {queries}, out_dim]"
                           + (", [L] or [L, out_dim]" if queries == 1 else "") + f", got {shape}")
    if L and not 0 <= task < tasks:
        raise GlamHipError(f"HitList.update: task = {task} is outside the {tasks} task column(s) of scores {shape}")
    if L > MAX_ID:
        raise GlamHipError(f"HitList.update: scores holds {L} candidates, a call takes at most 2^31 - 1")
    if ids is None:
        if offered + L - 1 > MAX_ID:
            raise GlamHipError(f"HitList.update: {offered} candidates were offered and {L} more would take the default ids past 2^31 - 1: "
                               "pass ids of your own, or keep one list per 2^31 candidates")
    elif torch.is_tensor(ids) and ids.device.type != "cpu":
        if ids.dtype != torch.int32 or tuple(ids.shape) != (L,) or not ids.is_contiguous():
            raise GlamHipError(f"HitList.update: device ids must be a contiguous int32 [{L}] tensor (one per candidate), got {ids.dtype} "
                               f"{tuple(ids.shape)}; they are trusted to lie in [0, 2^31 - 1] — host ids are checked")
    else:
        ids = ops.host_ints(ids, "ids", "have one entry per candidate", n=L, below=MAX_ID + 1).astype(np.int32)
    return L, (task * ld_task if L else 0), ld_row, ld_col, ids


class HitList:
    """The best ``k`` candidates of each of ``queries`` columns, on ``device``: ``update`` offers a batch of scores, ``result`` hands
    the lists back, ``reset`` empties them.  ``largest``: whether a larger score is better.  ``k`` in 1..1024.

    Ids.  A candidate's id is the caller's (``ids``) or, by default, its position in everything offered so far (a count kept on the
    device, so it continues across hipGraph replays).  Caller ids are NOT deduplicated: a ligand offered twice can hold two slots.

    ``offered`` is the host's count of candidates offered, kept only to refuse a default id past ``2^31 - 1`` before the launch;
    a replayed capture of ``update`` does not pass through the host, so whoever replays adds the replayed candidates to it."""

    def __init__(self, queries, k, device, largest=True):
        self.k = check_k(k)
        if isinstance(queries, bool) or not isinstance(queries, (int, np.integer)) or queries < 0:
            raise GlamHipError(f"HitList: queries must be a non-negative integer, got {queries!r}")
        self.queries, self.largest, self.device = int(queries), bool(largest), torch.device(device)
        if self.device.type != "cuda":
            raise GlamHipError(f"HitList: the lists live on an MI355X HIP device (got device '{self.device}'); there is no CPU fallback")
        self.scores = torch.empty(self.queries, self.k, dtype=torch.float32, device=self.device)
        self.ids = torch.empty(self.queries, self.k, dtype=torch.int32, device=self.device)
        self.seen = torch.empty(1, dtype=torch.int64, device=self.device)
        self.device = self.scores.device                      # ('cuda' -> 'cuda:N')
        self.offered, self._ws = 0, None
        self.reset()

    def reset(self):
        """Empty lists (score NaN, id -1) and a count of zero: one launch."""
        require_device(self.scores)
        _lib.api().glam_hits_reset(ptr(self.scores), ptr(self.ids), ptr(self.seen), self.queries, self.k, stream())
        self.offered = 0
        return self

    def update(self, scores, ids=None, task=0, slabs=0):
        """Offer the ``L`` candidates of ``scores`` — float32 on the lists' device, ``[L, queries]`` or ``[L, queries, out_dim]`` (column
        ``task``), with one query also ``[L]`` or ``[L, out_dim]``, of ANY strides: it is read in place, never copied — to the lists.
        ``ids``: host integers (sequence / numpy / CPU tensor, one per candidate, in ``[0, 2^31 - 1]``: validated, then staged once),
        an int32 device tensor ``[L]`` (trusted), or ``None`` = the running count.  Two launches, no host synchronisation; with
        ``ids=None`` or a device ``ids`` the call can be captured in a hipGraph.  ``slabs``: blocks per column, 0 = the library chooses;
        the result does not depend on it.  Refusals: ``update_plan``; a CPU ``scores`` or one on another device raises."""
        L, offset, ld_row, ld_col, ids = update_plan(scores, ids, task, self.queries, self.offered)
        require_device(scores, self.scores, ids if torch.is_tensor(ids) else None)          # (host ids are a numpy vector by now)
        if isinstance(slabs, bool) or not isinstance(slabs, (int, np.integer)) or slabs < 0:
            raise GlamHipError(f"HitList.update: slabs must be 0 (choose) or the blocks per column, got {slabs!r}")
        if L and self.queries:
            if isinstance(ids, np.ndarray):
                ids = _stage_int32(ids, self.device, "HitList.update: a host ids vector")
            lib = _lib.api()
            need = lib.glam_hits_workspace_bytes(L, self.queries, self.k)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            lib.glam_hits_merge(scores.data_ptr() + 4 * offset, ld_row, ld_col, ptr(ids), L, self.queries, self.k, int(self.largest),
                                int(slabs), ptr(self.scores), ptr(self.ids), ptr(self.seen), ptr(self._ws), self._ws.numel(), stream())
        self.offered += L
        return self

    def result(self):
        """``(scores [queries, k] float32, ids [queries, k] int32, counts [queries] int64)`` on the device, every list sorted best
        first; the slots past ``counts[j]`` hold NaN and -1.  The first two are the live state (clone them to keep them across
        an ``update``)."""
        return self.scores, self.ids, (self.ids >= 0).sum(1)
