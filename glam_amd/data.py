"""Graph containers, PyG-style collation and synthetic ESOL / protein-shaped graphs.

The reference builds its inputs with RDKit + ``torch_geometric.data`` (neither is
available), so the path's *input layout* is restated here:

* ``Data`` / ``Batch.from_data_list`` follow PyG collation semantics as used by the
  reference ``DataLoader`` (``src_1gp/trainer.py:37-41``): concatenate ``x`` /
  ``edge_attr`` / ``y``, offset ``edge_index`` by the cumulative node count, and emit a
  non-decreasing ``batch`` vector.
* ``synth_molecule`` emits the tensor layout of ``get_mol_nodes_edges``
  (``src_1gp/dataset.py:60-97``): ``x[n,15]`` = one-hot(9) atom type | one-hot(3)
  hybridisation | atomic number, aromatic flag, #H ; ``edge_index`` int64 ``[2,E]`` with
  both directions of every bond, sorted by ``src*n+dst`` (``dataset.py:84-86``);
  ``edge_attr[E,4]`` one-hot bond type.  Sizes follow SURVEY.md §8d: atoms/mol ~
  U{12..28}, chain + ring-closure bonds => E/N ~ 2.05, in-degree 1..4.
* ``synth_protein`` emits the layout of the contact-map graphs of
  ``src_2gi_dti_scr/dataset.py:67-103``: ``x[n,49]``, chain edges then symmetric random
  contacts (unsorted, may hold duplicates), ``edge_attr[E,8]`` continuous.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

_ATOMIC_NUMBERS = np.array([1, 6, 7, 8, 9, 16, 17, 35, 53], dtype=np.float32)


def _carry_marks(src, dst):
    """Copy the host-side validation marks of ``src`` onto its device copy ``dst`` — only the marks that are still valid
    for ``src`` (made at its current version counter): a tensor written in place after validation, or a different tensor
    assigned to the field, carries nothing over and is validated on the device like any foreign tensor."""
    if dst is src:
        return
    if getattr(src, "_glam_trusted", None) == src._version:
        dst._glam_trusted = dst._version
    oh = getattr(src, "_glam_onehot", None)
    if oh is not None and oh[1] == src._version:
        dst._glam_onehot = (oh[0], dst._version)


class Data:
    """Minimal attribute bag with the fields the reference model reads
    (``model.py:47-57``: ``x, edge_index, edge_attr, batch``) plus ``y``."""

    def __init__(self, x=None, edge_index=None, edge_attr=None, y=None, batch=None, **kw):
        self.x, self.edge_index, self.edge_attr, self.y, self.batch = x, edge_index, edge_attr, y, batch
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def num_nodes(self):
        return 0 if self.x is None else self.x.size(0)

    @property
    def num_edges(self):
        return 0 if self.edge_index is None else self.edge_index.size(1)

    def _tensor_items(self):
        return [(k, v) for k, v in self.__dict__.items() if torch.is_tensor(v)]

    def to(self, device, non_blocking=False):
        out = self.__class__.__new__(self.__class__)
        out.__dict__.update(self.__dict__)
        for k, v in self._tensor_items():
            moved = v.to(device, non_blocking=non_blocking)
            _carry_marks(v, moved)
            setattr(out, k, moved)
        # device-side staging caches (CSR) are per-object and per-device
        out.__dict__.pop("_glam_cache", None)
        return out

    def _apply_marks(self):
        """Validation facts established on the host (PackedDataset.collate, on the tensors it has just built) ride on the
        tensors so that the device-side staging needs no read-back: ``edge_index`` / ``batch`` ids valid by construction,
        ``edge_attr`` rows one-hot or not.  Called once, by the collation that built the tensors; ``to()`` never re-derives a
        mark from the field name — it copies the mark of the very tensor it moves, and only while that mark is still valid."""
        for field, (attr, value) in self.__dict__.pop("_glam_marks", {}).items():
            t = getattr(self, field, None)
            if torch.is_tensor(t):      # tied to the tensor's version counter: an in-place write voids the mark
                setattr(t, attr, t._version if attr == "_glam_trusted" else (value, t._version))

    def __repr__(self):
        body = ", ".join(f"{k}={list(v.shape)}" for k, v in self._tensor_items())
        return f"{self.__class__.__name__}({body})"


class Batch(Data):
    """Disjoint union of graphs (PyG ``Batch.from_data_list`` semantics)."""

    num_graphs = 0

    @classmethod
    def from_data_list(cls, data_list):
        """PyG ``Batch.from_data_list`` semantics: concatenate ``x`` / ``edge_attr`` / ``y``, offset ``edge_index`` by the
        running node count, build ``batch``.  Vectorised: one ``repeat_interleave`` each for the offsets and the batch vector
        (a Python loop of per-graph tensor ops cost 40 ms per 1 024 molecules, 40x the device step)."""
        B = len(data_list)
        ns = torch.tensor([d.x.size(0) for d in data_list], dtype=torch.long)
        es = torch.tensor([d.edge_index.size(1) for d in data_list], dtype=torch.long)
        node_off = ns.cumsum(0) - ns
        ei = torch.cat([d.edge_index for d in data_list], 1) if B else torch.zeros(2, 0, dtype=torch.long)
        ei = ei + torch.repeat_interleave(node_off, es, output_size=int(ei.size(1))).unsqueeze(0)
        eas = [d.edge_attr for d in data_list if d.edge_attr is not None]
        ys = [d.y for d in data_list if d.y is not None]
        n_total = int(ns.sum()) if B else 0
        out = cls(x=torch.cat([d.x for d in data_list], 0), edge_index=ei,
                  edge_attr=torch.cat(eas, 0) if eas else None, y=torch.cat(ys, 0) if ys else None,
                  batch=torch.repeat_interleave(torch.arange(B), ns, output_size=n_total))
        out.num_graphs = B
        out.ptr = torch.cat([ns.new_zeros(1), ns.cumsum(0)])
        return out


class _few_threads:
    """Host-side collation is dozens of tiny tensor ops: with torch's default of one intra-op thread per core they spend
    their time waking a 100+ thread pool (6 ms instead of 0.2 ms per 32-molecule batch on a 128-core host).  Same remedy
    as ``torch.utils.data`` workers: a small thread count while collating, restored afterwards."""

    def __init__(self, n=4):
        self.n = n

    def __enter__(self):
        self.prev = torch.get_num_threads()
        if self.prev > self.n:
            torch.set_num_threads(self.n)

    def __exit__(self, *exc):
        if torch.get_num_threads() != self.prev:
            torch.set_num_threads(self.prev)
        return False


class PackedDataset:
    """All graphs of a dataset in flat tensors (node / edge prefix sums), so that collating ANY set of graph ids is a
    handful of vectorised gathers instead of ``len(ids)`` small concatenations (with the device step
    at ~1 ms for 1 024 molecules, host collation is what caps a shuffling loader)."""

    def __init__(self, data_list):
        data_list = list(data_list)
        self.n = len(data_list)
        ns = torch.tensor([d.x.size(0) for d in data_list], dtype=torch.long)
        es = torch.tensor([d.edge_index.size(1) for d in data_list], dtype=torch.long)
        self.ns, self.es = ns, es
        self.node_ptr = torch.cat([ns.new_zeros(1), ns.cumsum(0)])
        self.edge_ptr = torch.cat([es.new_zeros(1), es.cumsum(0)])
        self.x = torch.cat([d.x for d in data_list], 0)
        self.ei = torch.cat([d.edge_index for d in data_list], 1)            # graph-local node ids
        has_ea = [d.edge_attr is not None for d in data_list]
        has_y = [d.y is not None for d in data_list]
        if any(has_ea) != all(has_ea) or any(has_y) != all(has_y):
            raise ValueError("PackedDataset: edge_attr / y must be present for all graphs or for none")
        self.ea = torch.cat([d.edge_attr for d in data_list], 0) if all(has_ea) and data_list else None
        self.y = torch.cat([d.y for d in data_list], 0) if all(has_y) and data_list else None
        self.y_rows = None if self.y is None else torch.tensor([d.y.size(0) for d in data_list], dtype=torch.long)
        # host-side validation, once: what the device-side staging would otherwise read back for every new batch
        loc_n = torch.repeat_interleave(ns, es, output_size=int(self.ei.size(1)))
        self.valid_ids = bool(((self.ei >= 0) & (self.ei < loc_n.unsqueeze(0))).all()) if self.ei.numel() else True
        self.onehot = None if self.ea is None else \
            (bool((((self.ea == 0) | (self.ea == 1)).all() & (self.ea.sum(dim=1) == 1).all())) if self.ea.numel() else True)
        if self.y_rows is not None and not bool((self.y_rows == 1).all()):
            self.y_ptr = torch.cat([self.y_rows.new_zeros(1), self.y_rows.cumsum(0)])
        else:
            self.y_ptr = None

    @staticmethod
    def _ranges(starts, lens, total):
        """Concatenation of ``arange(s, s + l)`` for every (s, l): one repeat_interleave + one arange."""
        off = lens.cumsum(0) - lens
        return torch.repeat_interleave(starts - off, lens, output_size=total) + torch.arange(total)

    def collate(self, ids):
        ids = torch.as_tensor(ids, dtype=torch.long)
        B = int(ids.numel())
        ns, es = self.ns[ids], self.es[ids]
        n_total, e_total = int(ns.sum()), int(es.sum())
        nodes = self._ranges(self.node_ptr[ids], ns, n_total)
        edges = self._ranges(self.edge_ptr[ids], es, e_total)
        node_off = ns.cumsum(0) - ns
        ei = self.ei[:, edges] + torch.repeat_interleave(node_off, es, output_size=e_total).unsqueeze(0)
        if self.y is None:
            y = None
        elif self.y_ptr is None:
            y = self.y[ids]
        else:
            y = self.y[self._ranges(self.y_ptr[ids], self.y_rows[ids], int(self.y_rows[ids].sum()))]
        out = Batch(x=self.x[nodes], edge_index=ei, edge_attr=None if self.ea is None else self.ea[edges], y=y,
                    batch=torch.repeat_interleave(torch.arange(B), ns, output_size=n_total))
        out.num_graphs = B
        out.ptr = torch.cat([ns.new_zeros(1), ns.cumsum(0)])
        out._glam_marks = {"edge_index": ("_glam_trusted", True), "batch": ("_glam_trusted", True)} if self.valid_ids else {}
        if self.onehot is not None:
            out._glam_marks["edge_attr"] = ("_glam_onehot", self.onehot)
        out._apply_marks()
        return out


def resident_table(ids, ns, es, y_rows):
    """The slot table of ``DeviceDataset.collate`` (host, O(B) numpy): ``(table, N, E, Y)`` with ``table`` int32 ``[4, B + 1]`` — row 0 the
    graph ids (one entry of padding), rows 1-3 the exclusive offsets of the slots' nodes, edges and ``y`` rows, each closed by its
    total.  ``ns`` / ``es`` / ``y_rows``: per-graph counts of the dataset.  ``IndexError`` for an id outside ``[0, len(ns))`` — before
    anything is launched; the kernel trusts the table."""
    ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).reshape(-1)
    if ids.size == 0:
        ids = np.zeros(0, dtype=np.int64)
    if ids.dtype.kind not in "iu":
        raise IndexError(f"graph ids must be integers, got {ids.dtype}")
    ids = ids.astype(np.int64)
    n, B = int(ns.shape[0]), int(ids.size)
    if B and (int(ids.min()) < 0 or int(ids.max()) >= n):
        raise IndexError(f"graph ids must lie in [0, {n}): got {int(ids.min())} .. {int(ids.max())}")
    table = np.zeros((4, B + 1), dtype=np.int64)
    table[0, :B] = ids
    for row, counts in zip(table[1:], (ns, es, y_rows)):
        np.cumsum(counts[ids], out=row[1:])
    if B and int(table[1:, B].max()) >= 2 ** 31 - 1:
        from ._lib import GlamHipError
        raise GlamHipError("DeviceDataset.collate: the batch's node / edge / y rows do not fit int32")
    return table.astype(np.int32), int(table[1, B]), int(table[2, B]), int(table[3, B])


def _phantom_rows(phantom_rows):
    m = int(phantom_rows)
    if m != phantom_rows or m < 1:
        raise ValueError(f"phantom_rows bounds the nodes of a phantom graph: an integer >= 1 or None, got {phantom_rows!r}")
    return m


def _top(v, B):
    return int(np.partition(v, v.size - B)[v.size - B:].sum())


def _bottom(v, B):
    return int(np.partition(v, B - 1)[:B].sum())


def phantom_graphs(ns, batch_size, n_cap, phantom_rows):
    """``K``, the number of phantom graphs of a bucket of ``n_cap`` nodes: 1 for ``phantom_rows = None`` (the single phantom graph), else the
    fewest graphs of at most ``phantom_rows`` nodes that hold the largest surplus any ``batch_size`` distinct graphs leave,
    ``ceil((n_cap - botB(ns)) / phantom_rows)`` with ``botB`` = the sum of the ``batch_size`` smallest entries."""
    if phantom_rows is None:
        return 1
    ns = np.asarray(ns, dtype=np.int64)
    return max(1, -(-(int(n_cap) - _bottom(ns, int(batch_size))) // _phantom_rows(phantom_rows)))


def padded_capacity(ns, es, batch_size, ell, phantom_rows=None):
    """``(N_cap, E_cap)`` of a fixed-capacity batch (``DeviceDataset.padded``) that holds ANY ``batch_size`` distinct graphs of a dataset
    with per-graph node / edge counts ``ns`` / ``es`` (host numpy).  ``topB(v)`` = the sum of the ``batch_size`` largest entries of ``v``:
    ``E_cap = topB(es)``, ``N_cap = topB(ns) + 1`` — one phantom node at least.  ``ell``: the batch carries an ELL form (in- or out-degree
    <= 4 per node), which the phantom nodes must keep: ``N_cap >= ceil((E_cap + topB(4 ns - es)) / 4)`` gives, for every such set S,
    ``4 (N_cap - N(S)) - (E_cap - E(S)) = 4 N_cap - E_cap - sum_S (4 n - e) >= 4 N_cap - E_cap - topB(4 ns - es) >= 0``.

    ``phantom_rows = m``: the surplus ``P = N_cap - N(S)`` is cut into ``K`` phantom graphs of ``1 .. m`` nodes each, so ``K <= P <= K m`` for
    every S: ``N_cap = max(topB(ns) + K, the ELL term)`` gives ``P >= N_cap - topB(ns) >= K``, and ``K`` is the smallest integer with
    ``K m >= N_cap - botB(ns) >= P`` — found by iterating ``K <- ceil((N_cap(K) - botB(ns)) / m)`` from 1, which climbs to the least fixed
    point.  ``phantom_graphs(ns, batch_size, N_cap, m)`` gives that ``K`` back.  ``ValueError`` for ``m = 1`` over graphs of unequal sizes
    (``K >= topB - botB + K`` has no solution)."""
    ns, es = np.asarray(ns, dtype=np.int64), np.asarray(es, dtype=np.int64)
    B = int(batch_size)
    if not 1 <= B <= ns.size:
        raise ValueError(f"padded batches hold 1 .. {ns.size} distinct graphs of this dataset, got batch_size = {batch_size}")
    e_cap, n_top = _top(es, B), _top(ns, B)
    n_ell = -(-(e_cap + _top(4 * ns - es, B)) // 4) if ell else 0
    if phantom_rows is None:
        return max(n_top + 1, n_ell), e_cap
    m = _phantom_rows(phantom_rows)
    if m == 1 and n_top != _bottom(ns, B):
        raise ValueError(f"phantom_rows = 1 gives every surplus node a graph of its own, which one fixed count of phantom graphs can do "
                         f"only where every {B} graphs have the same node count; here it ranges over {_bottom(ns, B)} .. {n_top}")
    K = 1
    while True:
        n_cap = max(n_top + K, n_ell)
        need = phantom_graphs(ns, B, n_cap, m)
        if need <= K:
            return n_cap, e_cap
        K = need


def padded_bucket(ns, es, y_rows, batch_size, capacity, ell, phantom_rows=None, labels=True):
    """The checked ``(N_cap, E_cap, r)`` of ``DeviceDataset.padded``: ``capacity`` (or ``padded_capacity``) and the one constant count of
    ``y`` rows per graph.  ``ValueError`` for ``y`` rows that differ between graphs or are absent, and for a capacity that the dataset's
    largest graph does not fit with one phantom node beside it — with ``phantom_rows``, one node for each of the
    ``phantom_graphs(ns, batch_size, N_cap, phantom_rows)`` phantom graphs.  ``labels=False``: the graphs carry no ``y`` (the ligand side
    of a resident pair batch, whose labels belong to the pairs): ``r = 0``."""
    y_rows = np.asarray(y_rows, dtype=np.int64)
    r = int(y_rows[0]) if y_rows.size and labels else 0
    if labels and (r < 1 or bool((y_rows != r).any())):
        raise ValueError("padded batches need the same number (>= 1) of y rows for every graph: the loss reads output[:B] against y[B * r]")
    n_cap, e_cap = padded_capacity(ns, es, batch_size, ell, phantom_rows) if capacity is None else (int(capacity[0]), int(capacity[1]))
    if phantom_rows is not None and not 1 <= int(batch_size) <= np.size(ns):
        raise ValueError(f"padded batches hold 1 .. {np.size(ns)} distinct graphs of this dataset, got batch_size = {batch_size}")
    K = phantom_graphs(ns, batch_size, n_cap, phantom_rows)
    if n_cap - K < int(np.max(ns)) or e_cap < int(np.max(es)) or max(n_cap, e_cap) >= 2 ** 31 - 1:
        raise ValueError(f"capacity ({n_cap}, {e_cap}) does not hold the dataset's largest graph ({int(np.max(ns))} nodes + "
                         f"{'1 phantom node' if K == 1 else f'{K} phantom nodes, one per phantom graph'}, {int(np.max(es))} edges) or exceeds int32")
    return n_cap, e_cap, r


def padded_fit(batch_size, B, N, E, n_cap, e_cap, ell, phantoms=1, phantom_rows=None):
    """``ValueError`` unless a table of ``B`` slots with ``N`` nodes and ``E`` edges fits the bucket ``(batch_size, n_cap, e_cap)``: one
    phantom node at least, and phantom degrees <= 4 where the batch carries an ELL form.  Distinct ids always fit the capacity of
    ``padded_capacity``; repeated ids may not.  With ``phantoms = K`` graphs of at most ``phantom_rows`` nodes the surplus must satisfy
    ``K <= n_cap - N <= K * phantom_rows``: no phantom graph empty, none above the bound."""
    if B != batch_size:
        raise ValueError(f"this padded batch holds exactly {batch_size} graphs, got {B} ids")
    if N > n_cap - phantoms or E > e_cap:
        raise ValueError(f"{N} nodes / {E} edges exceed the capacity ({n_cap} nodes, {'one' if phantoms == 1 else phantoms} of them phantom, "
                         f"{e_cap} edges): repeated ids?")
    if phantom_rows is not None and n_cap - N > phantoms * phantom_rows:
        raise ValueError(f"{n_cap - N} surplus nodes exceed the {phantoms} phantom graphs of {phantom_rows} nodes of this bucket: repeated ids?")
    if ell and 4 * (n_cap - N) < e_cap - E:
        raise ValueError(f"{e_cap - E} surplus edges on {n_cap - N} phantom nodes exceed degree 4 (the ELL form): repeated ids?")


class DeviceDataset:
    """A dataset that LIVES ON THE DEVICE, graph index included, so that collating any set of graph ids is one kernel launch
    (``glam_collate``, csrc/collate.hip) behind one small host-to-device copy — no per-field copies, no CSR / ELL builds, no read-back.

    A batch is a disjoint union of graphs: its CSR by target and by source and its ELL records are the per-graph ones with two offsets
    added.  So they are built ONCE, at construction, for the dataset taken as one big disjoint graph (``glam_csr_build`` both ways,
    ``glam_ell_build`` on each; the two degree flags are read back here and never again), and a batch is a segmented copy.

    On the device: the flat ``x``, graph-local ``ei`` (int32), ``ea``, ``y``; the node / edge / y prefix sums; both CSRs; both ELL pairs
    (where no degree exceeds 4).  On the host: ``ns`` / ``es`` / ``y_rows`` (numpy), ``valid_ids`` / ``onehot`` as ``PackedDataset``
    checks them, ``ell_ok`` / ``ell_t_ok``."""

    def __init__(self, data, device):
        from . import ops
        packed = data if isinstance(data, PackedDataset) else PackedDataset(data)
        self.device = device = torch.device(device)
        if device.type != "cuda":
            raise ops.GlamHipError(f"DeviceDataset lives on an MI355X HIP device (got {device}); the host path is PackedDataset")
        self.n = packed.n
        self.ns, self.es = packed.ns.numpy().copy(), packed.es.numpy().copy()
        self.y_rows = np.zeros(self.n, dtype=np.int64) if packed.y is None else packed.y_rows.numpy().copy()
        self.valid_ids, self.onehot = packed.valid_ids, packed.onehot
        if not self.valid_ids:      # (the dataset-wide index is the per-graph ones side by side only if no edge leaves its graph)
            raise IndexError("DeviceDataset: an edge_index holds node ids outside its own graph")
        Nd, Ed, Yd = int(self.ns.sum()), int(self.es.sum()), int(self.y_rows.sum())
        if max(Nd, Ed, Yd) >= 2 ** 31 - 1:
            raise ops.GlamHipError(f"DeviceDataset: {Nd} nodes / {Ed} edges / {Yd} y rows do not fit int32")
        self._row_bytes = []
        for name, t in (("x", packed.x), ("edge_attr", packed.ea), ("y", packed.y)):
            rb = 0 if t is None else int(np.prod(t.shape[1:], dtype=np.int64)) * t.element_size()
            if rb % 4:
                raise ops.GlamHipError(f"DeviceDataset: rows of {name} ({t.dtype} {tuple(t.shape[1:])}) are no multiple of 4 bytes")
            self._row_bytes.append(rb)
        i32 = lambda t: t.to(torch.int32).contiguous().to(device)       # noqa: E731
        self.x = packed.x.contiguous().to(device)
        self.ei = i32(packed.ei)
        self.ea = None if packed.ea is None else packed.ea.contiguous().to(device)
        self.y = None if packed.y is None else packed.y.contiguous().to(device)
        self.node_ptr, self.edge_ptr = i32(packed.node_ptr), i32(packed.edge_ptr)
        self.y_ptr = i32(torch.from_numpy(np.concatenate([[0], np.cumsum(self.y_rows)])))
        # the dataset as ONE disjoint graph, through the builds every batch's index went through so far
        ei_all = (packed.ei + torch.repeat_interleave(packed.node_ptr[:-1], packed.es, output_size=Ed).unsqueeze(0)).to(device)
        gi = ops.GraphIndex(ei_all, Nd, validate=False)
        self.rowptr, self.src, self.eid = gi.rowptr, gi.src, gi.eid
        self.colptr, self.dst, self.eid_t = gi.transpose()
        self.ell, self.ell_t = gi.ell(), gi.ell_t()             # (the one read-back of each degree flag)
        self.ell_ok, self.ell_t_ok = self.ell is not None, self.ell_t is not None
        fields = [self.x, self.ei, self.ea, self.y, self.node_ptr, self.edge_ptr, self.y_ptr, self.rowptr, self.src, self.eid,
                  self.colptr, self.dst, self.eid_t, *(self.ell or (None, None)), *(self.ell_t or (None, None))]
        self._ds = (ctypes.c_void_p * len(fields))(*[None if t is None else t.data_ptr() for t in fields])

    def __len__(self):
        return self.n

    def collate(self, ids):
        """The batch of the graphs ``ids`` (any host sequence, repeats allowed), field by field what
        ``PackedDataset.collate(ids).to(device)`` gives, with its ``GraphIndex`` and ``SegmentPtr`` already installed in the caches of
        ``ops.graph_index`` / ``ops.segment_ptr``: the model's first step on it builds nothing and reads nothing back."""
        from . import _lib, ops
        table, N, E, Y = resident_table(ids, self.ns, self.es, self.y_rows)
        B = table.shape[1] - 1
        dev = self.device
        _lib.require_device(self.x)
        # the one host-to-device copy of a batch, out of pinned memory so that it is only enqueued: the host does not wait for the step
        # before (torch's host allocator hands the block out again once the copy has run)
        staged = torch.empty(table.shape, dtype=torch.int32, pin_memory=True)
        staged.numpy()[...] = table
        tab = staged.to(dev, non_blocking=True)
        new = lambda t, rows: None if t is None else torch.empty((rows,) + t.shape[1:], dtype=t.dtype, device=dev)   # noqa: E731
        x, ea, y = new(self.x, N), new(self.ea, E), new(self.y, Y)
        ei = torch.empty(2, E, dtype=torch.int64, device=dev)
        batch, ptr = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(B + 1, dtype=torch.int64, device=dev)
        # the index tensors out of one allocation, every one on a 16-byte boundary
        ell, ell_t = self.ell_ok and N > 0, self.ell_t_ok and N > 0
        sizes = [B + 1, N + 1, E, E, N + 1, E, E] + [4 * N if ell else 0] * 2 + [4 * N if ell_t else 0] * 2
        starts = np.concatenate([[0], np.cumsum([(s + 3) & ~3 for s in sizes])])
        arena = torch.empty(int(starts[-1]), dtype=torch.int32, device=dev)
        ptr32, rowptr, src, eid, colptr, dst, eid_t, *ells = [arena[a:a + s] for a, s in zip(starts[:-1].tolist(), sizes)]
        ells = [t.view(N, 4) if t.numel() else None for t in ells]
        out = [x, ei, ea, y, batch, ptr, ptr32, rowptr, src, eid, colptr, dst, eid_t, *ells]
        out = (ctypes.c_void_p * len(out))(*[None if t is None else t.data_ptr() for t in out])
        _lib.api().glam_collate(self._ds, out, _lib.ptr(tab), B, N, E, Y, int(self.ei.size(1)), *self._row_bytes, _lib.stream())
        gi = ops.GraphIndex.from_parts(ei, N, rowptr, src, eid, (colptr, dst, eid_t), tuple(ells[:2]) if ell else None,
                                       tuple(ells[2:]) if ell_t else None)
        ops._GI_CACHE.put(ei, (N, gi))
        ops._SP_CACHE.put(batch, ops.SegmentPtr.from_parts(ptr32, N, B))
        b = Batch(x=x, edge_index=ei, edge_attr=ea, y=y, batch=batch)
        b.num_graphs, b.ptr = B, ptr
        b._glam_marks = {"edge_index": ("_glam_trusted", True), "batch": ("_glam_trusted", True)}
        if self.onehot is not None:
            b._glam_marks["edge_attr"] = ("_glam_onehot", self.onehot)
        b._apply_marks()
        return b


    def capacity(self, batch_size, phantom_rows=None):
        """``(N_cap, E_cap)`` that hold any ``batch_size`` distinct graphs of this dataset (``padded_capacity``; pure host numpy)."""
        return padded_capacity(self.ns, self.es, batch_size, self.ell_ok or self.ell_t_ok, phantom_rows)

    def padded(self, batch_size, capacity=None, phantom_rows=None):
        """A ``PaddedBatch`` of ``batch_size`` graphs: every tensor allocated once, filled by ``load(ids)``.  ``phantom_rows = m``: the
        surplus rows go to several phantom graphs of at most ``m`` nodes (``int(ds.ns.max())`` keeps them no larger than a real graph),
        not to one that grows with the batch."""
        return PaddedBatch(self, batch_size, capacity, phantom_rows)


class PaddedBatch(Batch):
    """A batch of FIXED CAPACITY over a ``DeviceDataset``: the same tensors, at the same addresses and of the same shapes, hold whatever
    ``load(ids)`` puts into them (``glam_collate_padded``, csrc/collate.hip), so a training step captured on this object replays for
    every batch of a shuffling loop (``glam_amd.graphs.GraphedTrainStep``).

    It is an ordinary, valid batch of ``num_graphs = B + 1`` graphs: the ``num_real_graphs = B`` loaded ones first, then one PHANTOM
    graph that owns the surplus ``N_cap - N`` nodes (zero ``x`` rows) and ``E_cap - E`` edges (self-loops, copies of the dataset's edge
    row 0).  No kernel knows about it; a model that treats graphs independently gives the real graphs their usual rows, and a loss over
    ``output[:B]`` (``graphs.padded_loss``) gives the phantom rows a zero gradient.  ``y`` has the real graphs' ``B * r`` rows only.
    ``x`` is the ``[N_cap, F]`` view of a buffer whose rows are zero-padded to 16 bytes: ``ops.pad_cols`` hands the kernels the buffer
    itself (a cached padded COPY would go stale with the second ``load``: a kernel write does not bump ``_version``).

    ``phantom_rows = m``: the surplus nodes are cut into ``num_phantom_graphs = K`` phantom graphs of ``1 .. m`` nodes
    each (``glam_collate_padded_split``), ``K`` fixed for the bucket, so ``num_graphs = B + K`` and the model's output has ``B + K`` rows.
    The kernels that give a graph to one wave or block then never meet a graph larger than ``m``.  ``None``: one phantom graph."""

    def __init__(self, dataset, batch_size, capacity=None, phantom_rows=None, labels=True):
        from . import ops
        ds, B = dataset, int(batch_size)
        self.ell, self.ell_t = ds.ell_ok, ds.ell_t_ok
        has_y = ds.y is not None
        if not labels and has_y:
            raise ValueError("labels=False is the padded batch of graphs WITHOUT y (the ligands of a resident pair batch); this dataset has y")
        N_cap, E_cap, r = padded_bucket(ds.ns, ds.es, ds.y_rows if has_y else np.zeros(0), B, capacity, self.ell or self.ell_t, phantom_rows,
                                        labels)
        K = phantom_graphs(ds.ns, B, N_cap, phantom_rows)
        self.num_phantom_graphs, self.phantom_rows = K, None if phantom_rows is None else int(phantom_rows)
        dev = ds.device
        xrb, earb, yrb = ds._row_bytes
        stride = (xrb + 15) & ~15
        if stride != xrb and ds.x.dim() != 2:
            raise ValueError(f"padded batches pad the rows of a 2-D x to 16 bytes; x is {tuple(ds.x.shape)}")
        xbuf = torch.empty((N_cap, stride // ds.x.element_size()) if stride != xrb else (N_cap,) + ds.x.shape[1:], dtype=ds.x.dtype, device=dev)
        x = ops.slice_cols(xbuf, ds.x.size(1)) if stride != xrb else xbuf
        new = lambda t, rows: None if t is None else torch.empty((rows,) + t.shape[1:], dtype=t.dtype, device=dev)   # noqa: E731
        ea, y = new(ds.ea, E_cap), new(ds.y, B * r)
        ei = torch.empty(2, E_cap, dtype=torch.int64, device=dev)
        batch, ptr = torch.empty(N_cap, dtype=torch.int64, device=dev), torch.empty(B + K + 1, dtype=torch.int64, device=dev)
        sizes = [B + K + 1, N_cap + 1, E_cap, E_cap, N_cap + 1, E_cap, E_cap] + [4 * N_cap if self.ell else 0] * 2 + [4 * N_cap if self.ell_t else 0] * 2
        starts = np.concatenate([[0], np.cumsum([(s + 3) & ~3 for s in sizes])])
        arena = torch.empty(int(starts[-1]), dtype=torch.int32, device=dev)
        ptr32, rowptr, src, eid, colptr, dst, eid_t, *ells = [arena[a:a + s] for a, s in zip(starts[:-1].tolist(), sizes)]
        ells = [t.view(N_cap, 4) if t.numel() else None for t in ells]
        out = [xbuf, ei, ea, y, batch, ptr, ptr32, rowptr, src, eid, colptr, dst, eid_t, *ells]
        self._out = (ctypes.c_void_p * len(out))(*[None if t is None else t.data_ptr() for t in out])
        self._keep = (xbuf, arena)
        self._launch_args = (B, N_cap, E_cap, r, int(ds.ei.size(1)), xrb, stride, earb, yrb)
        self._ds, self._table = ds, torch.zeros(4, B + 1, dtype=torch.int32, device=dev)
        self._tables = self.totals = None
        self._launched = False
        super().__init__(x=x, edge_index=ei, edge_attr=ea, y=y, batch=batch)
        self.num_graphs, self.num_real_graphs, self.ptr = B + K, B, ptr
        self.capacity = (N_cap, E_cap)
        gi = ops.GraphIndex.from_parts(ei, N_cap, rowptr, src, eid, (colptr, dst, eid_t), tuple(ells[:2]) if self.ell else None,
                                       tuple(ells[2:]) if self.ell_t else None)
        ops._GI_CACHE.put(ei, (N_cap, gi))
        ops._SP_CACHE.put(batch, ops.SegmentPtr.from_parts(ptr32, N_cap, B + K))
        self._glam_marks = {"edge_index": ("_glam_trusted", True), "batch": ("_glam_trusted", True)}
        if ds.onehot is not None:
            self._glam_marks["edge_attr"] = ("_glam_onehot", ds.onehot)
        self._apply_marks()

    def _tensor_items(self):
        return [(k, v) for k, v in super()._tensor_items() if not k.startswith("_")]

    def to(self, device, non_blocking=False):
        if torch.device(device) != self._ds.device:
            raise ValueError("a PaddedBatch lives on its dataset's device")
        return self

    def _fit(self, B, N, E):
        padded_fit(self.num_real_graphs, B, N, E, *self.capacity, self.ell or self.ell_t, self.num_phantom_graphs, self.phantom_rows)

    def load(self, ids=None, step=None, launch=True):
        """Put the graphs ``ids`` (exactly ``B`` of them) into this batch: the slot table goes to the device out of pinned memory, not
        waited for, and one launch writes every field and the whole index.  ``step=i`` instead of ``ids``: table ``i`` of the last
        ``load_many``, a device-to-device copy.  ``launch=False`` uploads the table only — for a batch that a ``GraphedTrainStep`` runs
        next, whose step (eager, captured or replayed) holds the launch itself.  ``IndexError`` for ids outside the dataset, ``ValueError``
        for a wrong count or ids (repeated ones) that exceed the capacity — before anything is enqueued."""
        from . import _lib
        if (ids is None) == (step is None):
            raise ValueError("PaddedBatch.load takes either ids or step=")
        if step is not None:
            if self._tables is None or not 0 <= int(step) < self._tables.size(0):
                raise IndexError(f"step {step}: load_many has uploaded {0 if self._tables is None else self._tables.size(0)} tables")
            self._table.copy_(self._tables[int(step)])
        else:
            table, N, E, _Y = resident_table(ids, self._ds.ns, self._ds.es, self._ds.y_rows)
            self._fit(table.shape[1] - 1, N, E)
            _lib.require_device(self.edge_index)
            staged = torch.empty(table.shape, dtype=torch.int32, pin_memory=True)
            staged.numpy()[...] = table
            self._table.copy_(staged, non_blocking=True)
        self._launched = False
        if launch:
            self.glam_reload()
            self._launched = True
        return self

    def load_many(self, id_lists):
        """The tables of ``len(id_lists)`` batches (an epoch's) from one numpy pass and ONE upload; ``load(step=i)`` then installs table
        ``i``.  Same errors as ``load``, for every list, before anything is enqueued.  Returns the number of tables."""
        ds = self._ds
        B = self.num_real_graphs
        rows = [np.asarray(i.cpu() if torch.is_tensor(i) else i).reshape(-1) for i in id_lists]
        if any(r.size != B for r in rows):
            raise ValueError(f"this padded batch holds exactly {B} graphs, got id lists of {sorted({int(r.size) for r in rows})}")
        ids = np.stack(rows) if rows else np.zeros((0, B), dtype=np.int64)
        if ids.dtype.kind not in "iu":
            raise IndexError(f"graph ids must be integers, got {ids.dtype}")
        ids = ids.astype(np.int64)
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= ds.n):
            raise IndexError(f"graph ids must lie in [0, {ds.n}): got {int(ids.min())} .. {int(ids.max())}")
        tables = np.zeros((ids.shape[0], 4, B + 1), dtype=np.int64)
        tables[:, 0, :B] = ids
        for k, counts in enumerate((ds.ns, ds.es, ds.y_rows), 1):
            np.cumsum(counts[ids], axis=1, out=tables[:, k, 1:])
        for N, E in zip(tables[:, 1, B].tolist(), tables[:, 2, B].tolist()):
            self._fit(B, N, E)
        staged = torch.empty(tables.shape, dtype=torch.int32, pin_memory=True)
        staged.numpy()[...] = tables
        self._tables = staged.to(ds.device, non_blocking=True)
        self.totals = tables[:, 1:3, B].copy()       # (N, E) per table: what the padding overhead is measured against
        return int(ids.shape[0])

    def glam_reload(self):
        """The reload hook of ``GraphedTrainStep``: enqueue the collate launch for the table now on the device — on the current
        stream, so inside a capture it becomes the graph's first node.  Outside a capture a ``load`` that has launched already is not
        repeated."""
        from . import _lib
        if self._launched and not torch.cuda.is_current_stream_capturing():
            self._launched = False
            return
        B, N_cap, E_cap, r, Ed, xrb, stride, earb, yrb = self._launch_args
        if self.phantom_rows is None:
            _lib.api().glam_collate_padded(self._ds._ds, self._out, _lib.ptr(self._table), B, N_cap, E_cap, r, Ed, xrb, stride, earb, yrb,
                                           _lib.stream())
        else:
            _lib.api().glam_collate_padded_split(self._ds._ds, self._out, _lib.ptr(self._table), B, self.num_phantom_graphs, N_cap, E_cap, r, Ed,
                                                 xrb, stride, earb, yrb, _lib.stream())


# --------------------------------------------------------------------------------------
# resident pair data: a dataset's pair table on the device, and batches of fixed capacity that one launch refills
# --------------------------------------------------------------------------------------
def pair_ids_table(ids, n_pairs, batch_size):
    """The checked pair ids of one load of a resident pair batch (host, numpy) -> int32 ``[batch_size]``.  ``ops.host_ints``'s refusals —
    a device tensor (``GlamHipError``), a non-integer dtype, another shape than a vector, an id outside ``[0, n_pairs)`` (``IndexError``) —
    then ``ValueError`` for another count than ``batch_size``: before anything is enqueued; the kernel trusts the table."""
    from . import ops
    a = ops.host_ints(ids, "pair ids", "be a vector of pair ids", below=int(n_pairs))
    if a.shape[0] != int(batch_size):
        raise ValueError(f"this pair batch holds exactly {int(batch_size)} pairs, got {a.shape[0]} ids (run a shorter last batch eagerly on a "
                         "host ops.pair_index, or drop it)")
    return a.astype(np.int32)


def dti_tables(pair_ids, first, ns, es, batch_size):
    """The host side of one DTI load (O(B) numpy) -> ``(table, N, E)``: ``table`` int32 ``[4 * (B + 1) + B]`` — the ligand slot table of
    ``resident_table`` over the ligands ``first[pair_ids]`` (ids, then the exclusive node / edge / y offsets: no y rows), then the pair ids
    themselves — and the slots' node and edge totals for the capacity check.  Errors of ``pair_ids_table``."""
    ids = pair_ids_table(pair_ids, first.shape[0], batch_size)
    slots, N, E, _Y = resident_table(first[ids], ns, es, np.zeros(ns.shape[0], dtype=np.int64))
    return np.concatenate([slots.reshape(-1), ids]), N, E


def protein_slot_ids(second_of_pairs, ns, slots):
    """The protein side of one refill load (host, O(B log B) numpy) -> ``(slot_ids, keys, U)``: ``u`` = the sorted distinct entries of
    ``second_of_pairs`` (the proteins of the step's pairs), ``U = len(u)``; ``slot_ids`` int64 ``[slots]`` = ``u`` followed by ``slots - U``
    FILLER proteins, the smallest by ``(ns, id)`` that are not in ``u`` — exactly ``slots`` distinct graphs, the case ``padded_capacity``
    guarantees to fit; ``keys`` = ``searchsorted(u, second_of_pairs)``, the slot of every pair's protein.  ``ValueError`` for ``U > slots``
    (the caller runs that step eagerly on ``proteins.collate(u)`` with ``ops.pair_index``) — before anything is enqueued."""
    sec = np.asarray(second_of_pairs, dtype=np.int64)
    ns = np.asarray(ns, dtype=np.int64)
    u = np.unique(sec)
    U, Q = int(u.size), int(slots)
    if U > Q:
        raise ValueError(f"this step's pairs name {U} distinct proteins, the batch holds protein_slots = {Q}: run the step eagerly on "
                         f"proteins.collate(u) with ops.pair_index, or build the batch with more slots")
    # (among the Q smallest at most U are in u: Q - U fillers are always found there)
    smallest = np.lexsort((np.arange(ns.size), ns))[:Q]
    fill = smallest[~np.isin(smallest, u)][:Q - U]
    return np.concatenate([u, fill]).astype(np.int64), np.searchsorted(u, sec).astype(np.int32), U


def dti_refill_tables(pair_ids, first, second, lig_ns, lig_es, pro_ns, pro_es, batch_size, slots, phantoms):
    """The host side of one load of a ``ResidentDTIRefillBatch`` -> ``(table, (N, E), (Np, Ep))``: ``table`` int32 — the ligand slot table
    and the pair ids as ``dti_tables`` lays them out, then the protein slot table ``[4 * (slots + 1)]`` of ``resident_table`` over
    ``protein_slot_ids``' ids, then the ``batch_size + phantoms`` keys (the phantom ligand slots keep key 0) — and both sides' node / edge
    totals for the capacity checks.  Errors of ``pair_ids_table`` and ``protein_slot_ids``."""
    lig, N, E = dti_tables(pair_ids, first, lig_ns, lig_es, batch_size)
    ids = lig[-int(batch_size):]
    slot_ids, keys, _U = protein_slot_ids(second[ids], pro_ns, slots)
    pro, Np, Ep, _Y = resident_table(slot_ids, pro_ns, pro_es, np.zeros(pro_ns.shape[0], dtype=np.int64))
    return np.concatenate([lig, pro.reshape(-1), keys, np.zeros(int(phantoms), dtype=np.int32)]), (N, E), (Np, Ep)


def ddi_table(pair_ids, n_pairs, batch_size):
    """The host side of one DDI load: the checked pair ids, int32 ``[B]`` (``pair_ids_table``)."""
    return pair_ids_table(pair_ids, n_pairs, batch_size)


def _pair_column(v, name):
    from . import ops
    return ops.host_ints(v, name, "be a vector with one segment id per pair", below=2 ** 31 - 1).astype(np.int32)


class ResidentPairs:
    """A dataset's pair table ON THE DEVICE: two int32 columns ``first`` / ``second`` ``[Np]`` — a graph id per pair and side (DTI: ligand,
    protein; DDI: drug, drug) — and the labels ``y`` ``[Np, r]``.  Host copies of the columns (``first_host`` / ``second_host``, numpy) stay
    for the O(B) table arithmetic of a load.  Validated once, here: integer columns of equal length with entries >= 0 (``IndexError`` /
    ``ValueError``), one label row per pair whose bytes are a multiple of 4.  ``dti_batch`` / ``ddi_batch`` make the batch objects that one
    launch refills from it per step."""

    def __init__(self, first, second, y, device):
        from . import ops
        self.first_host, self.second_host = _pair_column(first, "first"), _pair_column(second, "second")
        self.n = int(self.first_host.shape[0])
        if self.second_host.shape[0] != self.n:
            raise ValueError(f"ResidentPairs: the two columns disagree: {self.n} first ids, {self.second_host.shape[0]} second ids")
        y = torch.as_tensor(y)
        if y.dim() == 1:
            y = y.unsqueeze(1)
        if y.size(0) != self.n:
            raise ValueError(f"ResidentPairs: {self.n} pairs but {y.size(0)} label rows")
        rb = int(np.prod(y.shape[1:], dtype=np.int64)) * y.element_size()
        if rb < 4 or rb % 4:
            raise ValueError(f"ResidentPairs: label rows ({y.dtype} {tuple(y.shape[1:])}) are no positive multiple of 4 bytes")
        self.device = device = torch.device(device)
        if device.type != "cuda":
            raise ops.GlamHipError(f"ResidentPairs lives on an MI355X HIP device (got {device}); the host path is ops.pair_index per step")
        both = torch.from_numpy(np.concatenate([self.first_host, self.second_host])).to(device)        # (one copy)
        self.first, self.second = both[:self.n], both[self.n:]
        self.y = y.contiguous().to(device)

    def __len__(self):
        return self.n

    def dti_batch(self, ligands, proteins, batch_size, phantom_rows=None, capacity=None, protein_slots=None, protein_phantom_rows=None,
                  protein_capacity=None):
        """The refillable batch of ``batch_size`` (ligand, protein) pairs for ``ArchitectureDTI.forward_shared`` — ``first`` = ligand id in
        the ``DeviceDataset`` ``ligands`` (which carries no ``y``), ``second`` = protein id in the ``Batch`` ``proteins``: see
        ``ResidentDTIBatch``.  ``phantom_rows`` / ``capacity``: as ``DeviceDataset.padded``.

        ``proteins`` a ``DeviceDataset`` (no ``y``) instead: ``second`` = protein id in that dataset, and the protein side is refilled per
        load too — a padded batch of ``protein_slots`` protein graphs (``protein_phantom_rows`` / ``protein_capacity``: as
        ``DeviceDataset.padded``), so a step runs the protein tower over the step's distinct proteins, not over the dataset's: see
        ``ResidentDTIRefillBatch``."""
        if isinstance(proteins, DeviceDataset):
            if protein_slots is None:
                raise ValueError("dti_batch: a DeviceDataset of proteins needs protein_slots = the protein graphs a step holds")
            return ResidentDTIRefillBatch(self, ligands, proteins, batch_size, protein_slots, phantom_rows, capacity, protein_phantom_rows,
                                          protein_capacity)
        if protein_slots is not None or protein_phantom_rows is not None or protein_capacity is not None:
            raise ValueError("dti_batch: protein_slots / protein_phantom_rows / protein_capacity go with a DeviceDataset of proteins; a "
                             "Batch of proteins is held whole")
        return ResidentDTIBatch(self, ligands, proteins, batch_size, phantom_rows, capacity)

    def ddi_batch(self, drugs1, drugs2=None, batch_size=32):
        """The refillable batch of ``batch_size`` (drug, drug) pairs for ``ArchitectureDDI.forward_shared`` — ``first`` = drug id in the
        ``Batch`` ``drugs1``, ``second`` = drug id in ``drugs2`` (``None``: ``drugs1`` serves both towers): see ``ResidentDDIBatch``."""
        return ResidentDDIBatch(self, drugs1, drugs2, batch_size)


class _ResidentPairBatch:
    """What the two resident pair batches share: the fixed device table a load fills (one pinned, non-blocking copy), an epoch's tables
    from one upload (``load_many`` / ``load(step=i)``), and the reload protocol of ``PaddedBatch`` — ``load(launch=False)`` uploads only
    and ``glam_reload()`` enqueues the launches on the current stream, first in the step of a ``GraphedTrainStep``, so that a capture holds
    them; outside a capture a ``load`` that has launched already is not repeated.  Subclasses give ``_host_table(ids)`` (the checked int32
    table of one load, ``ValueError`` / ``IndexError`` before anything is enqueued) and ``_enqueue()`` (the launches)."""

    def _init_table(self, words, device):
        self._table = torch.zeros(words, dtype=torch.int32, device=device)
        self._tables, self._launched = None, False

    def load(self, ids=None, step=None, launch=True):
        """Put the pairs ``ids`` — exactly ``B`` pair ids of the ``ResidentPairs`` table, host integers — into this batch; ``step=i``
        instead: table ``i`` of the last ``load_many``, a device-to-device copy.  ``launch=False`` uploads the table only, for a batch
        that a ``GraphedTrainStep`` runs next.  ``IndexError`` for ids outside the table, ``ValueError`` for another count than ``B`` (a
        caller runs a shorter last batch eagerly on a host ``ops.pair_index``, or drops it) or slots beyond the capacity — before
        anything is enqueued."""
        if (ids is None) == (step is None):
            raise ValueError(f"{type(self).__name__}.load takes either ids or step=")
        if step is not None:
            if self._tables is None or not 0 <= int(step) < self._tables.size(0):
                raise IndexError(f"step {step}: load_many has uploaded {0 if self._tables is None else self._tables.size(0)} tables")
            self._table.copy_(self._tables[int(step)])
        else:
            table = self._host_table(ids)
            from . import _lib
            _lib.require_device(self._table)
            staged = torch.empty(table.shape, dtype=torch.int32, pin_memory=True)
            staged.numpy()[...] = table
            self._table.copy_(staged, non_blocking=True)
        self._launched = False
        if launch:
            self.glam_reload()
            self._launched = True
        return self

    def load_many(self, id_lists):
        """The tables of ``len(id_lists)`` loads (an epoch's) from one numpy pass and ONE upload; ``load(step=i)`` then installs table
        ``i``.  Same errors as ``load``, for every list, before anything is enqueued.  Returns the number of tables."""
        tables = [self._host_table(ids) for ids in id_lists]
        stacked = np.stack(tables) if tables else np.zeros((0, self._table.numel()), dtype=np.int32)
        staged = torch.empty(stacked.shape, dtype=torch.int32, pin_memory=True)
        staged.numpy()[...] = stacked
        self._tables = staged.to(self._table.device, non_blocking=True)
        return len(tables)

    def glam_reload(self):
        """The reload hook of ``GraphedTrainStep``: enqueue this batch's launches for the table now on the device, on the current stream."""
        if self._launched and not torch.cuda.is_current_stream_capturing():
            self._launched = False
            return
        self._enqueue()


def _check_ids_below(col, n, what, things):
    if col.size and int(col.max()) >= n:
        raise IndexError(f"ResidentPairs: the {what} column names {things} up to {int(col.max())}, but only {n} are given")


class ResidentDTIBatch(_ResidentPairBatch):
    """One batch of FIXED CAPACITY of ``B`` (ligand, protein) pairs, refilled in place by ``load(pair_ids)`` — two launches behind one
    small copy: the padded collate of the ligands (``glam_collate_padded``) and ``glam_pair_list_load`` for the pair -> protein lists and
    the labels — so a ``GraphedTrainStep(SharedStep(model), ...)`` captures ONE graph and replays it for every batch of a shuffled epoch.

    ``mol``: a ``PaddedBatch`` of ``num_graphs = B + K`` ligand graphs (``K`` phantom graphs, ``phantom_rows``); ``pro``: the ``Batch`` of the
    ``Q`` distinct proteins, held once, on the device — EVERY step runs the protein tower over all of them, which fits a target set or a
    panel of tens of proteins, not thousands of long ones; ``index``: ``ops.PairList(B + K, Q)`` whose phantom ligand slots point at protein
    ``pad = 0`` (their output rows stay out of the loss: ``graphs.padded_loss``); ``y`` ``[B, r]``: the pairs' labels; ``num_real_graphs = B``.
    Exactly ``B`` pair ids per load — a shorter last batch runs eagerly on a host ``ops.pair_index``, or is dropped."""

    def __init__(self, pairs, ligands, proteins, batch_size, phantom_rows=None, capacity=None):
        from . import ops
        if not isinstance(ligands, DeviceDataset) or ligands.y is not None:
            raise ValueError("dti_batch: ligands must be a DeviceDataset without y (the labels belong to the pairs: ResidentPairs.y)")
        dev = pairs.device
        if ligands.device != dev:
            raise ValueError(f"dti_batch: the ligands live on {ligands.device}, the pair table on {dev}")
        Q = int(getattr(proteins, "num_graphs", 0))
        if Q < 1:
            raise ValueError("dti_batch: proteins must be a collated Batch of the Q >= 1 distinct proteins")
        _check_ids_below(pairs.first_host, ligands.n, "first", "ligands")
        _check_ids_below(pairs.second_host, Q, "second", "proteins")
        self.pairs, B = pairs, int(batch_size)
        if B < 1:
            raise ValueError(f"dti_batch: batch_size must be >= 1, got {batch_size}")
        mol = PaddedBatch(ligands, B, capacity, phantom_rows, labels=False)
        self.index = ops.PairList(mol.num_graphs, Q, dev, pad=0)          # (refuses a list beyond the kernel's bounds)
        self.mol, self.pro = mol, proteins if proteins.x.device == dev else proteins.to(dev)
        self.y = torch.empty((B,) + pairs.y.shape[1:], dtype=pairs.y.dtype, device=dev)
        self.num_graphs, self.num_real_graphs = mol.num_graphs, B
        self._init_table(4 * (B + 1) + B, dev)
        mol._table = self._table[:4 * (B + 1)].view(4, B + 1)             # (the ligand slot table travels in this batch's one copy)
        self._ids = self._table[4 * (B + 1):]

    def _host_table(self, ids):
        ds = self.mol._ds
        table, N, E = dti_tables(ids, self.pairs.first_host, ds.ns, ds.es, self.num_real_graphs)
        self.mol._fit(self.num_real_graphs, N, E)
        return table

    def _enqueue(self):
        from . import ops
        self.mol._launched = False
        self.mol.glam_reload()
        ops.pair_list_launch(self._ids, None, None, self.index, self.pairs.second, self.num_real_graphs, self.pairs.y, self.y)

    def glam_admission(self, model):
        """The admission check a ``GraphedTrainStep`` runs on its first step with this batch (``graphs.dti_admission``): ``padded_admission``'s
        rules for the ligand tower and the head, the protein tower exempt.  ``model``: the ``SharedStep`` or the ``ArchitectureDTI``."""
        from .graphs import dti_admission
        return dti_admission(getattr(model, "model", model))


class ResidentDTIRefillBatch(_ResidentPairBatch):
    """``ResidentDTIBatch`` whose PROTEIN side is refilled too: a step runs the protein tower over the step's distinct
    proteins — at most ``Qb = protein_slots`` of a ``DeviceDataset`` of hundreds or thousands — not over the whole dataset.  One small copy
    and four launches per load: the ligand collate, the protein collate (``glam_collate_padded`` / ``_split``, unchanged), the pair lists
    from the uploaded keys (``PairList``'s staged-keys launch) and the label gather (``glam_pair_list_load`` without a side).

    ``mol``: as ``ResidentDTIBatch``; ``pro``: a ``PaddedBatch`` of ``Qb + Kp`` protein graphs whose ``edge_index`` carries the mark of
    ``ops.mark_gcn_inline`` (``layer.GCNConv`` then reads self-loops and normalisation from the batch's own CSR, csrc/gcn.hip);
    ``index``: ``ops.PairList(B + K, Qb + Kp, pad=0)``; ``y`` ``[B, r]``.  The slots of a load (``protein_slot_ids``): the sorted distinct
    proteins ``u`` of its pairs, then ``Qb - U`` fillers — real proteins without a pair: an empty list, a zero gradient; ``slots`` / ``keys``
    / ``distinct`` keep the last ``load(ids)``'s on the host.  Order contract: the real part of ``pro`` equals ``proteins.collate(slots)``
    field by field, ``index`` the lists ``ops.pair_index(keys, B + K, Qb + Kp)`` builds on the host, bit for bit.  ``ValueError`` for a
    load with more than ``Qb`` distinct proteins, before anything is enqueued."""

    def __init__(self, pairs, ligands, proteins, batch_size, protein_slots, phantom_rows=None, capacity=None, protein_phantom_rows=None,
                 protein_capacity=None):
        from . import ops
        if not isinstance(ligands, DeviceDataset) or ligands.y is not None:
            raise ValueError("dti_batch: ligands must be a DeviceDataset without y (the labels belong to the pairs: ResidentPairs.y)")
        if not isinstance(proteins, DeviceDataset) or proteins.y is not None:
            raise ValueError("dti_batch: refilled proteins must be a DeviceDataset without y")
        dev = pairs.device
        for name, ds in (("ligands", ligands), ("proteins", proteins)):
            if ds.device != dev:
                raise ValueError(f"dti_batch: the {name} live on {ds.device}, the pair table on {dev}")
        _check_ids_below(pairs.first_host, ligands.n, "first", "ligands")
        _check_ids_below(pairs.second_host, proteins.n, "second", "proteins")
        self.pairs, B, Qb = pairs, int(batch_size), int(protein_slots)
        if B < 1:
            raise ValueError(f"dti_batch: batch_size must be >= 1, got {batch_size}")
        if not 1 <= Qb <= proteins.n:
            raise ValueError(f"dti_batch: protein_slots must lie in 1 .. {proteins.n} (the dataset's proteins), got {protein_slots}")
        mol = PaddedBatch(ligands, B, capacity, phantom_rows, labels=False)
        pro = PaddedBatch(proteins, Qb, protein_capacity, protein_phantom_rows, labels=False)
        ops.mark_gcn_inline(pro.edge_index)
        self.index = ops.PairList(mol.num_graphs, pro.num_graphs, dev, pad=0)
        self.mol, self.pro = mol, pro
        self.y = torch.empty((B,) + pairs.y.shape[1:], dtype=pairs.y.dtype, device=dev)
        self.num_graphs, self.num_real_graphs, self.protein_slots = mol.num_graphs, B, Qb
        # one table, one copy: ligand slots | pair ids | protein slots | keys
        cuts = np.cumsum([0, 4 * (B + 1), B, 4 * (Qb + 1), mol.num_graphs]).tolist()
        self._init_table(cuts[-1], dev)
        mol._table = self._table[cuts[0]:cuts[1]].view(4, B + 1)
        self._ids = self._table[cuts[1]:cuts[2]]
        pro._table = self._table[cuts[2]:cuts[3]].view(4, Qb + 1)
        self.index._stage = self._table[cuts[3]:cuts[4]]              # (the list's launch reads the keys where this batch's copy lands)
        self._cuts = cuts
        self.slots = self.keys = self.distinct = None

    def _host_table(self, ids):
        lig, pro = self.mol._ds, self.pro._ds
        B, Qb = self.num_real_graphs, self.protein_slots
        table, (N, E), (Np, Ep) = dti_refill_tables(ids, self.pairs.first_host, self.pairs.second_host, lig.ns, lig.es, pro.ns, pro.es, B, Qb,
                                                    self.mol.num_phantom_graphs)
        self.mol._fit(B, N, E)
        self.pro._fit(Qb, Np, Ep)
        c = self._cuts
        self.slots, self.keys = table[c[2]:c[2] + Qb].astype(np.int64), table[c[3]:c[3] + B].copy()
        self.distinct = int(self.keys.max()) + 1
        return table

    def _enqueue(self):
        from . import ops
        for part in (self.mol, self.pro, self.index):
            part._launched = False
            part.glam_reload()
        ops.pair_list_launch(self._ids, None, None, None, None, self.num_real_graphs, self.pairs.y, self.y)

    def glam_admission(self, model):
        """``graphs.dti_refill_admission``: ``dti_admission``'s rules, and ``padded_admission``'s for the protein tower with ``_GCNConv``
        admitted.  ``model``: the ``SharedStep`` or the ``ArchitectureDTI``."""
        from .graphs import dti_refill_admission
        return dti_refill_admission(getattr(model, "model", model))


class ResidentDDIBatch(_ResidentPairBatch):
    """One batch of FIXED CAPACITY of ``B`` (drug, drug) pairs, refilled in place by ``load(pair_ids)`` — ONE launch behind one small copy
    (``glam_pair_list_load``: both sides' lists and the labels) — so a ``GraphedTrainStep(SharedStep(model), ...)`` captures ONE graph and
    replays it for every batch of a shuffled epoch.

    ``mol1`` / ``mol2``: the ``Batch`` of the ``Q1`` / ``Q2`` distinct drugs of each side, held once, on the device (one ``Batch`` may serve
    both) — EVERY step runs both towers over all of them (DrugBank's ~1.7 k drugs fit); ``first`` / ``second``: ``ops.PairList(B, Q1)`` /
    ``(B, Q2)``; ``y`` ``[B, r]``; ``num_real_graphs = B``: no phantom.  Exactly ``B`` pair ids per load — a shorter last batch runs eagerly
    on host ``ops.pair_index`` lists, or is dropped."""

    def __init__(self, pairs, drugs1, drugs2=None, batch_size=32):
        from . import ops
        dev = pairs.device
        drugs2 = drugs1 if drugs2 is None else drugs2
        Q1, Q2 = int(getattr(drugs1, "num_graphs", 0)), int(getattr(drugs2, "num_graphs", 0))
        if Q1 < 1 or Q2 < 1:
            raise ValueError("ddi_batch: drugs1 / drugs2 must be collated Batches of the distinct drugs of each side")
        _check_ids_below(pairs.first_host, Q1, "first", "drugs")
        _check_ids_below(pairs.second_host, Q2, "second", "drugs")
        self.pairs, B = pairs, int(batch_size)
        if B < 1:
            raise ValueError(f"ddi_batch: batch_size must be >= 1, got {batch_size}")
        self.first = ops.PairList(B, Q1, dev, name="first", over="drugs")
        self.second = ops.PairList(B, Q2, dev, name="second", over="drugs")
        same = drugs2 is drugs1
        self.mol1 = drugs1 if drugs1.x.device == dev else drugs1.to(dev)
        self.mol2 = self.mol1 if same else (drugs2 if drugs2.x.device == dev else drugs2.to(dev))
        self.y = torch.empty((B,) + pairs.y.shape[1:], dtype=pairs.y.dtype, device=dev)
        self.num_graphs = self.num_real_graphs = B
        self._init_table(B, dev)

    def _host_table(self, ids):
        return ddi_table(ids, self.pairs.n, self.num_real_graphs)

    def _enqueue(self):
        from . import ops
        ops.pair_list_launch(self._table, self.first, self.pairs.first, self.second, self.pairs.second, self.num_real_graphs,
                             self.pairs.y, self.y)

    def glam_admission(self, model):
        """No phantom: nothing to admit beyond ``forward_shared``'s own refusals (a no-op context)."""
        import contextlib
        return contextlib.nullcontext()


class DataLoader:
    """Sequential mini-batch iterator over a list of ``Data`` (the reference's train
    loader does not shuffle: ``src_1gp/trainer.py:37-38``).

    ``device`` / ``cache``: without shuffling the batch composition repeats every epoch, so the collated batches
    can be built and moved to the device ONCE and handed out again as the same tensor objects.  The CSR staging of
    ``ops.graph_index`` is keyed on the ``edge_index`` object, so from the second epoch on a step does no
    collation, no host-to-device copy, no CSR build and no validation sync.

    ``resident=True`` (needs a ``device``): the dataset moves to the device once, index included (``DeviceDataset``), and every batch
    — in the same order, from the same shuffle — is one launch behind one small copy, its graph index installed: what a loop that
    shuffles, samples or walks a library larger than the cache pays per FRESH batch.  ``cache`` keeps its meaning.

    ``padded=True`` (needs ``resident=True``): every FULL batch of an epoch is the SAME ``PaddedBatch`` object, reloaded — same order, same
    shuffle — so that a ``GraphedTrainStep`` captures one graph and replays it for all of them; whoever keeps a yielded batch sees the
    next one in it.  An epoch's tables are uploaded at once (``PaddedBatch.load_many``).  A short last batch comes from the ordinary
    ``collate``.  ``collate_in_step=True``: the loader uploads the table only and leaves the launch to the stepper's graph.
    ``phantom_rows``: handed to ``DeviceDataset.padded`` (several bounded phantom graphs; the size to use at large batches)."""

    def __init__(self, dataset, batch_size=32, shuffle=False, seed=0, device=None, cache=None, resident=False, padded=False,
                 collate_in_step=False, phantom_rows=None):
        self.dataset, self.batch_size, self.shuffle, self.seed = list(dataset), batch_size, shuffle, seed
        self.device = device
        self.padded, self._padded, self.collate_in_step = bool(padded), None, bool(collate_in_step)
        if self.padded and not resident:
            raise ValueError("DataLoader: padded=True reloads one batch of a device-resident dataset: pass resident=True")
        if phantom_rows is not None and not self.padded:
            raise ValueError("DataLoader: phantom_rows shapes the phantom graphs of padded batches: pass padded=True")
        self.phantom_rows = None if phantom_rows is None else _phantom_rows(phantom_rows)
        if self.padded and cache:
            raise ValueError("DataLoader: padded=True hands out one batch object, reloaded: there is nothing to cache")
        self.cache = (not shuffle and not self.padded) if cache is None else bool(cache)
        if self.cache and shuffle:
            raise ValueError("DataLoader: cached batches need a fixed order (shuffle=False)")
        self._epoch = 0
        self._batches = None
        self._packed = None
        self.resident, self._resident = bool(resident), None
        if self.resident:
            if device is None:
                raise ValueError("DataLoader: resident=True keeps the dataset on a device: pass device=")
            try:
                self._packed = PackedDataset(self.dataset)
            except (ValueError, AttributeError, RuntimeError) as e:
                raise ValueError(f"DataLoader: resident=True needs records of one layout ({e})") from e

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _collate(self, idx):
        if self.resident:
            if self._resident is None:
                self._resident = DeviceDataset(self._packed, self.device)
            return self._resident.collate(idx)
        if self._packed is None:
            try:
                self._packed = PackedDataset(self.dataset)
            except (ValueError, AttributeError, RuntimeError):    # heterogeneous records: per-batch concatenation
                self._packed = False
        with _few_threads():
            b = self._packed.collate(idx) if self._packed else Batch.from_data_list([self.dataset[i] for i in idx])
            return b if self.device is None else b.to(self.device)

    def __iter__(self):
        order = np.arange(len(self.dataset))
        if self.shuffle:
            np.random.default_rng(self.seed + self._epoch).shuffle(order)
        self._epoch += 1
        if self.cache:
            if self._batches is None:
                self._batches = [self._collate(order[s:s + self.batch_size]) for s in range(0, len(order), self.batch_size)]
            yield from self._batches
            return
        full = 0
        if self.padded and len(order) >= self.batch_size:
            if self._resident is None:
                self._resident = DeviceDataset(self._packed, self.device)
            if self._padded is None:
                self._padded = self._resident.padded(self.batch_size, phantom_rows=self.phantom_rows)
            full = self._padded.load_many(order[:len(order) // self.batch_size * self.batch_size].reshape(-1, self.batch_size))
            for i in range(full):
                yield self._padded.load(step=i, launch=not self.collate_in_step)
        for s in range(full * self.batch_size, len(order), self.batch_size):
            yield self._collate(order[s:s + self.batch_size])


# --------------------------------------------------------------------------------------
# synthetic graphs
# --------------------------------------------------------------------------------------
def _mol_arrays(rng, n_min=12, n_max=28):
    n = int(rng.integers(n_min, n_max + 1))
    bonds = {(i, i + 1) for i in range(n - 1)}
    for _ in range(max(1, n // 10)):
        i = int(rng.integers(0, max(1, n - 3)))
        j = min(n - 1, i + int(rng.integers(3, 6)))
        if j > i:
            bonds.add((i, j))
    bonds = sorted(bonds)
    btype = rng.integers(0, 4, size=len(bonds))
    src = np.array([b[0] for b in bonds] + [b[1] for b in bonds], dtype=np.int64)
    dst = np.array([b[1] for b in bonds] + [b[0] for b in bonds], dtype=np.int64)
    bt = np.concatenate([btype, btype])
    perm = np.argsort(src * n + dst, kind="stable")
    src, dst, bt = src[perm], dst[perm], bt[perm]
    edge_attr = np.zeros((src.size, 4), dtype=np.float32)
    edge_attr[np.arange(src.size), bt] = 1.0
    at = rng.integers(0, 9, size=n)
    hyb = rng.integers(0, 3, size=n)
    x = np.zeros((n, 15), dtype=np.float32)
    x[np.arange(n), at] = 1.0
    x[np.arange(n), 9 + hyb] = 1.0
    x[:, 12] = _ATOMIC_NUMBERS[at]
    x[:, 13] = rng.integers(0, 2, size=n)
    x[:, 14] = rng.integers(0, 4, size=n)
    return x, np.stack([src, dst]), edge_attr


def synth_molecule(rng, n_tasks=1, task="regression"):
    x, ei, ea = _mol_arrays(rng)
    if task == "regression":
        y = rng.standard_normal((1, n_tasks)).astype(np.float32)
    else:  # multi-task labels with -1 = missing (src_1gp/dataset.py:138)
        y = rng.integers(-1, 2, size=(1, n_tasks)).astype(np.float32)
    return Data(torch.from_numpy(x), torch.from_numpy(ei), torch.from_numpy(ea), torch.from_numpy(y))


def synth_protein(rng, n_min=200, n_max=800, contacts_per_res=4.0):
    n = int(rng.integers(n_min, n_max + 1))
    chain = np.arange(n - 1, dtype=np.int64)
    m = int(contacts_per_res * n / 2)
    a = rng.integers(0, n, size=m)
    b = rng.integers(0, n, size=m)
    keep = a != b
    a, b = a[keep], b[keep]
    src = np.concatenate([chain, chain + 1, a, b])
    dst = np.concatenate([chain + 1, chain, b, a])
    x = rng.standard_normal((n, 49)).astype(np.float32)
    ea = rng.random((src.size, 8)).astype(np.float32)
    y = rng.standard_normal((1, 1)).astype(np.float32)
    return Data(torch.from_numpy(x), torch.from_numpy(np.stack([src, dst])), torch.from_numpy(ea),
                torch.from_numpy(y))


def synth_batch(num_graphs, seed=0, n_tasks=1, task="regression"):
    """ESOL-shaped batch: ``num_graphs`` synthetic molecules collated the
    PyG way.  B=1024, seed 0 gives N~20.7k nodes, E~42.5k directed edges."""
    rng = np.random.default_rng(seed)
    xs, eis, eas, bs, ys = [], [], [], [], []
    off = 0
    for g in range(num_graphs):
        x, ei, ea = _mol_arrays(rng)
        xs.append(x)
        eis.append(ei + off)
        eas.append(ea)
        bs.append(np.full(x.shape[0], g, dtype=np.int64))
        off += x.shape[0]
    if task == "regression":
        y = rng.standard_normal((num_graphs, n_tasks)).astype(np.float32)
    else:
        y = rng.integers(-1, 2, size=(num_graphs, n_tasks)).astype(np.float32)
    out = Batch(torch.from_numpy(np.concatenate(xs)), torch.from_numpy(np.concatenate(eis, 1)),
                torch.from_numpy(np.concatenate(eas)), torch.from_numpy(y),
                torch.from_numpy(np.concatenate(bs)))
    out.num_graphs = num_graphs
    sizes = np.array([x.shape[0] for x in xs])
    out.ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]))
    return out


def synth_protein_batch(num_graphs, seed=0, n_min=200, n_max=800):
    rng = np.random.default_rng(seed)
    return Batch.from_data_list([synth_protein(rng, n_min, n_max) for _ in range(num_graphs)])
