"""Shared by tests/test_index_cases_host.py (CPU) and tests/test_gpu_index_kernels.py (GPU): the edge lists, batch vectors and word
buffers on which the INDEX kernels can go wrong — ``glam_csr_build`` / ``glam_batch_ptr`` (csrc/csr.hip), ``glam_ell_build``
(csrc/triplet_pipe.hip), ``glam_batch_fingerprint`` (csrc/core.hip) — and a plain restatement of each.  numpy and torch only; imports
no HIP and nothing of ``glam_amd``.  Integers in, integers out: every comparison made with these is exact.

Why these cases.  The CSR build is count (atomics) -> three-level exclusive scan (2 048 items per block, 8 per thread; the block sums
scanned by ONE block, 256 at a time with a carry) -> fill (atomic cursor, arrival order) -> one thread per segment restoring edge-id
order (insertion sort up to 32 entries, heap sort above).  Every grid but the scan's is capped at 2 048 blocks of 256 threads and
strides beyond.  So the sizes that matter are 8 and 2 048 items (``scan_edges``), 256 scan blocks (``second_chunk``), 524 288 work
items (``second_chunk``: nodes, ``many_edges``: edges, the long batch vector) and segment lengths 32 / 33 (``segment_ladder``).  Each
builder asserts the properties it exists for, so that an edit cannot quietly lose the edge it covers."""
import functools
import types

import numpy as np
import torch

SCAN_ITEMS = 2048                      # items per scan block (csrc/csr.hip: kScanItems)
SCAN_THREAD_ITEMS = 8                  # consecutive items per thread of k_scan_apply
BLOCK = 256                            # kBlock: threads per block, and block sums per chunk of k_scan_top
MAX_BLOCKS = 2048                      # kMaxBlocks: the cap of the grid-stride grids
TRIP = BLOCK * MAX_BLOCKS              # 524 288 work items: what one trip of a capped grid covers
SORT_SWITCH = 32                       # longest segment that k_csr_sort_segments sorts by insertion
MAX_SEGMENT = 4096                     # no case holds a longer segment (one thread sorts a segment)
ELL_WIDTH = 4
U64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------
# the launch geometry, restated
# ---------------------------------------------------------------------------------------------
def scan_blocks(N):
    """Blocks of ``k_scan_block_sums`` / ``k_scan_apply``: the scan runs over the ``N + 1`` entries of ``rowptr``."""
    return (N + 1 + SCAN_ITEMS - 1) // SCAN_ITEMS


def scan_top_chunks(N):
    """Trips of ``k_scan_top``'s loop over the block sums (256 per trip; from the second on, the carry counts)."""
    return (scan_blocks(N) + BLOCK - 1) // BLOCK


def grid_for(work, per_block=BLOCK, cap=MAX_BLOCKS):
    return min(max((work + per_block - 1) // per_block, 1), cap)


def trips(work, per_block=BLOCK, cap=MAX_BLOCKS):
    """Most trips any thread of a capped grid-stride loop over ``work`` items makes."""
    g = grid_for(work, per_block, cap)
    return (work + g * BLOCK - 1) // (g * BLOCK)


def _np_edges(edge_index):
    ei = edge_index.numpy() if isinstance(edge_index, torch.Tensor) else np.asarray(edge_index)
    assert ei.dtype == np.int64 and ei.ndim == 2 and ei.shape[0] == 2
    return ei


# ---------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------
def valid_edges(edge_index, N):
    """Mask of the edges whose ids lie in ``[0, N)`` on BOTH rows (the others are dropped by count and fill alike)."""
    ei = _np_edges(edge_index)
    return (ei[0] >= 0) & (ei[0] < N) & (ei[1] >= 0) & (ei[1] < N)


def csr_ref(edge_index, N, by):
    """``(ptr[N + 1], nbr[V], eid[V])`` int32 of ``glam_csr_build``: the valid edges sorted STABLY by the key row (``by = 0``: row 1,
    the target — ``nbr`` holds sources; ``by = 1``: row 0), ``ptr`` the cumulative sum of the key's bincount, ``eid`` the position of
    each edge in ``edge_index`` (invalid edges keep their numbers: they are skipped, not renumbered)."""
    ei = _np_edges(edge_index)
    key, val = (ei[1], ei[0]) if by == 0 else (ei[0], ei[1])
    keep = np.flatnonzero(valid_edges(ei, N))
    order = keep[np.argsort(key[keep], kind="stable")]
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(key[keep], minlength=N), out=ptr[1:])
    return ptr.astype(np.int32), val[order].astype(np.int32), order.astype(np.int32)


def ell_ref(ptr, nbr, eid, N):
    """``(ell_nbr[N, 4], ell_eid[N, 4], overflow)`` of ``glam_ell_build``: the first ``min(deg, 4)`` entries of every segment in order,
    -1 in the free slots; ``overflow`` iff some degree exceeds 4 (the records are written all the same)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    deg = ptr[1:] - ptr[:-1]
    slot = np.arange(ELL_WIDTH)[None, :]
    take = slot < np.minimum(deg, ELL_WIDTH)[:, None]
    pos = np.where(take, ptr[:-1, None] + slot, 0)
    pad = lambda a: np.concatenate([np.asarray(a, dtype=np.int32), np.zeros(1, np.int32)])       # (pos 0 of an empty list)
    ell_nbr = np.where(take, pad(nbr)[pos], -1).astype(np.int32).reshape(N, ELL_WIDTH)
    ell_eid = np.where(take, pad(eid)[pos], -1).astype(np.int32).reshape(N, ELL_WIDTH)
    return ell_nbr, ell_eid, bool((deg > ELL_WIDTH).any())


def batch_ptr_ref(batch, B=None):
    """``ptr[B + 1]`` int32 of ``glam_batch_ptr`` (``ptr[g]``: the first node of graph ``g``, empty graphs included), or ``None`` for
    an invalid vector: decreasing somewhere, or an id outside ``[0, B)``.  ``B = None``: inferred as ``batch[-1] + 1`` (0 when empty)."""
    b = batch.numpy() if isinstance(batch, torch.Tensor) else np.asarray(batch)
    assert b.dtype == np.int64 and b.ndim == 1
    if B is None:
        B = int(b[-1]) + 1 if b.size else 0
    if B < 0 or (b.size and ((b < 0).any() or (b >= B).any() or (b[1:] < b[:-1]).any())):
        return None
    ptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.bincount(b, minlength=B), out=ptr[1:])
    return ptr.astype(np.int32)


FP_SALT = 0x9E3779B97F4A7C15
FP_M1, FP_M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def fp_mix(z):
    """The splitmix64 finaliser on a uint64 array (multiplication mod 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(FP_M1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(FP_M2)
    return z ^ (z >> np.uint64(31))


def fp_salt(t):
    return np.uint64((FP_SALT * (t + 1)) & U64)


def fingerprint_ref(buffers):
    """``glam_batch_fingerprint`` of up to four buffers of 32-bit words, as a Python int in ``[0, 2^64)``: every word ``w`` at index
    ``i`` of buffer ``t`` (its POSITION among the buffers, empty ones counted) contributes
    ``mix((w << 32 | i mod 2^32) ^ salt_t ^ (i >> 32))`` with ``salt_t = 0x9E3779B97F4A7C15 * (t + 1)``; the sum is taken mod 2^64."""
    assert 1 <= len(buffers) <= 4
    total = 0
    with np.errstate(over="ignore"):
        for t, buf in enumerate(buffers):
            w = np.asarray(buf).view(np.uint32).astype(np.uint64)
            i = np.arange(w.size, dtype=np.uint64)
            z = ((w << np.uint64(32)) | (i & np.uint64(0xFFFFFFFF))) ^ fp_salt(t) ^ (i >> np.uint64(32))
            total += int(fp_mix(z).sum(dtype=np.uint64))
    return total & U64


# ---------------------------------------------------------------------------------------------
# graph cases
# ---------------------------------------------------------------------------------------------
def degrees(edge_index, N):
    """``(in_degree[N], out_degree[N])`` over the valid edges."""
    ei = _np_edges(edge_index)
    ei = ei[:, valid_edges(ei, N)]
    return np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)


def _graph(name, ei, N, **props):
    ei = torch.from_numpy(np.ascontiguousarray(np.asarray(ei, dtype=np.int64).reshape(2, -1)))
    din, dout = degrees(ei, N)
    assert max(int(din.max(initial=0)), int(dout.max(initial=0))) <= MAX_SEGMENT, f"{name}: a segment longer than {MAX_SEGMENT}"
    return types.SimpleNamespace(name=name, edge_index=ei, N=N, E=ei.size(1), **props)


SCAN_EDGE_N = (0, 1, 7, 8, 9, 2046, 2047, 2048, 2049, 4096)


def scan_marks(N):
    """The nodes of ``scan_edges``: first, last, and both neighbours of every thread edge (8) and block edge (2 048, 4 096) below N."""
    marks = {0, N - 1}
    for edge in (SCAN_THREAD_ITEMS, SCAN_ITEMS, 2 * SCAN_ITEMS):
        marks |= {edge - 1, edge}
    return sorted(m for m in marks if 0 <= m < N)


def scan_edges(N):
    """Edges on the marked nodes only (``scan_marks``): mark ``k`` sends ``k % 3 + 1`` parallel edges to the next mark and one to the
    one before (cyclically; a lone mark to itself), the list then reversed so that keys do not arrive in order.  Every other node
    is isolated, so a ``rowptr`` that is off by one item shows as an edge on a node that has none."""
    marks = scan_marks(N)
    src, dst = [], []
    for k, m in enumerate(marks):
        src += [m] * (k % 3 + 1) + [m]
        dst += [marks[(k + 1) % len(marks)]] * (k % 3 + 1) + [marks[k - 1]]
    g = _graph(f"scan_edges[{N}]", [src[::-1], dst[::-1]], N, marks=marks)
    din, dout = degrees(g.edge_index, N)
    assert (N == 0) == (g.E == 0)
    assert sorted(np.flatnonzero(din)) == marks and sorted(np.flatnonzero(dout)) == marks          # the rest is isolated
    assert scan_blocks(N) == {0: 1, 1: 1, 7: 1, 8: 1, 9: 1, 2046: 1, 2047: 1, 2048: 2, 2049: 2, 4096: 3}[N]
    return g


LADDER = (0, 1, 2, 31, 32, 33, 64, 257, 1000)
LADDER_N = 1033
LADDER_ORDERS = ("ascending", "descending", "shuffled")


def segment_ladder(order="shuffled", flip=False):
    """One graph whose nodes ``1 + k`` have key-side degree ``LADDER[k]`` (in-degree; ``flip``: the rows swapped, so the out-degree and
    ``by = 1`` see the ladder).  Nodes 0 and N - 1 are isolated.  Sources are drawn without repetition inside a segment from the nodes
    behind the ladder, except for what is put in on purpose:

    * ``loop_only``: the node of degree 1 — its only edge is a self-loop;
    * ``tie``: the node of degree 33 (the shortest heap-sorted segment) — three of its edges come from the same source ``tie_src``.

    ``order``: the edge list sorted by key ascending (a stable sort has nothing to do), descending (with the edges of a segment in
    reverse drawing order), or shuffled."""
    rng = np.random.default_rng(20)
    N = LADDER_N
    first_src = 1 + len(LADDER)
    pool = np.arange(first_src, N - 1)
    loop_only, tie = 1 + LADDER.index(1), 1 + LADDER.index(33)
    src, dst, tie_src = [], [], None
    for k, d in enumerate(LADDER):
        n = 1 + k
        s = rng.permutation(pool)[:d]
        if n == loop_only:
            s[:] = n
        if n == tie:
            s[[7, 20]] = s[0]
            tie_src = int(s[0])
        src.append(s)
        dst.append(np.full(d, n))
    ei = np.stack([np.concatenate(src), np.concatenate(dst)])
    ei = {"ascending": ei, "descending": ei[:, ::-1], "shuffled": ei[:, rng.permutation(ei.shape[1])]}[order]
    if flip:
        ei = ei[::-1]
    g = _graph(f"segment_ladder[{order}{',flip' if flip else ''}]", ei, N, loop_only=loop_only, tie=tie, tie_src=tie_src, by=int(flip),
               isolated=(0, N - 1))
    din, dout = degrees(g.edge_index, N)
    walked, other = (dout, din) if flip else (din, dout)
    assert tuple(walked[1:first_src]) == LADDER and not walked[first_src:].any() and walked[0] == 0
    assert all(din[n] == 0 and dout[n] == 0 for n in g.isolated)
    s, d = g.edge_index.numpy()[::-1] if flip else g.edge_index.numpy()
    assert ((s == tie_src) & (d == tie)).sum() == 3 and ((s == d) == (d == loop_only)).all()      # the tie; no other self-loop
    assert {SORT_SWITCH, SORT_SWITCH + 1} <= set(LADDER) and N % 8 and N % 256
    return g


def one_node():
    g = _graph("one_node", np.zeros((2, 40), dtype=np.int64), 1)
    assert g.N == 1 and g.E == 40 > SORT_SWITCH
    return g


SECOND_CHUNK_N = (TRIP - 1, TRIP, TRIP + 1)
_SC_SHIFTS = (1, 17, 101, 333)
_SC_HALF = 350


def second_chunk(N, twin=False):
    """``N`` around 524 288 (256 scan blocks = one chunk of ``k_scan_top`` / 257 = a second chunk of one block sum behind the carry;
    one trip of the node-parallel grids / a second trip of one node).  About 4 000 edges among the ~2 000 nodes within 350 ids of the
    anchors 0, 2 048, 262 144, 524 288 and N - 1 — node ``W[i]`` of that set receives from ``W[i + s]`` for the first ``(7 i + 3) % 5``
    shifts ``s`` of (1, 17, 101, 333), the last node from all four — so every in- and out-degree is at most 4 and both ELL forms
    exist.  ``twin``: one edge more, into the last node (in-degree 5) from a node that had fewer than 4 outgoing edges."""
    rng = np.random.default_rng(N)
    anchors = (0, SCAN_ITEMS, TRIP // 2, TRIP, N - 1)
    W = np.unique(np.concatenate([np.arange(max(a - _SC_HALF, 0), min(a + _SC_HALF, N)) for a in anchors]))
    m = W.size
    d = (7 * np.arange(m) + 3) % 5
    d[-1] = 4
    src, dst = [], []
    for r, s in enumerate(_SC_SHIFTS):
        i = np.flatnonzero(d > r)
        src.append(W[(i + s) % m])
        dst.append(W[i])
    ei = np.stack([np.concatenate(src), np.concatenate(dst)])
    ei = ei[:, rng.permutation(ei.shape[1])]
    extra = None
    if twin:
        dout = np.bincount(ei[0], minlength=N)
        extra = int(W[np.flatnonzero(dout[W] < ELL_WIDTH)[0]])
        ei = np.concatenate([ei, [[extra], [N - 1]]], 1)
    g = _graph(f"second_chunk[{N}{',twin' if twin else ''}]", ei, N, twin=twin, extra_src=extra, window=W)
    din, dout = degrees(g.edge_index, N)
    assert 3500 <= g.E <= 4500 and W[0] == 0 and W[-1] == N - 1
    for a in (1, SCAN_ITEMS, TRIP // 2, TRIP - 1, TRIP, N - 1):  # both neighbours of every block / chunk / trip edge carry edges
        assert all(din[n] + dout[n] > 0 for n in (a - 1, a) if n < N), a
    assert dout.max() <= ELL_WIDTH and din[:-1].max() <= ELL_WIDTH and din[-1] == (5 if twin else 4)
    assert set(range(ELL_WIDTH + 1)) <= set(din) and (ei[1] < TRIP - SCAN_ITEMS).sum() > 0      # a non-zero carry into block 256
    assert scan_blocks(N) == {TRIP - 1: 256, TRIP: 257, TRIP + 1: 257}[N] and scan_top_chunks(N) == (1 if N < TRIP else 2)
    assert trips(N) == (1 if N <= TRIP else 2)
    return g


MANY_EDGES = (1000, TRIP + 3)


def many_edges():
    """Ids uniform under a fixed seed: a second trip of ``k_csr_count`` / ``k_csr_fill`` (three edges behind 2 048 blocks x 256), and
    1 000 heap sorts of about 524 entries."""
    N, E = MANY_EDGES
    g = _graph("many_edges", np.random.default_rng(7).integers(0, N, size=(2, E), dtype=np.int64), N)
    din, dout = degrees(g.edge_index, N)
    assert g.E > TRIP and trips(g.E) == 2 and grid_for(g.E) == MAX_BLOCKS
    assert SORT_SWITCH < min(din.min(), dout.min()) and max(din.max(), dout.max()) < 700
    return g


_BAD_BASE_N = 10


def bad_ids():
    """Edge lists over 10 nodes with ids outside ``[0, 10)``: ``{name: graph}``; ``graph.bad`` lists the positions of the bad edges."""
    N = _BAD_BASE_N
    rng = np.random.default_rng(3)
    base = rng.integers(0, N, size=(2, 24), dtype=np.int64)
    base[:, 5] = base[:, 17]                                       # a duplicate among the valid ones
    edits = {
        "id_equal_N_on_key_row": [(1, 9, N)],
        "negative_id_on_key_row": [(1, 12, -1)],
        "value_row_only": [(0, 9, N + 5)],
        "value_row_only_negative": [(0, 3, -(2 ** 40))],
        "first_edge": [(1, 0, 2 ** 33)],
        "last_edge": [(0, 23, N)],
        "several": [(0, 0, -7), (1, 4, N), (0, 4, N), (1, 11, 2 ** 31), (0, 23, -1), (1, 22, N + 1)],
    }
    out = {}
    for name, e in edits.items():
        ei = base.copy()
        for row, pos, val in e:
            ei[row, pos] = val
        g = _graph(f"bad_ids[{name}]", ei, N, bad=sorted({pos for _, pos, _ in e}))
        assert list(np.flatnonzero(~valid_edges(g.edge_index, N))) == g.bad
        if name.startswith("value_row_only"):                      # the key (by = 0: row 1) of the bad edge is a valid node
            assert all(0 <= int(ei[1, p]) < N for p in g.bad)
        out[name] = g
    assert len(out["several"].bad) == 5 and sum(len(g.bad) == 1 for g in out.values()) == 6
    return out


@functools.lru_cache(maxsize=None)
def graph_case(name):
    """The graph case ``name`` (``GRAPH_CASES``), built once per process; treat it as read-only."""
    return _GRAPH_BUILDERS[name]()


_GRAPH_BUILDERS = {f"scan_edges[{n}]": functools.partial(scan_edges, n) for n in SCAN_EDGE_N}
_GRAPH_BUILDERS.update({f"segment_ladder[{o}{',flip' if f else ''}]": functools.partial(segment_ladder, o, f)
                        for o in LADDER_ORDERS for f in (False, True)})
_GRAPH_BUILDERS["one_node"] = one_node
_GRAPH_BUILDERS.update({f"second_chunk[{n}{',twin' if t else ''}]": functools.partial(second_chunk, n, t)
                        for n in SECOND_CHUNK_N for t in (False, True)})
_GRAPH_BUILDERS["many_edges"] = many_edges
GRAPH_CASES = tuple(_GRAPH_BUILDERS)
BAD_ID_CASES = ("id_equal_N_on_key_row", "negative_id_on_key_row", "value_row_only", "value_row_only_negative", "first_edge",
                "last_edge", "several")


# ---------------------------------------------------------------------------------------------
# batch-vector cases
# ---------------------------------------------------------------------------------------------
def _sizes_to_batch(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)


def _batch_cases():
    """``{name: (batch int64[N], B or None, valid)}``; ``B = None``: the caller leaves ``num_graphs`` to be inferred."""
    c = {}
    c["N0_B0"] = (np.zeros(0, np.int64), 0, True)
    c["N0_B3"] = (np.zeros(0, np.int64), 3, True)
    c["N0_inferred"] = (np.zeros(0, np.int64), None, True)
    c["N1_B1"] = (np.zeros(1, np.int64), 1, True)
    c["N1_inferred_id4"] = (np.full(1, 4, np.int64), None, True)                   # four empty graphs first
    for N in (255, 256, 257):                                                        # one block of k_batch_ptr / its edge / a second block
        sizes = np.array([0, 0, 3, 0, 1, N - 4 - 7, 0, 0, 0, 7, 0, 0])              # empty first, in the middle and last
        c[f"N{N}_empties"] = (_sizes_to_batch(sizes), len(sizes), True)
        c[f"N{N}_inferred"] = (_sizes_to_batch(sizes), None, True)                   # (inferred: the trailing empties are not there)
    c["all_in_last_of_5000"] = (np.full(300, 4999, np.int64), 5000, True)           # thread 0 fills 5 000 entries
    c["all_in_last_of_5000_inferred"] = (np.full(300, 4999, np.int64), None, True)
    c["all_in_first_of_5000"] = (np.zeros(300, np.int64), 5000, True)               # thread N fills 4 999 entries
    rng = np.random.default_rng(11)
    sizes = rng.integers(0, 41, size=26000)
    sizes[:3] = 0
    sizes[-2:] = 0
    sizes[-3] += TRIP + 1 - sizes.sum()
    c["N524289"] = (_sizes_to_batch(sizes), len(sizes), True)                        # a second trip of k_batch_ptr
    ok = _sizes_to_batch(np.array([2, 0, 3, 1, 4]))                                   # 10 nodes, B = 5
    def edit(pos, val):
        b = ok.copy()
        b[pos] = val
        return b
    c["decreasing_first"] = (edit(0, 1), 5, False)
    c["decreasing_middle"] = (edit(5, 1), 5, False)
    c["decreasing_last"] = (edit(9, 3), 5, False)
    c["decreasing_last_inferred"] = (edit(9, 3), None, False)
    c["negative_middle"] = (edit(4, -1), 5, False)
    c["id_equal_B"] = (edit(9, 5), 5, False)
    c["id_equal_B_middle"] = (edit(4, 5), 5, False)
    c["negative_first"] = (edit(0, -3), 5, False)
    c["negative_first_N1"] = (np.full(1, -1, np.int64), 2, False)
    return c


BATCH_CASES = _batch_cases()
for _name, (_b, _B, _valid) in BATCH_CASES.items():
    assert (batch_ptr_ref(_b, _B) is not None) == _valid, _name
assert BATCH_CASES["N524289"][0].size == TRIP + 1 and trips(TRIP + 2) == 2 and trips(258) == 1 and grid_for(258) == 2
assert {b.size for b, _, _ in BATCH_CASES.values()} >= {0, 1, 255, 256, 257, TRIP + 1}


# ---------------------------------------------------------------------------------------------
# fingerprint cases
# ---------------------------------------------------------------------------------------------
FP_TOTALS = (1, 255, 256, 257, 1023, 1024, 1025, 262144, 262145, 300001)


def _words(rng, n, kind):
    if kind == "random":
        w = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    elif kind == "zeros":
        w = np.zeros(n, np.uint32)
    elif kind == "ones":
        w = np.full(n, 0xFFFFFFFF, np.uint32)
    else:                                                             # "repeated": three values, among them 0 and 0xFFFFFFFF
        w = np.array([0, 0xFFFFFFFF, 0x01234567], np.uint32)[rng.integers(0, 3, size=n)]
    return w


def _fp_cases():
    """``{name: [uint32 buffers]}``: 1..4 buffers, a zero-length one in each position, every total of ``FP_TOTALS``."""
    rng = np.random.default_rng(5)
    c = {}
    kinds = ("random", "repeated", "zeros", "ones")
    for k, total in enumerate(FP_TOTALS):                             # the grid of the launch: ceil(total / 1024) blocks, at most 256
        nbuf = k % 4 + 1
        cuts = np.sort(rng.integers(0, total + 1, size=nbuf - 1))
        lens = np.diff(np.concatenate([[0], cuts, [total]]))
        c[f"total_{total}_in_{nbuf}"] = [_words(rng, int(n), kinds[(k + t) % 2]) for t, n in enumerate(lens)]
    for kind in kinds[1:]:
        c[f"{kind}_1000"] = [_words(rng, 1000, kind)]
    base = [_words(rng, n, "random") for n in (5, 300, 77)]
    for pos in range(4):                                              # the buffers behind the empty one move up a salt
        c[f"empty_at_{pos}"] = base[:pos] + [np.zeros(0, np.uint32)] + base[pos:]
    c["empty_only_tail"] = [base[0], np.zeros(0, np.uint32)]
    return c


FP_CASES = _fp_cases()
assert {sum(b.size for b in bufs) for bufs in FP_CASES.values()} >= set(FP_TOTALS)
assert {len(bufs) for bufs in FP_CASES.values()} == {1, 2, 3, 4}
assert grid_for(262144, 4 * BLOCK, 256) == 256 == grid_for(300001, 4 * BLOCK, 256) and grid_for(1025, 4 * BLOCK, 256) == 2
