"""CPU: the cases and restatements of tests/index_cases.py, which tests/test_gpu_index_kernels.py holds the index kernels against
(``glam_csr_build``, ``glam_ell_build``, ``glam_batch_ptr``, ``glam_batch_fingerprint``).  Three things are established here, without a
GPU:

* the vectorised restatements ARE the plain per-edge / per-node / per-word loops (small cases), and the fingerprint's the scalar
  64-bit formula of ``k_fingerprint``;
* every case delivers what it exists for: the degrees, the scan block and chunk counts (1, 2, 256, 257), the trip counts of the
  capped grids (1, 2), both sides of the 32 / 33 sort switch, both ``by`` directions, both ELL outcomes on each side, both kinds of
  refusal;
* the cases discriminate: eleven wrong builders, each a small edit of a restatement, differ from it on a named case (every
  comparison of this family is exact, so "fails" means "is not equal")."""
import numpy as np
import pytest
import torch

from tests import index_cases as I


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------
# the restatements against naive loops
# ---------------------------------------------------------------------------------------------
def _csr_naive(edge_index, N, by):
    ei = edge_index.tolist()
    seg = [[] for _ in range(N)]
    for e in range(len(ei[0])):
        s, d = ei[0][e], ei[1][e]
        if not (0 <= s < N and 0 <= d < N):
            continue
        key, val = (d, s) if by == 0 else (s, d)
        seg[key].append((val, e))                       # appended in edge order: stable
    ptr, nbr, eid = [0], [], []
    for n in range(N):
        nbr += [v for v, _ in seg[n]]
        eid += [e for _, e in seg[n]]
        ptr.append(len(nbr))
    return np.array(ptr, np.int32), np.array(nbr, np.int32), np.array(eid, np.int32)


def _ell_naive(ptr, nbr, eid, N):
    en, ee, ovf = np.full((N, 4), -1, np.int32), np.full((N, 4), -1, np.int32), False
    for n in range(N):
        for k in range(ptr[n], ptr[n + 1]):
            if k - ptr[n] < 4:
                en[n, k - ptr[n]], ee[n, k - ptr[n]] = nbr[k], eid[k]
            else:
                ovf = True
    return en, ee, ovf


_SMALL = [n for n in I.GRAPH_CASES if n.startswith(("scan_edges", "segment_ladder", "one_node"))]


@pytest.mark.parametrize("by", [0, 1])
@pytest.mark.parametrize("name", _SMALL)
def test_csr_and_ell_ref_are_the_naive_loops(name, by):
    g = I.graph_case(name)
    ref = I.csr_ref(g.edge_index, g.N, by)
    assert all(a.dtype == np.int32 for a in ref)
    assert _same(ref, _csr_naive(g.edge_index, g.N, by))
    assert _same(I.ell_ref(*ref, g.N), _ell_naive(*ref, g.N))
    assert ref[0][-1] == g.E == ref[1].size == ref[2].size


@pytest.mark.parametrize("by", [0, 1])
@pytest.mark.parametrize("name", I.BAD_ID_CASES)
def test_csr_ref_drops_bad_edges_like_the_naive_loop(name, by):
    g = I.bad_ids()[name]
    ref = I.csr_ref(g.edge_index, g.N, by)
    assert _same(ref, _csr_naive(g.edge_index, g.N, by))
    assert ref[0][-1] == g.E - len(g.bad) and not set(ref[2].tolist()) & set(g.bad)
    # the valid subset, built on its own, is the same index up to the numbering of the edges
    keep = I.valid_edges(g.edge_index, g.N)
    sub = I.csr_ref(g.edge_index[:, torch.from_numpy(keep)], g.N, by)
    assert np.array_equal(sub[0], ref[0]) and np.array_equal(sub[1], ref[1])
    assert np.array_equal(np.flatnonzero(keep)[sub[2]], ref[2])


def test_ell_ref_on_the_large_cases_matches_the_loop_on_their_window():
    g = I.graph_case("second_chunk[524289,twin]")
    for by in (0, 1):
        ptr, nbr, eid = I.csr_ref(g.edge_index, g.N, by)
        en, ee, ovf = I.ell_ref(ptr, nbr, eid, g.N)
        assert ovf == (by == 0)
        deg = np.diff(ptr)
        assert (en[deg == 0] == -1).all() and not np.setdiff1d(np.flatnonzero(deg), g.window).size
        for n in g.window[::7].tolist() + [g.N - 1]:
            want = nbr[ptr[n]:ptr[n + 1]][:4].tolist()
            assert en[n].tolist() == want + [-1] * (4 - len(want))
            want = eid[ptr[n]:ptr[n + 1]][:4].tolist()
            assert ee[n].tolist() == want + [-1] * (4 - len(want))


def _batch_ptr_naive(batch, B):
    b = batch.tolist()
    if B is None:
        B = b[-1] + 1 if b else 0
    if B < 0 or any(not 0 <= x < B for x in b) or any(y < x for x, y in zip(b, b[1:])):
        return None
    return np.array([sum(1 for x in b if x < g) for g in range(B + 1)], np.int32)


@pytest.mark.parametrize("name", [n for n, (b, _, _) in I.BATCH_CASES.items() if b.size <= 300 and "5000" not in n])
def test_batch_ptr_ref_is_the_naive_loop(name):
    batch, B, valid = I.BATCH_CASES[name]
    got, want = I.batch_ptr_ref(batch, B), _batch_ptr_naive(batch, B)
    assert (got is None) == (want is None) == (not valid)
    if valid:
        assert got.dtype == np.int32 and np.array_equal(got, want)


def _mix_scalar(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & I.U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & I.U64
    return z ^ (z >> 31)


def _fingerprint_scalar(buffers, index=True, salt=True):
    """``k_fingerprint`` word by word in Python ints; ``index`` / ``salt`` = False: the two wrong kernels of the mutation test."""
    h = 0
    for t, buf in enumerate(buffers):
        s = (0x9E3779B97F4A7C15 * (t + 1)) & I.U64 if salt else 0
        for i, w in enumerate(buf.tolist()):
            h += _mix_scalar(((w << 32) | ((i & 0xFFFFFFFF) if index else 0)) ^ s ^ (i >> 32))
    return h & I.U64


@pytest.mark.parametrize("name", [n for n, bufs in I.FP_CASES.items() if sum(b.size for b in bufs) <= 1100])
def test_fingerprint_ref_is_the_scalar_formula(name):
    bufs = I.FP_CASES[name]
    assert I.fingerprint_ref(bufs) == _fingerprint_scalar(bufs)
    as_i32 = [b.view(np.int32) for b in bufs]                       # the GPU test hands int32 tensors over: the same bits
    assert I.fingerprint_ref(as_i32) == I.fingerprint_ref(bufs)


def test_fingerprint_ref_known_values():
    """Anchors that do not come from this file's own arithmetic: splitmix64's published first outputs (seed 0: the finaliser applied to
    the golden-ratio increment and to twice it)."""
    z = np.array([0x9E3779B97F4A7C15, (2 * 0x9E3779B97F4A7C15) & I.U64], dtype=np.uint64)
    with np.errstate(over="ignore"):
        assert [int(v) for v in I.fp_mix(z)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    assert _mix_scalar(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    # one zero word at index 0 of buffer 0: mix(salt_0) = that first output
    assert I.fingerprint_ref([np.zeros(1, np.uint32)]) == 0xE220A8397B1DCDAF
    assert I.fingerprint_ref([np.zeros(0, np.uint32)]) == 0


# ---------------------------------------------------------------------------------------------
# the cases deliver
# ---------------------------------------------------------------------------------------------
def test_every_graph_case_builds_and_asserts_itself():
    for name in I.GRAPH_CASES:
        g = I.graph_case(name)
        assert g.name == name and g.edge_index.dtype == torch.int64 and g.edge_index.is_contiguous()
        din, dout = I.degrees(g.edge_index, g.N)
        assert max(din.max(initial=0), dout.max(initial=0)) <= I.MAX_SEGMENT
        assert I.valid_edges(g.edge_index, g.N).all()


def test_scan_block_and_chunk_counts_are_each_reached_by_a_named_case():
    blocks = {name: I.scan_blocks(I.graph_case(name).N) for name in I.GRAPH_CASES}
    assert blocks["scan_edges[2047]"] == 1 and blocks["scan_edges[2048]"] == 2 and blocks["scan_edges[4096]"] == 3
    assert blocks["second_chunk[524287]"] == 256 and blocks["second_chunk[524288]"] == 257 == blocks["second_chunk[524289]"]
    assert {1, 2, 256, 257} <= set(blocks.values())
    chunks = {name: I.scan_top_chunks(I.graph_case(name).N) for name in I.GRAPH_CASES}
    assert chunks["second_chunk[524287]"] == 1 and chunks["second_chunk[524288]"] == 2 and set(chunks.values()) == {1, 2}
    # rowptr[N] as the LAST item of a scan block, as the FIRST (alone in its block) and in between; alone in its thread's 8 too
    pos = {N: (N % I.SCAN_ITEMS, N % I.SCAN_THREAD_ITEMS) for N in I.SCAN_EDGE_N + I.SECOND_CHUNK_N}
    assert pos[2047] == (2047, 7) and pos[2048] == (0, 0) and pos[4096] == (0, 0) and pos[8] == (8, 0) and pos[7] == (7, 7)
    assert pos[524287][0] == 2047 and pos[524288][0] == 0 and pos[524289][0] == 1
    # the carry of the second chunk is not zero, and rowptr moves behind it
    for N in (524288, 524289):
        for by in (0, 1):
            ptr = I.csr_ref(I.graph_case(f"second_chunk[{N}]").edge_index, N, by)[0]
            assert ptr[256 * I.SCAN_ITEMS] > 0 and ptr[N] > ptr[256 * I.SCAN_ITEMS - 1]


def test_trip_counts_of_the_capped_grids_are_each_reached_by_a_named_case():
    g = I.graph_case("many_edges")
    assert g.E > 524288 and I.trips(g.E) == 2                                    # k_csr_count, k_csr_fill
    assert I.trips(I.graph_case("segment_ladder[shuffled]").E) == 1
    assert [I.trips(N) for N in I.SECOND_CHUNK_N] == [1, 1, 2]                    # k_csr_sort_segments, k_ell_build (per node)
    assert I.graph_case("second_chunk[524289]").window[-1] == 524288              # ... and the node of the second trip holds edges
    sizes = {name: b.size for name, (b, _, _) in I.BATCH_CASES.items()}
    assert I.trips(sizes["N524289"] + 1) == 2 and I.trips(sizes["N257_empties"] + 1) == 1      # k_batch_ptr (per n in 0..N)
    assert I.grid_for(sizes["N255_empties"] + 1) == 1 and I.grid_for(sizes["N256_empties"] + 1) == 2
    # the fingerprint's grid: ceil(total / 1024) blocks up to 256, then strided trips
    grids = {t: I.grid_for(t, 4 * I.BLOCK, 256) for t in I.FP_TOTALS}
    assert [grids[t] for t in (1, 1024, 1025, 262144, 262145, 300001)] == [1, 1, 2, 256, 256, 256]
    longest = max(b.size for b in I.FP_CASES["total_300001_in_2"])
    assert -(-longest // (256 * I.BLOCK)) == 5 and -(-262145 // (256 * I.BLOCK)) == 5 and 262144 // (256 * I.BLOCK) == 4


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("order", I.LADDER_ORDERS)
def test_segment_ladder_delivers(order, flip):
    g = I.graph_case(f"segment_ladder[{order}{',flip' if flip else ''}]")
    by = int(flip)
    ptr, nbr, eid = I.csr_ref(g.edge_index, g.N, by)
    deg = np.diff(ptr)
    assert g.by == by and tuple(deg[1:1 + len(I.LADDER)]) == I.LADDER == (0, 1, 2, 31, 32, 33, 64, 257, 1000)
    assert deg[0] == 0 and deg[-1] == 0
    assert sorted(set(deg.tolist())) == sorted(set(I.LADDER))                  # both sides of the switch at 32 / 33, and nothing else
    seg = lambda n: slice(ptr[n], ptr[n + 1])
    assert nbr[seg(g.loop_only)].tolist() == [g.loop_only]                      # a self-loop that is the node's only edge
    tied = eid[seg(g.tie)][nbr[seg(g.tie)] == g.tie_src]
    assert tied.size == 3 and (np.diff(tied) > 0).all()                         # holds a tie; the three keep eid order
    assert deg[g.tie] == 33                                                     # ... in the shortest heap-sorted segment
    key = g.edge_index.numpy()[1 - by]
    if order == "ascending":
        assert (np.diff(key) >= 0).all() and np.array_equal(eid, np.arange(g.E))
    elif order == "descending":
        assert (np.diff(key) <= 0).all()
    else:
        assert (np.diff(key) < 0).any() and (np.diff(key) > 0).any()
    assert all((np.diff(eid[seg(n)]) > 0).all() for n in range(g.N))           # stable: eid ascending inside every segment


def test_scan_edges_deliver():
    for N in I.SCAN_EDGE_N:
        g = I.graph_case(f"scan_edges[{N}]")
        assert g.marks == sorted(m for m in {0, 7, 8, 2047, 2048, 4095, 4096, N - 1} if 0 <= m < N)
        for by in (0, 1):
            deg = np.diff(I.csr_ref(g.edge_index, N, by)[0])
            assert sorted(np.flatnonzero(deg)) == g.marks
    assert I.graph_case("scan_edges[0]").E == 0 and I.graph_case("scan_edges[0]").edge_index.shape == (2, 0)


def test_both_ell_outcomes_on_each_side():
    def forms(name):
        g = I.graph_case(name)
        return tuple(not I.ell_ref(*I.csr_ref(g.edge_index, g.N, by), g.N)[2] for by in (0, 1))        # (ell exists, ell_t exists)
    assert forms("second_chunk[524288]") == (True, True)
    for N in I.SECOND_CHUNK_N:
        assert forms(f"second_chunk[{N},twin]") == (False, True)                 # in-degree 5 on the last node only
    assert forms("segment_ladder[shuffled]")[0] is False and forms("segment_ladder[shuffled,flip]")[1] is False
    assert forms("scan_edges[9]") == (True, True) and forms("one_node") == (False, False) and forms("many_edges") == (False, False)
    g = I.graph_case("second_chunk[524289,twin]")
    din, dout = I.degrees(g.edge_index, g.N)
    assert din[-1] == 5 and (din[:-1] <= 4).all() and dout.max() <= 4 and g.edge_index[:, -1].tolist() == [g.extra_src, g.N - 1]
    assert torch.equal(g.edge_index[:, :-1], I.graph_case("second_chunk[524289]").edge_index)


def test_both_kinds_of_refusal_have_cases():
    invalid = [n for n, (_, _, valid) in I.BATCH_CASES.items() if not valid]
    assert {"decreasing_first", "decreasing_middle", "decreasing_last", "negative_middle", "id_equal_B", "negative_first"} <= set(invalid)
    for n in invalid:
        assert I.batch_ptr_ref(*I.BATCH_CASES[n][:2]) is None, n                # "is invalid": the exception
    assert set(I.bad_ids()) == set(I.BAD_ID_CASES)
    for g in I.bad_ids().values():
        assert not I.valid_edges(g.edge_index, g.N).all()
    assert I.bad_ids()["first_edge"].bad == [0] and I.bad_ids()["last_edge"].bad == [23]
    # the error code: byte counts no multiple of 4 and buffer counts outside 1..4 never reach a restatement
    for n in (0, 5):
        with pytest.raises(AssertionError):
            I.fingerprint_ref([np.zeros(1, np.uint32)] * n)


def test_batch_cases_deliver():
    c = I.BATCH_CASES
    for N in (255, 256, 257):
        ptr = I.batch_ptr_ref(*c[f"N{N}_empties"][:2])
        assert ptr.tolist() == [0, 0, 0, 3, 3, 4, N - 7, N - 7, N - 7, N - 7, N, N, N] and ptr.size == 13
        assert I.batch_ptr_ref(*c[f"N{N}_inferred"][:2]).tolist() == ptr[:11].tolist()
    assert I.batch_ptr_ref(*c["N0_B0"][:2]).tolist() == [0] and I.batch_ptr_ref(*c["N0_B3"][:2]).tolist() == [0, 0, 0, 0]
    assert I.batch_ptr_ref(*c["N0_inferred"][:2]).tolist() == [0]
    assert I.batch_ptr_ref(*c["all_in_last_of_5000"][:2]).tolist() == [0] * 5000 + [300]
    assert I.batch_ptr_ref(*c["all_in_last_of_5000_inferred"][:2]).size == 5001
    assert I.batch_ptr_ref(*c["all_in_first_of_5000"][:2]).tolist() == [0] + [300] * 5000
    big = I.batch_ptr_ref(*c["N524289"][:2])
    sizes = np.diff(big)
    assert big[-1] == 524289 and big.size == 26001 and (sizes[:3] == 0).all() and (sizes[-2:] == 0).all() and (sizes[3:-3] == 0).any()


def test_fingerprint_cases_deliver():
    c = I.FP_CASES
    assert sorted({sum(b.size for b in bufs) for n, bufs in c.items() if n.startswith("total_")}) == sorted(I.FP_TOTALS)
    assert [[b.size for b in c[f"empty_at_{p}"]].index(0) for p in range(4)] == [0, 1, 2, 3]
    assert len({I.fingerprint_ref(c[f"empty_at_{p}"]) for p in range(4)}) == 4      # the salts behind the empty buffer move
    words = np.concatenate([b for bufs in c.values() for b in bufs])
    assert (words == 0).any() and (words == 0xFFFFFFFF).any()
    assert not c["zeros_1000"][0].any() and (c["ones_1000"][0] == 0xFFFFFFFF).all() and np.unique(c["repeated_1000"][0]).size == 3
    # all-equal words still hash by position: 1 000 zeros are not 999 zeros, nor 1 000 times one term
    assert I.fingerprint_ref(c["zeros_1000"]) != I.fingerprint_ref([c["zeros_1000"][0][:999]])


# ---------------------------------------------------------------------------------------------
# the cases discriminate: wrong builders as small edits of the restatements
# ---------------------------------------------------------------------------------------------
_ARRIVAL_33 = np.random.default_rng(33).permutation(33)        # "arrival order" of an unsorted segment: a fixed permutation


def _segments(ptr):
    return [slice(int(a), int(b)) for a, b in zip(ptr[:-1], ptr[1:])]


def _csr_segments_reversed(ei, N, by):
    ptr, nbr, eid = I.csr_ref(ei, N, by)
    for s in _segments(ptr):
        nbr[s], eid[s] = nbr[s][::-1].copy(), eid[s][::-1].copy()
    return ptr, nbr, eid


def _csr_length_33_unsorted(ei, N, by):
    ptr, nbr, eid = I.csr_ref(ei, N, by)
    for s in _segments(ptr):
        if s.stop - s.start == 33:
            nbr[s], eid[s] = nbr[s][_ARRIVAL_33], eid[s][_ARRIVAL_33]
    return ptr, nbr, eid


def _csr_second_chunk_carry_dropped(ei, N, by):
    ptr, nbr, eid = I.csr_ref(ei, N, by)
    first = 256 * I.SCAN_ITEMS                            # first item of scan block 256: its offset restarts at 0
    if N + 1 > first:
        ptr[first:] -= ptr[first]
    return ptr, nbr, eid


def _csr_last_ptr_unwritten_at_block_multiples(ei, N, by):
    ptr, nbr, eid = I.csr_ref(ei, N, by)
    if N % I.SCAN_ITEMS == 0:                             # a scan grid of ceil(N / 2048) blocks: nobody owns item N
        ptr[N] = -1
    return ptr, nbr, eid


def _csr_invalid_counted_not_filled(ei, N, by):
    ptr, nbr, eid = I.csr_ref(ei, N, by)
    key = ei.numpy()[1 - by]
    key = key[(key >= 0) & (key < N)]                     # count checks the key alone, fill checks both rows
    full = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=N), out=full[1:])
    return full.astype(np.int32), nbr, eid


def _csr_duplicates_merged(ei, N, by):
    e = ei.numpy()
    _, first = np.unique(e.T, axis=0, return_index=True) if e.shape[1] else (None, np.zeros(0, np.int64))
    keep = np.sort(first)
    ptr, nbr, eid = I.csr_ref(torch.from_numpy(np.ascontiguousarray(e[:, keep])), N, by)
    return ptr, nbr, keep[eid].astype(np.int32)


def _ell_fifth_kept_no_flag(ptr, nbr, eid, N):
    en, ee, _ = I.ell_ref(ptr, nbr, eid, N)
    for n in np.flatnonzero(np.diff(ptr) > 4):
        for k in range(4, int(ptr[n + 1] - ptr[n])):
            en[n, k % 4], ee[n, k % 4] = nbr[ptr[n] + k], eid[ptr[n] + k]
    return en, ee, False


def _ell_free_slots_zero(ptr, nbr, eid, N):
    en, ee, ovf = I.ell_ref(ptr, nbr, eid, N)
    free = en < 0
    return np.where(free, 0, en), np.where(free, 0, ee), ovf


def _csr_case(name):
    g = I.bad_ids()[name[8:-1]] if name.startswith("bad_ids[") else I.graph_case(name)
    return g.edge_index, g.N


# wrong builder -> the cases that must catch it (on at least one ``by``) and cases that do not hold its edge and so must let it pass
_CSR_MUTATIONS = [
    (_csr_segments_reversed, ["segment_ladder[shuffled]", "segment_ladder[ascending,flip]", "one_node", "scan_edges[9]"], ["scan_edges[0]"]),
    (_csr_length_33_unsorted, [f"segment_ladder[{o}{f}]" for o in I.LADDER_ORDERS for f in ("", ",flip")], ["many_edges", "one_node", "scan_edges[4096]"]),
    (_csr_second_chunk_carry_dropped, ["second_chunk[524288]", "second_chunk[524289]", "second_chunk[524289,twin]"], ["second_chunk[524287]", "many_edges"]),
    (_csr_last_ptr_unwritten_at_block_multiples, ["scan_edges[2048]", "scan_edges[4096]", "second_chunk[524288]"], ["scan_edges[2047]", "scan_edges[2049]", "second_chunk[524287]"]),
    (_csr_invalid_counted_not_filled, ["bad_ids[value_row_only]", "bad_ids[value_row_only_negative]", "bad_ids[several]"], ["segment_ladder[shuffled]"]),
    (_csr_duplicates_merged, ["segment_ladder[shuffled]", "segment_ladder[descending,flip]", "one_node", "scan_edges[9]", "many_edges"], ["second_chunk[524289]"]),
]


@pytest.mark.parametrize("wrong,catchers,blind", _CSR_MUTATIONS, ids=[m[0].__name__.strip("_") for m in _CSR_MUTATIONS])
def test_cases_catch_the_wrong_csr_builder(wrong, catchers, blind):
    for name in catchers:
        ei, N = _csr_case(name)
        differs = [not _same(wrong(ei, N, by), I.csr_ref(ei, N, by)) for by in (0, 1)]
        assert any(differs), f"{wrong.__name__}: case {name} lets it pass"
        if name.startswith("segment_ladder") and wrong in (_csr_length_33_unsorted,):
            assert differs == [",flip" not in name, ",flip" in name]              # the side the ladder is on
    for name in blind:
        ei, N = _csr_case(name)
        assert all(_same(wrong(ei, N, by), I.csr_ref(ei, N, by)) for by in (0, 1)), f"{wrong.__name__}: expected unseen on {name}"


def test_value_row_only_bad_id_is_what_catches_count_without_fill():
    """A bad id on the KEY row is refused by any count; only a valid key next to a bad value separates count from fill — in the
    direction in which that row is the value row."""
    g = I.bad_ids()["value_row_only"]
    assert not _same(_csr_invalid_counted_not_filled(g.edge_index, g.N, 0), I.csr_ref(g.edge_index, g.N, 0))
    g = I.bad_ids()["id_equal_N_on_key_row"]
    assert _same(_csr_invalid_counted_not_filled(g.edge_index, g.N, 0), I.csr_ref(g.edge_index, g.N, 0))
    assert not _same(_csr_invalid_counted_not_filled(g.edge_index, g.N, 1), I.csr_ref(g.edge_index, g.N, 1))


_ELL_MUTATIONS = [
    (_ell_fifth_kept_no_flag, [("second_chunk[524289,twin]", 0), ("second_chunk[524287,twin]", 0), ("segment_ladder[shuffled,flip]", 1)],
     [("second_chunk[524289,twin]", 1), ("second_chunk[524289]", 0)]),
    (_ell_free_slots_zero, [("second_chunk[524288]", 0), ("second_chunk[524288]", 1), ("scan_edges[9]", 0), ("scan_edges[1]", 1)], []),
]


@pytest.mark.parametrize("wrong,catchers,blind", _ELL_MUTATIONS, ids=[m[0].__name__.strip("_") for m in _ELL_MUTATIONS])
def test_cases_catch_the_wrong_ell_builder(wrong, catchers, blind):
    for name, by in catchers:
        g = I.graph_case(name)
        csr = I.csr_ref(g.edge_index, g.N, by)
        got, ref = wrong(*csr, g.N), I.ell_ref(*csr, g.N)
        assert not _same(got, ref), f"{wrong.__name__}: case {name} (by = {by}) lets it pass"
        if wrong is _ell_fifth_kept_no_flag:
            assert ref[2] and not got[2] and not np.array_equal(got[0], ref[0])     # flag AND records differ
    for name, by in blind:
        g = I.graph_case(name)
        csr = I.csr_ref(g.edge_index, g.N, by)
        assert _same(wrong(*csr, g.N), I.ell_ref(*csr, g.N))


def _batch_ptr_trailing_empties_unfilled(batch, B=None):
    ptr = I.batch_ptr_ref(batch, B)
    if ptr is not None and ptr.size > 1:
        last = int(batch[-1]) if batch.size else -1       # the thread of n = N writes ptr[B] only
        ptr[last + 1:-1] = -1
    return ptr


def test_cases_catch_batch_ptr_without_the_trailing_fill():
    wrong = _batch_ptr_trailing_empties_unfilled
    for name in ("N255_empties", "N256_empties", "N257_empties", "N0_B3", "all_in_first_of_5000", "N524289"):
        batch, B, _ = I.BATCH_CASES[name]
        assert not np.array_equal(wrong(batch, B), I.batch_ptr_ref(batch, B)), name
    for name in ("N255_inferred", "all_in_last_of_5000", "N1_inferred_id4", "N0_B0"):      # no empty graph behind the last node
        batch, B, _ = I.BATCH_CASES[name]
        assert np.array_equal(wrong(batch, B), I.batch_ptr_ref(batch, B)), name


def swap_words(bufs, t, i, j):
    out = [b.copy() for b in bufs]
    out[t][[i, j]] = out[t][[j, i]]
    return out


def move_boundary(bufs, t):
    """The last word of buffer ``t`` becomes the first of buffer ``t + 1``: the same words in the same order."""
    out = [b.copy() for b in bufs]
    out[t], out[t + 1] = bufs[t][:-1].copy(), np.concatenate([bufs[t][-1:], bufs[t + 1]])
    return out


def test_cases_catch_a_fingerprint_without_index_or_salt():
    bufs = I.FP_CASES["total_257_in_4"]
    assert bufs[1][3] != bufs[1][40]
    swapped, moved = swap_words(bufs, 1, 3, 40), move_boundary(bufs, 0)
    assert np.array_equal(np.concatenate(moved), np.concatenate(bufs)) and moved[0].size == bufs[0].size - 1
    ref = I.fingerprint_ref(bufs)
    assert I.fingerprint_ref(swapped) != ref and I.fingerprint_ref(moved) != ref
    # without the word index a swap goes unnoticed (and only then); the boundary move is still seen through the salt
    no_index = lambda b: _fingerprint_scalar(b, index=False)
    assert no_index(bufs) != ref and no_index(swapped) == no_index(bufs) and no_index(moved) != no_index(bufs)
    # without the buffer salt, moving the LAST word of a buffer to the front of the next one changes indices: still seen; what goes
    # unnoticed is a boundary moved across words that keep their index — buffer t + 1 empty before, or the words re-dealt at equal index
    no_salt = lambda b: _fingerprint_scalar(b, salt=False)
    assert no_salt(bufs) != ref
    a, b = bufs[0], bufs[1][:bufs[0].size]
    dealt, redealt = [a, b], [b, a]                                                # the same (index, word) pairs, other buffers
    assert not np.array_equal(a, b) and no_salt(dealt) == no_salt(redealt) and I.fingerprint_ref(dealt) != I.fingerprint_ref(redealt)
    for p in range(3):                                                             # an empty buffer moved one place: only the salt tells
        x, y = I.FP_CASES[f"empty_at_{p}"], I.FP_CASES[f"empty_at_{p + 1}"]
        assert no_salt(x) == no_salt(y) and I.fingerprint_ref(x) != I.fingerprint_ref(y)
    tail = [bufs[0], np.zeros(0, np.uint32)]
    grown = [bufs[0][:-1], bufs[0][-1:]]                                           # boundary moved by one word into an empty buffer
    assert I.fingerprint_ref(tail) != I.fingerprint_ref(grown)
