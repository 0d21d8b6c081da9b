"""CPU: the host side of the screening hit lists (``glam_amd.hits.HitList`` / ``ArchitectureDTI.screen_top`` over ``glam_hits_*``) — the
C prototypes against their ctypes rows, the entry points' argument checks by status code, what ``HitList.update`` settles on the host
before a launch (``hits.update_plan``) and its refusals, ``screen_top``'s refusals — and the restatement the GPU tests compare against
(``tests/hits_restated.py``), checked here against a brute-force sort written from the words of the order."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from glam_amd import _lib, hits, model
from glam_amd._lib import GlamHipError
from tests import hits_restated as R
from tests.test_host_logic import _header_prototypes, _table_type
from tests.test_panel_host import _KW, _fake_encoding

_INTS = ("glam_hits_supported", "glam_hits_reset", "glam_hits_merge")


def test_hits_prototypes_match_their_signature_rows():
    """Header and ``SIGNATURES`` type for type; STATUS returns that ``api()`` checks; the ABI version stays 4."""
    protos = _header_prototypes()
    for name in _INTS + ("glam_hits_workspace_bytes",):
        res, args = _lib.SIGNATURES[name]
        assert (_table_type(res), [_table_type(a) for a in args]) == protos[name], name
    p, i64, i32, sz = "pointer", ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    assert protos["glam_hits_supported"] == (i32, [i32])
    assert protos["glam_hits_workspace_bytes"] == (sz, [i64, i64, i32])
    assert protos["glam_hits_reset"] == (i32, [p, p, p, i64, i32, p])
    assert protos["glam_hits_merge"] == (i32, [p, i64, i64, p, i64, i64, i32, i32, i32, p, p, p, p, sz, p])
    assert _lib.ABI_VERSION == 4
    for name in _INTS:
        assert name not in _lib.VALUE_RETURNS
        assert getattr(_lib.api(), name).errcheck is not None and getattr(_lib.load(), name).errcheck is None


def test_hits_queries():
    lib = _lib.load()
    assert [lib.glam_hits_supported(K) for K in (1, 64, 1024)] == [0] * 3                               # GLAM_OK
    assert [lib.glam_hits_supported(K) for K in (0, -1, 1025)] == [_lib.GLAM_E_UNSUPPORTED] * 3
    with pytest.raises(GlamHipError, match="K=1025 not in 1..1024"):
        _lib.api().glam_hits_supported(1025)
    ws = lib.glam_hits_workspace_bytes

    def expect(L, Qs, K):                    # per (column, slab) K keys of 8 bytes, K scores of 4, one count; at most min(64, L // 64) slabs
        lists = Qs * max(1, min(64, L // 64))
        return lists * K * 8 + (lists * K * 4 + 7) // 8 * 8 + (lists * 4 + 7) // 8 * 8
    for L, Qs, K in [(1, 1, 1), (63, 3, 5), (64, 1, 65), (1000, 17, 64), (4097, 3, 1024), (1 << 20, 15, 100)]:
        assert ws(L, Qs, K) == expect(L, Qs, K), (L, Qs, K)
    assert ws(0, 3, 5) == 0 and ws(7, 0, 5) == 0 and ws(7, 3, 0) == 0 and ws(-1, 3, 5) == 0 and ws(7, -3, 5) == 0 and ws(7, 3, -5) == 0
    assert ws(1 << 30, 1 << 30, 1024) == expect(1 << 30, 1 << 30, 1024) > 1 << 40                       # (a size_t product, not an int one)


def test_hits_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)                                                # (never dereferenced: each call fails a check first)

    def merge(score=fake, ld_row=3, ld_col=1, ids=None, L=100, Qs=3, K=10, largest=1, slabs=0, ts=fake, ti=fake, seen=fake, ws=fake,
              wsb=1 << 20):
        return lib.glam_hits_merge(score, ld_row, ld_col, ids, L, Qs, K, largest, slabs, ts, ti, seen, ws, wsb, None)
    nothing = dict(score=None, ts=None, ti=None, seen=None, ws=None, wsb=0)
    assert merge(L=0, **nothing) == 0 and merge(Qs=0, **nothing) == 0           # nothing to do, nothing dereferenced
    for K in (0, -1, 1025):
        assert merge(K=K) == _lib.GLAM_E_UNSUPPORTED
        assert merge(K=K, **nothing) == _lib.GLAM_E_UNSUPPORTED                 # ... before the pointers are looked at
        assert merge(K=K, L=0, **nothing) == _lib.GLAM_E_UNSUPPORTED
    for bad in (dict(L=-1), dict(Qs=-1), dict(L=2 ** 31), dict(L=2 ** 40), dict(ld_row=-1), dict(ld_col=-3), dict(slabs=-1),
                dict(ld_row=2 ** 62)):
        assert merge(**bad) == _lib.GLAM_E_INVALID, bad
    for name in ("score", "ts", "ti", "seen", "ws"):
        assert merge(**{name: None}) == _lib.GLAM_E_INVALID, name
    for name in ("score", "ids", "ts", "ti"):
        assert merge(**{name: ctypes.c_void_p(4098)}) == _lib.GLAM_E_INVALID, name                     # not a dword boundary
    assert merge(seen=ctypes.c_void_p(4100)) == _lib.GLAM_E_INVALID and merge(ws=ctypes.c_void_p(4100)) == _lib.GLAM_E_INVALID
    assert merge(wsb=lib.glam_hits_workspace_bytes(100, 3, 10) - 1) == _lib.GLAM_E_INVALID             # one byte short
    with pytest.raises(GlamHipError, match="glam_hits_merge"):
        _lib.api().glam_hits_merge(None, 1, 1, None, 4, 2, 10, 1, 0, None, None, None, None, 0, None)

    def reset(ts=fake, ti=fake, seen=fake, Qs=3, K=10):
        return lib.glam_hits_reset(ts, ti, seen, Qs, K, None)
    for K in (0, 1025):
        assert reset(K=K) == _lib.GLAM_E_UNSUPPORTED and reset(None, None, None, K=K) == _lib.GLAM_E_UNSUPPORTED
    assert reset(Qs=-1) == _lib.GLAM_E_INVALID
    for bad in (dict(ts=None), dict(ti=None), dict(seen=None), dict(ts=ctypes.c_void_p(4098)), dict(seen=ctypes.c_void_p(4100))):
        assert reset(**bad) == _lib.GLAM_E_INVALID, bad


def test_update_plan_reads_every_layout_by_stride():
    t = torch.zeros(6, 3, 2)
    assert hits.update_plan(t, None, 1, 3, 0) == (6, 1, 6, 2, None)                               # [L, Qs, out_dim], task 1
    assert hits.update_plan(t[:, :, 1], None, 0, 3, 0) == (6, 0, 6, 2, None)                      # a [L, Qs] view of the same column
    assert hits.update_plan(t[:, :, 0].t().contiguous().t(), None, 0, 3, 0) == (6, 0, 1, 6, None)   # query-major memory
    assert hits.update_plan(t[::2], None, 0, 3, 5) == (3, 0, 12, 2, None)
    one = torch.zeros(6, 4)
    assert hits.update_plan(one, None, 3, 1, 0) == (6, 3, 4, 0, None)                             # one query: [L, out_dim] ...
    assert hits.update_plan(one[:, 2], None, 0, 1, 0) == (6, 0, 4, 0, None)                       # ... [L]
    assert hits.update_plan(one[:, :1], None, 0, 1, 0) == (6, 0, 4, 0, None)                      # ... [L, 1]
    assert hits.update_plan(one.view(6, 1, 4), None, 2, 1, 0) == (6, 2, 4, 4, None)               # ... [L, 1, out_dim]
    assert hits.update_plan(torch.zeros(0, 3), None, 0, 3, 7)[0] == 0
    L, _, _, _, ids = hits.update_plan(t, torch.tensor([5, 4, 2 ** 31 - 1, 0, 1, 1]), 0, 3, 0)     # (ids are not deduplicated)
    assert ids.dtype == np.int32 and ids.tolist() == [5, 4, 2 ** 31 - 1, 0, 1, 1]
    dev_ids = torch.zeros(6, dtype=torch.int32, device="meta")
    assert hits.update_plan(t, dev_ids, 0, 3, 0)[4] is dev_ids                                    # a device vector: by dtype and shape


def test_update_plan_refusals_name_the_argument():
    t = torch.zeros(6, 3, 2)
    for bad in (t.double(), t.half(), t.long(), [[0.0] * 3] * 6, np.zeros((6, 3), dtype=np.float32)):
        with pytest.raises(GlamHipError, match="scores must be a float32 tensor"):
            hits.update_plan(bad, None, 0, 3, 0)
    for bad, q in ((t, 2), (t[:, 0], 3), (t[:, 0, 0], 3), (torch.zeros(6, 1, 3, 2), 1), (torch.zeros(()), 1), (torch.zeros(6, 2, 2), 1)):
        with pytest.raises(GlamHipError, match=r"scores must be \[L, "):
            hits.update_plan(bad, None, 0, q, 0)
    for task in (2, -1):
        with pytest.raises(GlamHipError, match="task = .* outside the 2 task column"):
            hits.update_plan(t, None, task, 3, 0)
    with pytest.raises(GlamHipError, match="task = 1 is outside the 1 task column"):
        hits.update_plan(t[:, :, 0], None, 1, 3, 0)
    with pytest.raises(GlamHipError, match="task must be an integer"):
        hits.update_plan(t, None, 0.0, 3, 0)
    with pytest.raises(IndexError, match="ids must hold integers"):
        hits.update_plan(t, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0], 0, 3, 0)
    with pytest.raises(IndexError, match=r"ids must lie in \[0, 2147483648\)"):
        hits.update_plan(t, [0, 1, -2, 3, 4, 5], 0, 3, 0)
    with pytest.raises(IndexError, match=r"ids must lie in \[0, 2147483648\)"):
        hits.update_plan(t, np.asarray([0, 1, 2, 3, 4, 2 ** 31]), 0, 3, 0)
    with pytest.raises(IndexError, match="ids must have one entry per candidate"):
        hits.update_plan(t, [0, 1, 2], 0, 3, 0)
    with pytest.raises(IndexError, match="ids must have one entry per candidate"):
        hits.update_plan(t, [[0, 1, 2, 3, 4, 5]], 0, 3, 0)
    for bad in (torch.zeros(6, dtype=torch.int64, device="meta"), torch.zeros(5, dtype=torch.int32, device="meta"),
                torch.zeros(12, dtype=torch.int32, device="meta")[::2]):
        with pytest.raises(GlamHipError, match="device ids must be a contiguous int32"):
            hits.update_plan(t, bad, 0, 3, 0)
    # default ids: the last one must not pass 2^31 - 1
    assert hits.update_plan(t, None, 0, 3, 2 ** 31 - 6)[0] == 6
    with pytest.raises(GlamHipError, match="default ids past 2\\^31 - 1"):
        hits.update_plan(t, None, 0, 3, 2 ** 31 - 5)
    assert hits.update_plan(t, [0, 1, 2, 3, 4, 5], 0, 3, 2 ** 40)[0] == 6                          # ids of the caller's own: no such bound


def test_hit_list_refusals_that_need_no_device():
    for k in (0, -1, 1025):
        with pytest.raises(GlamHipError, match="outside the kernels' lists"):
            hits.HitList(3, k, "cpu")
    for k in (10.0, "10", True, None):
        with pytest.raises(GlamHipError, match="k must be an integer"):
            hits.HitList(3, k, "cpu")
    for q in (-1, 2.0, None):
        with pytest.raises(GlamHipError, match="queries must be a non-negative integer"):
            hits.HitList(q, 10, "cpu")
    with pytest.raises(GlamHipError, match="no CPU fallback"):
        hits.HitList(3, 10, "cpu")
    with pytest.raises(GlamHipError, match="no CPU fallback"):
        hits.HitList(3, 10, torch.device("meta"))
    # update on a CPU tensor: the shape passes, the device does not (a list without a device, as update finds its fields)
    top = hits.HitList.__new__(hits.HitList)
    top.queries, top.k, top.offered, top.scores = 3, 10, 0, torch.zeros(3, 10)
    with pytest.raises(GlamHipError, match="CPU tensor"):
        top.update(torch.zeros(6, 3))
    with pytest.raises(GlamHipError, match=r"scores must be \[L, 3\]"):
        top.update(torch.zeros(6, 4))
    assert top.offered == 0


def test_screen_top_refusals_that_need_no_device():
    net = model.ArchitectureDTI(**_KW, out_dim=2)
    enc = _fake_encoding(net)
    for k in (0, 1025):
        with pytest.raises(GlamHipError, match="screen_top: k = .* outside the kernels' lists"):
            net.screen_top([None], enc, k=k)
    with pytest.raises(GlamHipError, match="screen_top: k must be an integer"):
        net.screen_top([None], enc, k=10.5)
    for task in (2, -1, 1.0, None):
        with pytest.raises(GlamHipError, match="screen_top: task = .* not one of the model's 2 task"):
            net.screen_top([None], enc, task=task)
    # screen_panel's own refusals, with its own messages — from the first batch, and from an empty stream
    for stream in ([None], []):
        with torch.no_grad(), pytest.raises(GlamHipError, match="screen_panel: the model is in training mode"):
            net.screen_top(stream, enc)
    net.eval()
    for stream in ([None], [(None, [0, 1])], []):
        with pytest.raises(GlamHipError, match="screen_panel is inference only.*no_grad"):
            net.screen_top(stream, enc)
        with torch.no_grad():
            with pytest.raises(GlamHipError, match="screen_panel: .*another model"):
                model.ArchitectureDTI(**_KW, out_dim=2).eval().screen_top(stream, enc)
            with pytest.raises(IndexError, match=r"proteins must lie in \[0, 3\)"):
                net.screen_top(stream, enc, [0, 3])
    with torch.no_grad():
        next(net.pro_conv.parameters()).add_(1)
        for stream in ([None], []):
            with pytest.raises(GlamHipError, match="screen_panel: the encoding is stale"):
                net.screen_top(stream, enc)


# ---------------------------------------------------------------------------------------------
# the restatement against a sort written from the words of the order
# ---------------------------------------------------------------------------------------------
def _before(a, b, largest):
    """Whether candidate ``a = (score, id)`` comes before ``b``: the order, word by word."""
    (sa, ia), (sb, ib) = a, b
    if math.isnan(sa) != math.isnan(sb):
        return math.isnan(sb)                                     # NaN after every number
    if not math.isnan(sa) and sa != sb:                           # (-0.0 == +0.0 in Python as in IEEE)
        return sa > sb if largest else sa < sb
    return ia < ib                                                # equal scores, and NaN among themselves: ascending id


def _brute(scores, ids, largest, rule=_before):
    cand = [(float(s), int(i), n) for n, (s, i) in enumerate(zip(scores, ids))]
    cmp = lambda a, b: -1 if rule(a[:2], b[:2], largest) else (1 if rule(b[:2], a[:2], largest) else 0)      # noqa: E731
    return [c[2] for c in sorted(cand, key=functools.cmp_to_key(cmp))]


def _cases():
    rng = np.random.default_rng(5)
    ids = rng.permutation(400).astype(np.int64)
    near = (2 ** 31 - 1 - rng.permutation(400)).astype(np.int64)                # ids up to 2^31 - 1
    yield "special", R.special_scores(400, rng), ids
    yield "special, ids near 2^31", R.special_scores(400, rng), near
    yield "all equal", np.full(400, 1.5, dtype=np.float32), near
    yield "all NaN", np.full(400, np.nan, dtype=np.float32), ids
    yield "zeros of both signs", np.where(rng.integers(0, 2, 400) == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32), ids
    yield "denormals", (rng.integers(0, 8, 400).astype(np.uint32) | (rng.integers(0, 2, 400).astype(np.uint32) << 31)).view(np.float32), ids
    yield "normals", rng.standard_normal(400).astype(np.float32), ids


@pytest.mark.parametrize("largest", [True, False])
def test_restated_order_equals_a_brute_force_sort(largest):
    for what, scores, ids in _cases():
        assert R.order(scores, ids, largest).tolist() == _brute(scores, ids, largest), what


@pytest.mark.parametrize("largest", [True, False])
def test_restated_order_differs_from_three_wrong_selections(largest):
    """Ties by DESCENDING id, NaN ranked FIRST, ``-0.0 < +0.0``: each is a selection someone could have written, and on the special
    scores each picks another top 300 of the 400 than the restatement does
    (300: past the infinities and the normals, through the zeros and into the NaNs)."""
    def desc_ties(a, b, lg):
        return _before((a[0], -a[1]), (b[0], -b[1]), lg)

    def nan_first(a, b, lg):
        if math.isnan(a[0]) != math.isnan(b[0]):
            return math.isnan(a[0])
        return _before(a, b, lg)

    def signed_zero(a, b, lg):
        if a[0] == 0 and b[0] == 0 and math.copysign(1, a[0]) != math.copysign(1, b[0]):
            return (math.copysign(1, a[0]) > 0) == lg            # +0.0 is the larger one
        return _before(a, b, lg)
    _, scores, ids = next(_cases())
    right = R.order(scores, ids, largest)[:300].tolist()
    assert right == _brute(scores, ids, largest)[:300]
    for rule in (desc_ties, nan_first, signed_zero):
        assert _brute(scores, ids, largest, rule)[:300] != right, rule.__name__


def test_restated_top_streams_pads_and_counts():
    rng = np.random.default_rng(9)
    parts = [R.special_scores(n * 2, rng).reshape(n, 2) for n in (3, 0, 4)]
    s, i, c = R.top([(p, None) for p in parts], 5, True)
    whole = np.concatenate(parts)
    for j in range(2):
        best = _brute(whole[:, j], np.arange(7), True)[:5]
        assert np.array_equal(R.bits(s[j]), R.bits(whole[best, j])) and i[j].tolist() == best
    assert c.tolist() == [5, 5] and i.dtype == np.int32 and s.dtype == np.float32
    s, i, c = R.top([(parts[0], [9, 2 ** 31 - 1, 4])], 5, False)
    assert c.tolist() == [3, 3] and (i[:, 3:] == -1).all() and (R.bits(s[:, 3:]) == R.NAN_BITS).all()
    assert sorted(i[0, :3].tolist()) == [4, 9, 2 ** 31 - 1]
