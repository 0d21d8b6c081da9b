"""GPU (MI355X): the screening hit lists — ``glam_hits_merge`` / ``glam_hits_reset`` (csrc/hits.hip), ``hits.HitList`` on top of them and
``ArchitectureDTI.screen_top`` on top of that — against the restatement of ``tests/hits_restated.py`` (``numpy.lexsort`` under the one
total order).  Selection involves no rounding: every comparison is bit for bit (scores by their uint32 image, so NaN payloads and the
sign of a zero count), and there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from glam_amd import _lib, hits, model
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_molecule, synth_protein
from tests import hits_restated as R

pytestmark = pytest.mark.gpu

_KS = [1, 5, 64, 65, 1024]                  # one slot; a list inside a wave; a power of two and one past it; the largest list
_LS = [1, 63, 64, 65, 1000, 4097]           # fewer candidates than slots; around a wave; several rounds of 256 and one candidate over
_QS = [1, 3, 17]
_KINDS = ["normal", "ascending", "descending", "equal", "special"]

_INPUTS = {}


def _input(kind, L, Qs, device):
    """``[L, Qs]`` scores of one kind, host and device: made ONCE and shared, never written.  The ramps differ per column."""
    key = (kind, L, Qs)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * L + 10 * Qs + _KINDS.index(kind))
        ramp = (np.arange(L, dtype=np.float32)[:, None] + np.arange(Qs, dtype=np.float32)[None, :] * 0.5)
        s = {"normal": lambda: rng.standard_normal((L, Qs)).astype(np.float32),
             "ascending": lambda: ramp,                             # largest: every candidate displaces one
             "descending": lambda: -ramp,                           # largest: nothing enters after the first K
             "equal": lambda: np.full((L, Qs), 0.25, dtype=np.float32),
             "special": lambda: R.special_scores(L * Qs, rng).reshape(L, Qs)}[kind]()
        s = np.ascontiguousarray(s, dtype=np.float32)
        _INPUTS[key] = (s, torch.from_numpy(s).to(device))
    return _INPUTS[key]


def _snapshot(top):
    s, i, c = top.result()
    return s.clone(), i.clone(), c.clone()


@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
@pytest.mark.parametrize("K", _KS)
def test_one_update_equals_the_restatement(device, K, largest):
    """Every L x Qs x kind of input: scores, ids and counts bit-equal to the restatement; lists with fewer than K candidates end in
    NaN / -1; a second run on a reset list gives the same bits."""
    for Qs in _QS:
        top = hits.HitList(Qs, K, device, largest)
        for L in _LS:
            for kind in _KINDS:
                host, dev = _input(kind, L, Qs, device)
                top.reset().update(dev)
                got = _snapshot(top)
                what = f"K={K} L={L} Qs={Qs} {kind}"
                assert R.same(got, R.top([(host, None)], K, largest)), what
                if L < K:
                    assert (got[1][:, L:] == -1).all() and (R.bits(got[0][:, L:]) == R.NAN_BITS).all() and (got[2] == L).all(), what
                if kind == "special":
                    top.reset().update(dev)
                    assert R.same(top.result(), (got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy())), what + ": two runs differ"
        assert top.offered == _LS[-1]


@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
@pytest.mark.parametrize("K", [5, 64, 200])
def test_streamed_updates_equal_one_update_of_their_concatenation(device, K, largest):
    """Five updates of uneven L (an empty one among them) = one update of the concatenation = the restatement: with default ids, which
    takes the device's count across the updates, and with the caller's non-monotone ids (2^31 - 1 among them), from the host and from
    the device."""
    Qs, sizes = 3, [37, 0, 300, 1, 129]
    rng = np.random.default_rng(K)
    for kind in ("normal", "special", "equal"):
        whole_h, whole_d = _input(kind, sum(sizes), Qs, device)
        cuts = np.cumsum([0] + sizes)
        ids = (2 ** 31 - 1 - rng.permutation(sum(sizes)) * 4099).astype(np.int64)            # distinct, non-monotone, 2^31 - 1 among them
        assert ids.min() >= 0 and ids.max() == 2 ** 31 - 1 and np.unique(ids).size == ids.size
        for use_ids in (None, "host", "device"):
            streamed, once = hits.HitList(Qs, K, device, largest), hits.HitList(Qs, K, device, largest)
            parts = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                part = None if use_ids is None else ids[a:b] if use_ids == "host" else torch.from_numpy(ids[a:b].astype(np.int32)).to(device)
                streamed.update(whole_d[a:b], part)
                parts.append((whole_h[a:b], None if use_ids is None else ids[a:b]))
            once.update(whole_d, None if use_ids is None else ids if use_ids == "host" else torch.from_numpy(ids.astype(np.int32)).to(device))
            expected = R.top(parts, K, largest)
            what = f"K={K} {kind} ids={use_ids}"
            assert R.same(streamed.result(), expected), what
            assert R.same(once.result(), expected), what + " (one update)"
            assert streamed.seen.item() == once.seen.item() == sum(sizes) == streamed.offered
    # default ids at the top of their range: the count stands at 2^31 - n, the last candidate gets 2^31 - 1
    n = sum(sizes)
    whole_h, whole_d = _input("ascending" if largest else "descending", n, Qs, device)      # the last candidate is the best one
    high = hits.HitList(Qs, K, device, largest)
    high.seen.fill_(2 ** 31 - n)
    high.offered = 2 ** 31 - n
    high.update(whole_d)
    assert R.same(high.result(), R.top([(whole_h, np.arange(2 ** 31 - n, 2 ** 31, dtype=np.int64))], K, largest))
    assert high.seen.item() == 2 ** 31 and (high.result()[1][:, 0] == 2 ** 31 - 1).all()
    with pytest.raises(GlamHipError, match="default ids past"):
        high.update(whole_d[:1])
    again = streamed.reset()
    assert again.seen.item() == 0 and (again.result()[1] == -1).all() and (again.result()[2] == 0).all() and again.offered == 0


@pytest.mark.parametrize("K", [5, 65, 1024])
def test_the_grid_does_not_show(device, K):
    """slabs 1, 2, 7 and the library's choice: identical bits (and the restatement's), on a list that is warm from an earlier batch too.
    Through the kernel timer: an update is the two launches the header documents, by name."""
    Qs, L = 3, 1000
    for kind in ("normal", "special", "ascending"):
        host, dev = _input(kind, L, Qs, device)
        warm_h, warm_d = _input("normal", 1000, Qs, device)
        results = []
        for slabs in (0, 1, 2, 7):
            top = hits.HitList(Qs, K, device)
            top.update(warm_d, slabs=slabs)
            with _lib.kernel_timer() as kt:
                top.update(dev, slabs=slabs)
                torch.cuda.synchronize()
            rec = kt.records()
            assert [r[0] for r in rec] == ["k_hits_slab", "k_hits_finish"], rec
            assert rec[0][1] == Qs * (slabs or 1) and rec[1][1] == Qs, rec                 # (1 000 candidates: the library takes one slab)
            results.append(_snapshot(top))
        expected = R.top([(warm_h, None), (host, None)], K, True)
        for slabs, got in zip((0, 1, 2, 7), results):
            assert R.same(got, expected), f"K={K} {kind} slabs={slabs}"
    with _lib.kernel_timer() as kt:                                                        # nothing to merge: nothing launched
        top.update(dev[:0])
        hits.HitList(0, K, device).update(torch.empty(5, 0, device=device))
        torch.cuda.synchronize()
    assert [r[0] for r in kt.records()] == ["k_hits_reset"]


def test_scores_are_read_by_stride(device):
    """Task column 2 of an ``[L, Qs, 3]`` tensor, a transposed (query-major) view, a row-skipping view, and with one query ``[L]`` /
    ``[L, out_dim]``: each equal to the same update on a contiguous copy — and no copy is made (no ATen launch is needed: the pointer,
    the two strides and the task offset go to the kernel)."""
    L, Qs, K = 333, 4, 50
    host, dev = _input("special", L, Qs, device)
    want = hits.HitList(Qs, K, device).update(dev)
    expected = tuple(t.cpu().numpy() for t in want.result())
    assert R.same(want.result(), R.top([(host, None)], K, True))
    three = torch.randn(L, Qs, 3, device=device)
    three[:, :, 2] = dev
    assert R.same(hits.HitList(Qs, K, device).update(three, task=2).result(), expected)
    assert R.same(hits.HitList(Qs, K, device).update(three[:, :, 2]).result(), expected)
    transposed = dev.t().contiguous().t()
    assert transposed.stride() == (1, L) and R.same(hits.HitList(Qs, K, device).update(transposed).result(), expected)
    skipping = torch.randn(2 * L, Qs, 3, device=device)
    skipping[::2, :, 1] = dev
    assert R.same(hits.HitList(Qs, K, device).update(skipping[::2], task=1).result(), expected)
    one = hits.HitList(1, K, device).update(dev[:, 3])                                     # [L], stride Qs
    col = R.top([(host[:, 3:4], None)], K, True)
    assert R.same(one.result(), col)
    assert R.same(hits.HitList(1, K, device).update(dev, task=3).result(), col)            # one query: [L, out_dim]
    assert R.same(hits.HitList(1, K, device).update(three[:, 3:4], task=2).result(), col)  # [L, 1, out_dim]
    other = torch.zeros(L, Qs, device="cpu")
    with _lib.kernel_timer() as kt:
        with pytest.raises(GlamHipError, match="CPU tensor"):
            want.update(other)
        with pytest.raises(GlamHipError, match=r"scores must be \[L, 4\]"):
            want.update(dev[:, :3])
        with pytest.raises(GlamHipError, match="scores must be a float32 tensor"):
            want.update(dev.double())
        with pytest.raises(IndexError, match="ids must lie in"):
            want.update(dev, [-1] * L)
        with pytest.raises(GlamHipError, match="device ids must be a contiguous int32"):
            want.update(dev, torch.zeros(L, dtype=torch.int64, device=device))
        want.offered = 2 ** 31 - L + 1
        with pytest.raises(GlamHipError, match="default ids past"):
            want.update(dev)
    assert kt.records() == [], "a refusal launched something"
    assert R.same(want.result(), expected), "a refused update changed the lists"


def test_a_captured_update_replays_on_fresh_data(device):
    """ONE ``update`` on a static input buffer, default ids, captured with ``torch.cuda.graph`` and replayed three times with fresh
    data copied in: the restatement over the three batches — the ids continue across the replays (the count lives on the device)."""
    L, Qs, K = 500, 3, 20
    batches = [_input(kind, L, Qs, device) for kind in ("normal", "special", "ascending")]
    top = hits.HitList(Qs, K, device)
    static = batches[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        top.update(static)                                       # eager warm-up (the workspace exists before the capture)
        top.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        top.update(static)
    for n, (host, dev) in enumerate(batches):
        static.copy_(dev)
        graph.replay()
        torch.cuda.synchronize()
        assert top.seen.item() == (n + 1) * L
        assert R.same(top.result(), R.top([(h, None) for h, _ in batches[:n + 1]], K, True)), n


# ---------------------------------------------------------------------------------------------
# ArchitectureDTI.screen_top
# ---------------------------------------------------------------------------------------------
def test_screen_top_equals_a_hit_list_fed_by_hand(device):
    """A small two-tower model, 4 proteins, selection ``[2, 0, 2]``, 5 ligand batches of 7..40 molecules, ``k=10``, ``task=1``:
    ``screen_top`` = a ``HitList`` fed with the ``screen_panel`` outputs of the same batches (the kernels are atomic-free: two runs give
    the same bits) = the restatement applied to those outputs; the duplicated protein holds the same list twice; items given as
    ``(data_mol, ids)``; a stale encoding and ``train()`` mode are refused with ``screen_panel``'s own messages."""
    rng = np.random.default_rng(3)
    sizes, sel = [7, 40, 13, 32, 21], [2, 0, 2]
    torch.manual_seed(5)
    net = model.ArchitectureDTI(e_dim=64, message_steps=2, out_dim=2).to(device).eval()
    net.graphed_call = False
    pros = Batch.from_data_list([synth_protein(rng, 40, 60) for _ in range(4)]).to(device)
    ligands = [Batch.from_data_list([synth_molecule(rng) for _ in range(n)]).to(device) for n in sizes]
    ids = [(2 ** 31 - 1 - 7 * np.arange(a, a + n)).astype(np.int64) for a, n in zip(np.cumsum([0] + sizes), sizes)]
    with torch.no_grad():
        enc = net.encode_proteins(pros)
        outs = [net.screen_panel(b, enc, sel) for b in ligands]
        assert all(o.shape == (n, 3, 2) for o, n in zip(outs, sizes))
        by_hand = hits.HitList(3, 10, device)
        for o in outs:
            by_hand.update(o, task=1)
        top = net.screen_top(ligands, enc, sel, k=10, task=1)
        assert isinstance(top, hits.HitList) and (top.queries, top.k, top.largest, top.offered) == (3, 10, True, sum(sizes))
        host = [o[:, :, 1].cpu().numpy() for o in outs]
        expected = R.top([(h, None) for h in host], 10, True)
        assert R.same(top.result(), expected) and R.same(by_hand.result(), expected)
        s, i, c = top.result()
        assert torch.equal(i[0], i[2]) and np.array_equal(R.bits(s[0]), R.bits(s[2])) and c.tolist() == [10, 10, 10]
        assert 0 <= int(i.min()) and int(i.max()) < sum(sizes)                            # default ids: positions in the stream
        # (data_mol, ids) items, host ids and device ids; the smallest scores of task 0; a generator as the stream
        mixed = ((b, d if n % 2 else torch.from_numpy(d.astype(np.int32)).to(device)) for n, (b, d) in enumerate(zip(ligands, ids)))
        low = net.screen_top(mixed, enc, sel, k=1024, task=0, largest=False)
        assert R.same(low.result(), R.top([(o[:, :, 0].cpu().numpy(), d) for o, d in zip(outs, ids)], 1024, False))
        assert low.result()[2].tolist() == [sum(sizes)] * 3
        all_q = net.screen_top(ligands[:2], enc, k=3)                                      # every protein, task 0
        assert R.same(all_q.result(), R.top([(net.screen_panel(b, enc)[:, :, 0].cpu().numpy(), None) for b in ligands[:2]], 3, True))
        empty = net.screen_top([], enc, sel, k=4)
        assert empty.queries == 3 and (empty.result()[1] == -1).all() and empty.offered == 0
        with pytest.raises(IndexError, match="ids must have one entry per candidate"):
            net.screen_top([], enc, sel).update(outs[0], ids[1])
        with pytest.raises(IndexError, match="ids must have one entry per candidate"):
            net.screen_top([(ligands[0], ids[1])], enc, sel)
        net.train()
        with pytest.raises(GlamHipError, match="screen_panel: the model is in training mode"):
            net.screen_top(ligands, enc, sel)
        net.eval()
        next(net.pro_conv.parameters()).add_(1)
        with pytest.raises(GlamHipError, match="screen_panel: the encoding is stale"):
            net.screen_top(ligands, enc, sel)
    with pytest.raises(GlamHipError, match="screen_panel is inference only"):
        net.screen_top(ligands, enc, sel)
