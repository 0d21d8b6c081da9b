"""GPU (MI355X): the class table — ``ops.pair_head_classes`` (``glam_pair_head_classes_fwd``: csrc/pairhead.hip),
``ArchitectureDDI.classify_matrix`` / ``ArchitectureDTI.classify_panel`` and ``score="logp"`` of ``matrix_top`` / ``screen_top``.

What everything rests on: a logit is the factored head's chain bit for bit, and the called class, its log-softmax and the selected
log-softmaxes are ONE fixed sequence over the pair's own logits in class order — so the op sits within the fp64-twin bound of the
restatement (``tests/pair_classes_restated.py``, shown equal to the listed head + ``torch.log_softmax`` / ``argmax`` on the CPU), calls
the fp64 class at every entry, does not depend on the table around an entry, and allocates neither the hidden matrix nor the logits."""
import numpy as np
import pytest
import torch

from glam_amd import _lib, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch
from tests import hits_restated
from tests import pair_classes_restated as C
from tests import pair_head_restated as H
from tests import test_gpu_panel as P
from tests.conftest import assert_fp32_parity, assert_twin_parity
from tests.test_gpu_ddi_matrix import _MCOLS, _MROWS, _drugs
from tests.test_gpu_ddi_pairs import _net, _oracle_ddi
from tests.test_gpu_pair_head import _on

pytestmark = pytest.mark.gpu

T = ops.HEAD_CLASS_TILE
_KINDS = ("k_pair_head_classes_side", "k_pair_head_classes")
# (R, Cs): one pair; rows and a column chunk with a 3-lane tail; exactly one chunk; more than two blocks of rows on the LANES (130 x 2)
# hid 15: padded views;  e_dim: a multiple of 64, 70 (the weight as a view of a wider matrix), the models' 1 024;  F: none, two steps, three
# out_dim: 2, the factored head's limit 8 and 9, one tile, one more, two tiles and three, 86, 128
CASES = [(1, 1, 60, 64, 0, T + 1, "none", 0.0), (5, 67, 15, 70, 4, 86, "relu", 0.0), (3, 64, 60, 1024, 6, 2 * T + 3, "leaky", 0.2),
         (130, 2, 15, 70, 6, 9, "leaky", 0.2), (130, 2, 60, 64, 0, 128, "relu", 0.0), (5, 67, 60, 64, 4, 2, "none", 0.0),
         (3, 64, 15, 70, 4, T, "none", 0.0), (1, 1, 15, 70, 6, 8, "relu", 0.0), (5, 67, 60, 70, 0, 8, "leaky", 0.2)]
_REFS = {}


def _selected(out_dim):
    """Last class, first, a middle one, the last again: out of order, with a duplicate, from several tiles."""
    return [out_dim - 1, 0, out_dim // 2, out_dim - 1]


def _case(R, Cs, hid, e_dim, F, out_dim, act, slope):
    """fp32 inputs and the restatement in fp32 / fp64 on the CPU, computed ONCE per case and shared (never written)."""
    key = (R, Cs, hid, e_dim, F, out_dim, act, slope)
    if key not in _REFS:
        t = H.inputs(R, Cs, hid, e_dim, F, out_dim, seed=R * 1000 + Cs)
        t32 = tuple(None if x is None else x.float() for x in t)
        t64 = [None if x is None else x.double() for x in t32]
        sel = _selected(out_dim)
        _REFS[key] = (t32, C.classes(*t32, act=act, slope=slope, classes=sel), C.classes(*t64, act=act, slope=slope, classes=sel))
    return _REFS[key]


def _run(args, act, slope, classes, logits=True):
    with torch.no_grad():
        return ops.pair_head_classes(*args, act=act, slope=slope, classes=classes, logits=logits)


def _same(x, y):
    """Two class tables bit for bit (NaN equals NaN)."""
    return (torch.equal(x.cls, y.cls) and all(np.array_equal(hits_restated.bits(a), hits_restated.bits(b))
                                              for a, b in ((x.logp, y.logp), (x.sel, y.sel), (x.logits, y.logits))))


@pytest.mark.parametrize("R,Cs,hid,e_dim,F,out_dim,act,slope", CASES)
def test_class_table_matches_the_restatement_within_the_fp64_twin_bound(device, R, Cs, hid, e_dim, F, out_dim, act, slope):
    """``logits`` / ``logp`` / ``sel`` within ``assert_fp32_parity`` of the fp64 restatement; ``cls`` IS the fp64 argmax at every entry (for
    these seeds the fp64 margin between the two largest logits is at least twice the parity bound at every entry: asserted here, on
    the references alone); ``cls`` is ``torch.argmax`` of the op's own logits exactly; two runs agree bit for bit."""
    t32, ref32, ref64 = _case(R, Cs, hid, e_dim, F, out_dim, act, slope)
    args = _on(t32, device, padded_rows=hid == 15, wide_weight=e_dim == 70)
    sel = _selected(out_dim)
    out, again = _run(args, act, slope, sel), _run(args, act, slope, sel)
    what = f"pair_head_classes {R}x{Cs} hid={hid} e_dim={e_dim} F={F} out_dim={out_dim} {act}"
    assert isinstance(out, ops.ClassTable) and out.cls.dtype == torch.int32 and out.cls.shape == (R, Cs) and out.logp.shape == (R, Cs)
    assert out.sel.shape == (R, Cs, 4) and out.logits.shape == (R, Cs, out_dim) and all(x.is_contiguous() for x in out)
    assert _same(out, again), "two runs differ"
    _, bound = assert_fp32_parity(out.logits, ref64[3], ref32[3], what + " logits")
    assert_fp32_parity(out.logp, ref64[1], ref32[1], what + " logp")
    assert_fp32_parity(out.sel, ref64[2], ref32[2], what + " sel")
    top2 = ref64[3].topk(2, -1).values
    margin = (top2[..., 0] - top2[..., 1]).min().item()
    print(f"{what}: fp64 top-two margin {margin:.2e}, logits bound {bound:.2e}")
    assert margin >= 2 * bound, f"{what}: an entry's two largest logits are {margin:.1e} apart, under twice the bound {bound:.1e}: another seed"
    assert torch.equal(out.cls.cpu().long(), ref64[0]), f"{what}: cls is not the fp64 argmax at every entry"
    assert torch.equal(out.cls.long(), torch.argmax(out.logits, -1)), f"{what}: cls is not the argmax of the op's own logits"
    lse = torch.logsumexp(out.logits.double(), -1)
    assert_fp32_parity(out.logp, out.logits.double().max(-1).values - lse, ref32[1], what + " logp vs max - lse of its logits")
    assert torch.equal(out.sel[..., 0], out.sel[..., 3]), "a class named twice is not the same column twice"
    bare = _run(args, act, slope, (), logits=False)                             # nothing selected, no logits: the same cls / logp
    assert bare.logits is None and bare.sel.shape == (R, Cs, 0)
    assert torch.equal(bare.cls, out.cls) and torch.equal(bare.logp, out.logp)


@pytest.mark.parametrize("R,Cs,hid,e_dim,F,out_dim,act,slope", [c for c in CASES if c[5] <= ops.HEAD_MAX_OUT])
def test_class_table_logits_are_the_factored_heads_chain(device, R, Cs, hid, e_dim, F, out_dim, act, slope):
    """For ``out_dim <= 8`` both heads exist: the logits are ``ops.pair_head`` on the same arguments bit for bit."""
    t32, _, _ = _case(R, Cs, hid, e_dim, F, out_dim, act, slope)
    args = _on(t32, device, padded_rows=hid == 15, wide_weight=e_dim == 70)
    with torch.no_grad():
        assert torch.equal(_run(args, act, slope, ()).logits, ops.pair_head(*args, act=act, slope=slope))


def test_class_table_entries_do_not_depend_on_the_selection(device):
    """Bit for bit on all four outputs: the 5 x 67 table's entries at 86 classes are those of the same op on row subsets, on column
    subsets (the 3-column one puts the ROWS on the lanes), on single pairs, and with ``classes`` in another order and with a duplicate."""
    t32, _, _ = _case(5, 67, 15, 70, 4, 86, "relu", 0.0)
    a, b, f, lin0, lin1 = _on(t32, device, padded_rows=True, wide_weight=True)
    sel = [85, 0, 43]

    def run(ra, cb, classes=sel):
        return _run((a[ra], b[cb], f[ra][:, cb], lin0, lin1), "relu", 0.0, classes)

    def cut(t, ra, cb):
        return ops.ClassTable(t.cls[ra][:, cb], t.logp[ra][:, cb], t.sel[ra][:, cb], t.logits[ra][:, cb])
    whole = run(slice(0, 5), slice(0, 67))
    for ra, cb in ((slice(0, 2), slice(0, 67)), (slice(2, 5), slice(0, 67)), (slice(0, 5), slice(0, 64)), (slice(0, 5), slice(64, 67)),
                   (slice(3, 4), slice(65, 66)), (slice(0, 1), slice(0, 1)), (slice(4, 5), slice(66, 67))):
        assert _same(run(ra, cb), cut(whole, ra, cb)), f"rows {ra} x columns {cb} differ from the whole table's"
    other = run(slice(0, 5), slice(0, 67), [43, 43, 85, 0, 0])
    assert torch.equal(other.cls, whole.cls) and torch.equal(other.logp, whole.logp) and torch.equal(other.logits, whole.logits)
    assert torch.equal(other.sel, whole.sel[..., [2, 2, 0, 1, 1]]), "classes in another order / twice are not the same columns"
    eight = run(slice(0, 5), slice(0, 67), list(range(80, 86)) + [0, 17])       # the most a call takes, from three tiles
    assert eight.sel.shape == (5, 67, 8) and torch.equal(eight.cls, whole.cls) and torch.equal(eight.logp, whole.logp)
    assert torch.equal(eight.sel[..., 5], whole.sel[..., 0]) and torch.equal(eight.sel[..., 6], whole.sel[..., 1])
    lsm = torch.log_softmax(whole.logits.double(), -1)[..., list(range(80, 86)) + [0, 17]]
    assert (eight.sel.double() - lsm).abs().max().item() <= 16 * 2.0 ** -24 * max(1.0, lsm.abs().max().item()), "eight selected classes"


def test_class_table_ties_and_nan(device):
    """Two ``lin1`` rows duplicated with the largest bias: ``cls`` is the SMALLER index, within a tile and across tiles.  One NaN in
    ``f[i, j]``: that entry is ``cls = 0`` with NaN ``logp`` / ``sel``, every other entry is the clean table's bit for bit."""
    t32, _, _ = _case(5, 67, 15, 70, 4, 86, "relu", 0.0)
    sel = [85, 0, 43]
    clean = _run(_on(t32, device, True, True), "relu", 0.0, sel)
    for lo, hi in ((3, 5), (20, 70), (0, 85)):
        tied = _run(_on(C.with_tie(t32, lo, hi), device, True, True), "relu", 0.0, sel)
        assert torch.equal(tied.logits[..., lo], tied.logits[..., hi]), "the duplicated rows do not tie exactly"
        assert (tied.cls == lo).all(), f"a tie of classes {lo} and {hi} does not call the smaller index everywhere"
        assert torch.equal(tied.cls.long(), torch.argmax(tied.logits, -1))
    for i, j in ((3, 65), (0, 0)):
        bad = _run(_on(C.with_nan(t32, i, j, 1), device, True, True), "relu", 0.0, sel)
        assert bad.cls[i, j] == 0 and torch.isnan(bad.logp[i, j]) and torch.isnan(bad.sel[i, j]).all() and torch.isnan(bad.logits[i, j]).all()
        keep = torch.ones(5, 67, dtype=torch.bool, device=device)
        keep[i, j] = False
        for got, want in zip(bad, clean):
            assert torch.equal(got[keep], want[keep]), "a NaN in one pair changed another entry"
    # one NaN CLASS (a NaN bias): torch.argmax calls it — the first of two — at every pair
    t = [None if x is None else x.clone() for x in t32]
    t[6][[40, 7]] = float("nan")
    nan_class = _run(_on(tuple(t), device, True, True), "relu", 0.0, sel)
    assert (nan_class.cls == 7).all() and torch.isnan(nan_class.logp).all() and torch.isnan(nan_class.sel).all()
    assert torch.equal(nan_class.cls.long(), torch.argmax(nan_class.logits, -1))


def test_class_table_launches_refusals_and_empty_tables(device):
    """One call is the side launch (both products and the transposed weight) plus ONE ``k_pair_head_classes``; an empty table and a
    refusal launch nothing."""
    t32, _, _ = _case(5, 67, 15, 70, 4, 86, "relu", 0.0)
    args = _on(t32, device, False)
    a, b, f, lin0, lin1 = args
    with _lib.kernel_timer() as kt:
        _run(args, "relu", 0.0, [1])
    # 5 x 67, hid = 15, e_dim = 70, 86 classes: the columns on the lanes.  A: 70 x ceil(5 / 4) threads = 1 block; Bt: 67 x ceil(70 / 4)
    # threads = 5 blocks; w1t: (70 + 1) x 96 elements = 27 blocks;  the table: two lane chunks x one group of 16 rows
    assert [(n, g) for n, g, _ in kt.records()] == [("k_pair_head_classes_side", 1 + 5 + 27), ("k_pair_head_classes", 2)]
    with _lib.kernel_timer() as kt:            # 130 x 2, e_dim = 64, 128 classes: the rows on the lanes — At: 130 x 16 threads = 9 blocks,
        t130, _, _ = _case(130, 2, 60, 64, 0, 128, "relu", 0.0)                  # B: 64 x 1 = 1, w1t: 65 x 128 = 33; three lane chunks
        _run(_on(t130, device, False), "relu", 0.0, ())
    assert [(n, g) for n, g, _ in kt.records()] == [("k_pair_head_classes_side", 9 + 1 + 33), ("k_pair_head_classes", 3)]
    with _lib.kernel_timer() as kt:
        e = _run((a[:0], b, f[:0], lin0, lin1), "relu", 0.0, [1, 2])
        assert e.cls.shape == (0, 67) and e.logp.shape == (0, 67) and e.sel.shape == (0, 67, 2) and e.logits.shape == (0, 67, 86)
        e = _run((a, b[:0], f[:, :0], lin0, lin1), "relu", 0.0, (), logits=False)
        assert e.cls.shape == (5, 0) and e.cls.dtype == torch.int32 and e.sel.shape == (5, 0, 0) and e.logits is None
        with torch.no_grad():
            with pytest.raises(GlamHipError, match="CPU tensor"):
                ops.pair_head_classes(a.cpu(), b, f, lin0, lin1)
            with pytest.raises(GlamHipError, match="pair_head_classes: the two sides disagree"):
                ops.pair_head_classes(a, b[:, :14], f, lin0, lin1)
            with pytest.raises(GlamHipError, match=r"pair_head_classes: f must be \[5, 67, F\]"):
                ops.pair_head_classes(a, b, f[:, :66], lin0, lin1)
            with pytest.raises(GlamHipError, match="pair_head_classes: lin1 must map the 70 outputs"):
                ops.pair_head_classes(a, b, f, lin0, (lin1[0][:, :69], lin1[1]))
            with pytest.raises(GlamHipError, match="pair_head_classes: out_dim = 1 is outside 2..1024"):
                ops.pair_head_classes(a, b, f, lin0, (lin1[0][:1], lin1[1][:1]))
            with pytest.raises(GlamHipError, match="pair_head_classes: out_dim = 1025 is outside 2..1024"):
                ops.pair_head_classes(a, b, f, lin0, (torch.zeros(1025, 70, device=device), torch.zeros(1025, device=device)))
            with pytest.raises(GlamHipError, match="pair_head_classes: F = 17 fusion columns are outside 0..16"):
                ops.pair_head_classes(a, b, torch.zeros(5, 67, 17, device=device), (torch.zeros(70, 47, device=device), lin0[1]), lin1)
            with pytest.raises(GlamHipError, match="act = 'celu'"):
                ops.pair_head_classes(a, b, f, lin0, lin1, "celu")
            with pytest.raises(IndexError, match=r"classes must lie in \[0, 86\)"):
                ops.pair_head_classes(a, b, f, lin0, lin1, classes=[86])
            with pytest.raises(GlamHipError, match="classes lives on a device"):
                ops.pair_head_classes(a, b, f, lin0, lin1, classes=torch.tensor([1], device=device))
        with pytest.raises(GlamHipError, match=r"pair_head_classes is inference only"):
            ops.pair_head_classes(a.clone().requires_grad_(True), b, f, lin0, lin1)
    assert kt.records() == [], "an empty table or a refusal launched something"


def test_class_table_never_allocates_the_logits(device):
    """130 x 67 pairs, e_dim = 1 024, 86 classes, without ``logits``: the peak above the starting allocation stays below the
    130 * 67 * 86 * 4 bytes (2.9 MB) of the logits table alone — the call holds ``A`` + ``Bt`` + the padded transposed weight (1.2 MB) and
    its three small results; a fortiori no ``[pairs, e_dim]`` hidden matrix (35.7 MB).  The same probe sees the logits when asked for."""
    args = _on(tuple(None if x is None else x.float() for x in H.inputs(130, 67, 60, 1024, 4, 86, seed=130067)), device, False)
    peaks = {}
    for logits in (False, True, False):                                        # (the first call loads the kernels; the others are measured)
        torch.cuda.synchronize()
        start = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = _run(args, "relu", 0.0, [1], logits=logits)
        torch.cuda.synchronize()
        peaks[logits] = torch.cuda.max_memory_allocated() - start
        del out
    table = 130 * 67 * 86 * 4
    print(f"peak above the start: without logits {peaks[False]} B, with {peaks[True]} B; the logits table {table} B")
    assert peaks[False] < table, f"pair_head_classes without logits peaked {peaks[False]} B above its start"
    assert peaks[True] >= table, "the probe does not see the logits table when it is asked for"


# ---------------------------------------------------------------------------------------------
# ArchitectureDDI.classify_matrix, matrix_top(score="logp")
# ---------------------------------------------------------------------------------------------
def _class_parity(table, o64, o32, sel, what):
    """A ``ClassTable`` with logits against the oracle's output in both precisions: the logits by twin parity, the rest against
    ``torch.log_softmax`` of the oracle's logits by the fp64-twin bound; ``cls`` the argmax of the table's own logits."""
    assert_twin_parity(lambda dt: (o64 if dt == torch.float64 else o32, []), table.logits, [], what + " logits")
    r64, r32 = C.from_logits(o64, sel), C.from_logits(o32, sel)
    assert_fp32_parity(table.logp, r64[1], r32[1], what + " logp")
    assert_fp32_parity(table.sel, r64[2], r32[2], what + " sel")
    assert torch.equal(table.cls.long(), torch.argmax(table.logits, -1)), what + ": cls is not the argmax of its logits"


def test_classify_matrix_vs_the_oracle_and_matrix_top_by_logp(device):
    """The small DDI net at 11 classes: ``classify_matrix`` against the oracle's two-drug model on the expanded batches; an entry is the
    call on its own pair bit for bit; ``matrix_top(score="logp")`` over three blocks of two row drugs is ``hits_restated.top`` of the whole
    table's ``sel[..., 0]`` exactly; ``score="logit"`` is the call without the keyword."""
    drugs = _drugs()
    net = _net(out_dim=11)
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    R, Cs, task = len(_MROWS), len(_MCOLS), 4
    cast = lambda b, dt: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
    first, second = np.repeat(_MROWS, Cs).tolist(), np.tile(_MCOLS, R).tolist()
    e1, e2 = Batch.from_data_list([drugs[q] for q in first]), Batch.from_data_list([drugs[q] for q in second])

    def oracle(dt):
        sd = {k: v.to(dt) if v.is_floating_point() else v for k, v in sd0.items()}
        with torch.no_grad():
            return _oracle_ddi(sd, cast(e1, dt), cast(e2, dt), R * Cs, dt, "_NNConv", "_None", "GlobalPool5", "_None").view(R, Cs, 11)
    net = net.to(device)
    net.graphed_call = False
    sel = [task, 10, 0]
    with torch.no_grad():
        enc = net.encode_drugs(Batch.from_data_list(drugs).to(device))
        with _lib.kernel_timer() as kt:
            table = net.classify_matrix(enc, _MROWS, _MCOLS, classes=sel, return_logits=True)
        names = [n for n, _, _ in kt.records()]
        assert [n for n in names if n.startswith("k_pair_head")] == list(_KINDS), "the class head is one side launch and one table launch"
        assert [n for n in names if n.startswith("k_pair_grid")] == ["k_pair_grid", "k_pair_grid_finish"] * 2
        assert table.cls.shape == (R, Cs) and table.sel.shape == (R, Cs, 3) and table.logits.shape == (R, Cs, 11)
        _class_parity(table, oracle(torch.float64), oracle(torch.float32), sel, "classify_matrix out_dim=11")
        assert _same(table, net.classify_matrix(enc, _MROWS, _MCOLS, classes=sel, return_logits=True)), "two runs differ"
        bare = net.classify_matrix(enc, _MROWS, _MCOLS)
        assert bare.logits is None and bare.sel.shape == (R, Cs, 0) and torch.equal(bare.cls, table.cls) and torch.equal(bare.logp, table.logp)
        for i, j in ((0, 0), (3, 1), (5, 4)):
            one = net.classify_matrix(enc, [_MROWS[i]], [_MCOLS[j]], classes=sel, return_logits=True)
            assert _same(one, ops.ClassTable(*[t[i:i + 1, j:j + 1] for t in table])), f"entry ({i}, {j}) alone differs"
        full = net.classify_matrix(enc, classes=sel, return_logits=True)
        assert _same(ops.ClassTable(*[t[_MROWS][:, _MCOLS] for t in full]), table), "entries picked from the whole table differ"
        assert net.classify_matrix(enc, [], _MCOLS, classes=sel).sel.shape == (0, Cs, 3)
        assert net.classify_matrix(enc, _MROWS, [], return_logits=True).logits.shape == (R, 0, 11)
        # the partner lists by log-probability of class `task`
        want = hits_restated.top([(table.sel[..., 0].cpu().numpy(), _MROWS)], 3, True)
        for block_rows in (2, 1, 0):                                            # three blocks, six, one
            top = net.matrix_top(enc, _MROWS, _MCOLS, k=3, task=task, block_rows=block_rows, score="logp")
            assert top.queries == Cs and top.offered == R
            assert hits_restated.same(top.result(), want), f"block_rows={block_rows}: not the top of the table's log-probabilities"
        low = net.matrix_top(enc, _MROWS, _MCOLS, k=3, task=task, largest=False, block_rows=2, score="logp")
        assert hits_restated.same(low.result(), hits_restated.top([(table.sel[..., 0].cpu().numpy(), _MROWS)], 3, False))
        with _lib.kernel_timer() as kt:
            empty = net.matrix_top(enc, [], _MCOLS, k=3, task=task, score="logp")
            with pytest.raises(GlamHipError, match="matrix_top: score = 'prob' is not"):
                net.matrix_top(enc, _MROWS, _MCOLS, score="prob")
            with pytest.raises(GlamHipError, match=r"score_matrix: head=\"factored\" keeps out_dim"):      # 11 columns: no factored head
                net.matrix_top(enc, _MROWS, _MCOLS, task=task)
        assert empty.queries == Cs and empty.offered == 0
        assert [n for n, _, _ in kt.records() if n.startswith("k_pair")] == [], "an empty rows or a refusal scored something"
        by_rows = net.matrix_top(enc, _MROWS, _MCOLS, k=3, task=task, block_rows=2, head="rows")
        logit = net.matrix_top(enc, _MROWS, _MCOLS, k=3, task=task, block_rows=2, head="rows", score="logit")
        assert hits_restated.same(logit.result(), tuple(x.cpu().numpy() for x in by_rows.result())), "score=\"logit\" is not the call of today"
    small = _net(out_dim=3).to(device)                                          # ... and on the factored head, the default route
    with torch.no_grad():
        enc3 = small.encode_drugs(Batch.from_data_list(drugs).to(device))
        plain = small.matrix_top(enc3, _MROWS, _MCOLS, k=3, task=2, block_rows=2)
        logit = small.matrix_top(enc3, _MROWS, _MCOLS, k=3, task=2, block_rows=2, score="logit")
        assert hits_restated.same(logit.result(), tuple(x.cpu().numpy() for x in plain.result()))
        assert torch.equal(small.classify_matrix(enc3, _MROWS, _MCOLS, return_logits=True).logits,
                           small.score_matrix(enc3, _MROWS, _MCOLS, head="factored")), "the logits are not the factored head's bits"


# ---------------------------------------------------------------------------------------------
# ArchitectureDTI.classify_panel, screen_top(score="logp")
# ---------------------------------------------------------------------------------------------
def test_classify_panel_vs_the_oracle_and_screen_top_by_logp(device):
    """The small DTI net with two classes: column ``j`` against the oracle's two-tower model on that column's expanded batch; a column is
    the call on its own protein bit for bit; ``screen_top(score="logp")`` over a stream of three batches is ``hits_restated.top`` of the
    batches' ``sel[..., 0]`` exactly; ``score="logit"`` is the call without the keyword."""
    mols, pros = P._graphs()
    mb = Batch.from_data_list(mols)
    net = P._net(out_dim=2)
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    cast = lambda b, dt: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
    sel = [2, 0]

    def oracle(dt):
        sd = {k: v.to(dt) for k, v in sd0.items()}
        with torch.no_grad():
            return torch.stack([P._oracle_dti(sd, cast(mb, dt), cast(Batch.from_data_list([pros[q]] * P._L), dt), P._L, "_NNConv",
                                              "_GCNConv", "_None", "_None") for q in sel], 1)
    net = net.to(device)
    net.graphed_call = False
    mol_dev = mb.to(device)
    with torch.no_grad():
        enc = net.encode_proteins(Batch.from_data_list(pros).to(device))
        with _lib.kernel_timer() as kt:
            table = net.classify_panel(mol_dev, enc, sel, classes=[1], return_logits=True)
        assert [n for n, _, _ in kt.records() if n.startswith("k_pair_head")] == list(_KINDS)
        assert table.cls.shape == (P._L, 2) and table.sel.shape == (P._L, 2, 1) and table.logits.shape == (P._L, 2, 2)
        _class_parity(table, oracle(torch.float64), oracle(torch.float32), [1], "classify_panel out_dim=2")
        assert torch.equal(table.logits, net.screen_panel(mol_dev, enc, sel, head="factored")), "the logits are not the factored head's bits"
        assert _same(table, net.classify_panel(mol_dev, enc, sel, classes=[1], return_logits=True)), "two runs differ"
        whole = net.classify_panel(mol_dev, enc, classes=[1], return_logits=True)
        assert _same(ops.ClassTable(*[t[:, sel] for t in whole]), table), "columns picked from the whole panel differ"
        one = net.classify_panel(mol_dev, enc, [sel[1]], classes=[1], return_logits=True)
        assert _same(one, ops.ClassTable(*[t[:, 1:2] for t in table])), "a column alone differs"
        assert net.classify_panel(mol_dev, enc, [], classes=[1]).sel.shape == (P._L, 0, 1)
        # a stream of three batches, with ids
        stream = [(Batch.from_data_list(mols[i0:i1]).to(device), list(range(100 + i0, 100 + i1))) for i0, i1 in ((0, 2), (2, 4), (4, 5))]
        want = hits_restated.top([(net.classify_panel(bm, enc, sel, classes=[1]).sel[..., 0].cpu().numpy(), ids) for bm, ids in stream], 3, True)
        top = net.screen_top(stream, enc, sel, k=3, task=1, score="logp")
        assert top.queries == 2 and top.offered == P._L
        assert hits_restated.same(top.result(), want), "screen_top(score=logp) is not the top of the batches' log-probabilities"
        plain = net.screen_top(stream, enc, sel, k=3, task=1)
        logit = net.screen_top(stream, enc, sel, k=3, task=1, score="logit")
        assert hits_restated.same(logit.result(), tuple(x.cpu().numpy() for x in plain.result())), "score=\"logit\" is not the call of today"
        with _lib.kernel_timer() as kt:
            with pytest.raises(GlamHipError, match="screen_top: score = 'x' is not"):
                net.screen_top(stream, enc, sel, score="x")
            assert net.screen_top([], enc, sel, k=3, task=1, score="logp").queries == 2
        # (the empty lists themselves are one k_hits_reset)
        assert [n for n, _, _ in kt.records() if n.startswith("k_pair")] == [], "a refusal or an empty stream scored something"
