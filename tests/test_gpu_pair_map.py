"""``ops.pair_map`` (csrc/pairmap.hip) against the restatement of tests/pair_map_restated.py — whose assertions tests/test_pair_map_host.py
shows to discriminate — and against the fusion it explains (``ops.pair_pool_gather``), bit for bit; then ``explain.explain_pair`` on small
DTI and DDI models against ``screen`` / ``score_pairs`` and against ``ops.pair_map`` on every step's rows."""
import functools

import numpy as np
import pytest
import torch

from glam_amd import _lib, explain, layer, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_batch, synth_molecule, synth_protein
from tests import pair_map_restated as R

pytestmark = pytest.mark.gpu


def _sp(sizes, device):
    return ops.SegmentPtr(R.batch_of(sizes).to(device), len(sizes))


def _equal(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in R.FIELDS + ("out_ptr1", "out_ptr2"))


@functools.lru_cache(maxsize=None)
def _modes(D):
    """Operands and both restatements (over all nine pairs, computed once) per index mode: a side without an index holds its segments
    physically gathered, one copy per pair."""
    x1, x2 = R.random_case(D)
    (g1, gs1), (g2, gs2) = R.gathered(x1, R.SIZES1, R.IDX1), R.gathered(x2, R.SIZES2, R.IDX2)
    out = {}
    for mode, args in (("both", (x1, x2, R.SIZES1, R.SIZES2, R.IDX1, R.IDX2)), ("idx1 only", (x1, g2, R.SIZES1, gs2, R.IDX1, None)),
                       ("idx2 only", (g1, x2, gs1, R.SIZES2, None, R.IDX2)), ("neither", (g1, g2, gs1, gs2, None, None))):
        out[mode] = (args, R.restate(*args, torch.float32), R.restate(*args, torch.float64))
    return out


def _operands(args, P, device):
    """The call on the first ``P`` pairs: an indexed side whole, an identity side cut to its first ``P`` segments."""
    xa, xb, sa, sb, ia, ib = args
    if ia is None:
        sa, xa = sa[:P], xa[:sum(sa[:P])]
    if ib is None:
        sb, xb = sb[:P], xb[:sum(sb[:P])]
    return (xa.to(device), xb.to(device), _sp(sa, device), _sp(sb, device)), (sa, sb, None if ia is None else ia[:P], None if ib is None else ib[:P])


@pytest.mark.parametrize("D", R.WIDTHS)
def test_maps_against_the_restatement_and_the_fusion(device, D):
    """16-byte form (4, 60, 64, 92, 128) and dword form (15); ``P`` = 1, 4, 5, 9: one wave, a full block, a partial block, three blocks and
    more; both indices, either one, neither.  Parity against fp64, the fills, and the tie-back to ``pair_pool_gather`` bit for bit."""
    (xa, xb, spa, spb), (sa, sb, ia, ib) = _operands(_modes(D)["both"][0], 9, device)
    with torch.no_grad():
        full = R.as_host(ops.pair_map(xa, xb, spa, spb, ops.map_plan(sa, sb, ia, ib)))
    for mode, (args, r32, r64) in _modes(D).items():
        for P in R.PAIRS:
            (xa, xb, spa, spb), (sa, sb, ia, ib) = _operands(args, P, device)
            plan = ops.map_plan(sa, sb, ia, ib)
            with _lib.kernel_timer() as kt, torch.no_grad():
                pm = ops.pair_map(xa, xb, spa, spb, plan)
            assert [(n, g) for n, g, _ in kt.records()] == [("k_pair_map", -(-plan.n_items // 4))], "one launch, one wave per item"
            with torch.no_grad():
                f_out, f_arg = ops.pair_pool_gather(xa, xb, spa, spb, ia, ib, return_argmax=True)
            got, what = R.as_host(pm), f"D={D} P={P} {mode}"
            p32, p64 = R.prefix(r32, P), R.prefix(r64, P)
            R.assert_parity(got, p64, p32, what)
            R.assert_fills(got, p64, what)
            R.assert_ties_back(got, p64, p32, f_out, f_arg, what)
            for k in ("max1", "mean1", "max2", "mean2"):      # values depend neither on the mode nor on the other pairs of the call
                assert torch.equal(getattr(got, k), _cut(full, k, P)), f"{what}: {k} differs from the slices of the full indexed call"


def _cut(full, k, P):
    return getattr(full, k)[:int((full.out_ptr1 if k.endswith("1") else full.out_ptr2)[P])]


@pytest.mark.parametrize("D", [8, 15, 45])
def test_maps_ties_go_to_the_smallest_row(device, D):
    """Small-integer rows (every score exact) with duplicated rows at 63 / 64 and 0 / 69 of the 70-row segment and on the small side:
    all six outputs against the fp64 brute force — 16-byte form (8) and dword form (15, 45), through swapping indices."""
    x1, x2 = R.tie_case(D)
    args = (x1, x2, R.TIE_SIZES1, R.TIE_SIZES2, R.TIE_IDX1, R.TIE_IDX2)
    r64 = R.restate(*args, torch.float64)
    assert (~r64.unique1).sum() > 5 and (~r64.unique2).sum() > 5, "the case must hold ties"
    with torch.no_grad():
        pm = ops.pair_map(x1.to(device), x2.to(device), _sp(R.TIE_SIZES1, device), _sp(R.TIE_SIZES2, device),
                          ops.map_plan(R.TIE_SIZES1, R.TIE_SIZES2, R.TIE_IDX1, R.TIE_IDX2))
    R.assert_exact(R.as_host(pm), r64, f"D={D}")


def test_maps_are_deterministic_and_independent_of_the_other_pairs(device):
    x1, x2 = R.random_case(60)
    d1, d2, sp1, sp2 = x1.to(device), x2.to(device), _sp(R.SIZES1, device), _sp(R.SIZES2, device)
    plan = ops.map_plan(R.SIZES1, R.SIZES2, R.IDX1, R.IDX2)
    sub = [7, 2, 4, 0]
    with torch.no_grad():
        a, b = ops.pair_map(d1, d2, sp1, sp2, plan), layer.dot_and_global_pool2_map(d1, d2, sp1, sp2, plan)
        part = ops.pair_map(d1, d2, sp1, sp2, ops.map_plan(R.SIZES1, R.SIZES2, [R.IDX1[i] for i in sub], [R.IDX2[i] for i in sub]))
    assert _equal(a, b), "two runs differ"
    a, part = R.as_host(a), R.as_host(part)
    for j, i in enumerate(sub):
        for k in R.FIELDS:
            pa, pp = (a.out_ptr1, part.out_ptr1) if k.endswith("1") else (a.out_ptr2, part.out_ptr2)
            assert torch.equal(getattr(part, k)[pp[j]:pp[j + 1]], getattr(a, k)[pa[i]:pa[i + 1]]), f"pair {i}: {k} depends on the other pairs"


def test_maps_empty_sides_and_no_pairs(device):
    """An empty partner: ``0, -1, 0`` on every row of the other side; an empty side has no rows; a matrix without any row; ``P = 0``
    launches nothing."""
    s1, s2, i1, i2 = [3, 0, 70], [0, 6], [0, 1, 2, 1, 2], [1, 1, 0, 0, 1]
    g = torch.Generator().manual_seed(0)
    x1, x2 = torch.randn(sum(s1), 60, generator=g), torch.randn(sum(s2), 60, generator=g)
    r32, r64 = (R.restate(x1, x2, s1, s2, i1, i2, dt) for dt in (torch.float32, torch.float64))
    d1, d2, sp1, sp2 = x1.to(device), x2.to(device), _sp(s1, device), _sp(s2, device)
    with torch.no_grad():
        got = R.as_host(ops.pair_map(d1, d2, sp1, sp2, ops.map_plan(s1, s2, i1, i2)))
    R.assert_parity(got, r64, r32, "empty sides")
    R.assert_fills(got, r64, "empty sides")
    assert got.out_ptr1.tolist() == [0, 3, 3, 73, 73, 143] and got.out_ptr2.tolist() == [0, 6, 12, 12, 12, 18]
    assert (got.arg1[3:73] == -1).all() and (got.max1[3:73] == 0).all() and (got.arg2[6:12] == -1).all()
    # every owner row of the call sits on ONE side, in matrices that both hold rows: the other side's outputs are empty, the fills are launched
    for j1, j2, side, rows in (([0, 2], [0, 0], 1, 73), ([1], [1], 2, 6), ([1, 1], [1, 1], 2, 12)):
        plan = ops.map_plan(s1, s2, j1, j2)
        assert (plan.R1, plan.R2) == ((rows, 0) if side == 1 else (0, rows)) and plan.n_items > 0
        with _lib.kernel_timer() as kt, torch.no_grad():
            pm = ops.pair_map(d1, d2, sp1, sp2, plan)
        assert [(n, g) for n, g, _ in kt.records()] == [("k_pair_map", -(-plan.n_items // 4))]
        one = R.as_host(pm)
        R.assert_fills(one, R.restate(x1, x2, s1, s2, j1, j2, torch.float64), f"one-sided {j1} {j2}")
        mx, arg, mean = (getattr(one, f"{k}{side}") for k in ("max", "arg", "mean"))
        assert mx.shape == (rows,) and (mx == 0).all() and (mean == 0).all() and (arg == -1).all()
        assert all(getattr(one, f"{k}{3 - side}").shape == (0,) for k in ("max", "arg", "mean"))
    # the second matrix has no row at all
    none = torch.zeros(0, 60, device=device)
    no_row = ops.SegmentPtr.from_parts(torch.zeros(3, dtype=torch.int32, device=device), 0, 2)      # two segments, no row
    with torch.no_grad():
        got = R.as_host(ops.pair_map(d1, none, sp1, no_row, ops.map_plan(s1, [0, 0], i1, i2)))
    assert got.max2.numel() == 0 and got.max1.shape == (143,) and (got.max1 == 0).all() and (got.mean1 == 0).all() and (got.arg1 == -1).all()
    with _lib.kernel_timer() as kt, torch.no_grad():
        pm = ops.pair_map(d1, d2, sp1, sp2, ops.map_plan(s1, s2, [], []))
    assert kt.records() == [], "P = 0 launched something"
    assert all(getattr(pm, k).shape == (0,) for k in R.FIELDS) and pm.out_ptr1.tolist() == [0] == pm.out_ptr2.tolist()


def test_maps_refusals_come_before_any_launch(device):
    s1, s2, ok1, ok2 = [3, 4, 2], [5, 6], [0, 2, 1, 1], [1, 0, 0, 1]
    x1, x2 = torch.randn(sum(s1), 60, device=device), torch.randn(sum(s2), 60, device=device)
    wide1, wide2 = torch.randn(sum(s1), 129, device=device), torch.randn(sum(s2), 129, device=device)
    sp1, sp2 = _sp(s1, device), _sp(s2, device)
    plan = ops.map_plan(s1, s2, ok1, ok2)
    with _lib.kernel_timer() as kt, torch.no_grad():
        with torch.enable_grad(), pytest.raises(GlamHipError, match="inference only.*no_grad.*ops.pair_pool"):
            ops.pair_map(x1.clone().requires_grad_(True), x2, sp1, sp2, plan)
        with torch.enable_grad(), pytest.raises(GlamHipError, match="inference only.*no_grad.*ops.pair_pool"):
            ops.pair_map(x1, x2.clone().requires_grad_(True), sp1, sp2, plan)
        with pytest.raises(GlamHipError, match="the plan was made for"):         # other sizes, the same counts
            ops.pair_map(x1, x2, sp1, sp2, ops.map_plan([3, 4, 3], s2, ok1, ok2))
        with pytest.raises(GlamHipError, match="the plan was made for"):         # another segment count
            ops.pair_map(x1, x2, sp1, sp2, ops.map_plan(s1, [5, 4, 2], ok1, ok2))
        with pytest.raises(GlamHipError, match="ops.map_plan"):
            ops.pair_map(x1, x2, sp1, sp2, plan.work)
        with pytest.raises(GlamHipError, match="129"):
            ops.pair_map(wide1, wide2, sp1, sp2, plan)
        with pytest.raises(GlamHipError, match="disagree"):                      # a width mismatch
            ops.pair_map(x1, x2[:, :56], sp1, sp2, plan)
        with pytest.raises(GlamHipError, match="idx2 lives on a device.*read-back"):
            ops.map_plan(s1, s2, ok1, torch.tensor(ok2, device=device))
        with pytest.raises(GlamHipError, match="sizes of side 1 live on a device"):
            ops.map_plan(torch.tensor(s1, device=device), s2, ok1, ok2)
        with pytest.raises(IndexError):
            ops.map_plan(s1, s2, ok1, [1, 2, 0, 1])
    assert kt.records() == [], "a refusal launched something"
    raw = _lib.load()
    assert raw.glam_pair_map_fwd(*[None] * 5, 4, 129, *[None] * 7) == _lib.GLAM_E_UNSUPPORTED
    assert raw.glam_pair_map_fwd(*[None] * 5, 4, 60, *[None] * 7) == _lib.GLAM_E_INVALID and b"null pointer" in raw.glam_last_error()
    assert raw.glam_pair_map_fwd(*[None] * 5, 0, 60, *[None] * 7) == 0
    with _lib.kernel_timer() as kt, torch.enable_grad():       # grad mode alone is fine: nothing here requires grad
        assert ops.pair_map(x1, x2, sp1, sp2, plan).max1.shape == (3 + 2 + 4 + 4,)
    assert [n for n, _, _ in kt.records()] == ["k_pair_map"]


# ---------------------------------------------------------------------------------------------
# explain.explain_pair
# ---------------------------------------------------------------------------------------------
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU")
_IDX = [0, 1, 1, 0, 1, 1]
_FIRST = [0, 1, 1, 4, 3, 1, 0, 4, 1]
_SECOND = [2, 1, 0, 4, 1, 3, 2, 0, 2]


def _dti(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDTI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **_ACTS, **kw).eval()


def _ddi(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDDI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **_ACTS, **kw).eval()


def _proteins(n, seed=4):
    rng = np.random.default_rng(seed)
    return [synth_protein(rng, 40, 130) for _ in range(n)]


def _drugs(n=6, seed=5):
    rng = np.random.default_rng(seed)
    return [synth_molecule(rng) for _ in range(n)]


def _sizes(sp):
    p = sp.ptr.cpu().numpy().astype(np.int64)
    return p[1:] - p[:-1]


def _spy(monkeypatch, name, seen):
    """Keep the operands and the result of every call of ``model.<name>`` (the fusion of ``screen`` / ``score_pairs``)."""
    inner = getattr(model, name)

    def f(*a, **k):
        r = inner(*a, **k)
        seen.append((a[0].detach().clone(), a[1].detach().clone(), r))
        return r
    monkeypatch.setattr(model, name, f)


def _check_explanation(ex, out, contacts, seen, sp1, sp2, plan, steps=2):
    assert torch.equal(ex.out, out) and len(ex.contacts) == len(contacts) == steps
    assert all(torch.equal(a, b) and a.dtype == torch.int32 for a, b in zip(ex.contacts, contacts))
    assert torch.equal(ex.fusion, torch.cat([r[0] for _, _, r in seen], dim=1)) and ex.fusion.shape == (plan.P, 2 * steps)
    assert len(ex.maps) == steps and ex.ptr1.tolist() == plan.out_ptr1.tolist() and ex.ptr2.tolist() == plan.out_ptr2.tolist()
    for s, (xa, xb, (f, arg)) in enumerate(seen):
        direct = ops.pair_map(xa, xb, sp1, sp2, plan)
        assert _equal(ex.maps[s], direct), f"step {s}: the maps differ from ops.pair_map on the step's rows"
        best = torch.stack([t.max() for t in ex.per_pair(ex.maps[s].max1, 1)])
        assert torch.equal(best, f[:, 0]) and torch.equal(torch.stack([t.max() for t in ex.per_pair(ex.maps[s].max2, 2)]), f[:, 0])
    assert ex.weights(1) is ex.maps[-1].max1 and ex.weights(2, "mean", 0) is ex.maps[0].mean2
    assert [t.numel() for t in ex.per_pair(ex.weights(2), 2)] == np.diff(plan.out_ptr2).tolist()
    with pytest.raises(ValueError):
        ex.weights(1, "median")
    with pytest.raises(ValueError):
        ex.per_pair(ex.maps[0].max1, 3)


@pytest.mark.parametrize("form", ["encoding", "batch"])
def test_explain_pair_dti(device, monkeypatch, form):
    mb, pros = synth_batch(6, seed=3).to(device), _proteins(2)
    net = _dti().to(device)
    seen = []
    with torch.no_grad():
        if form == "encoding":
            enc = net.encode_proteins(Batch.from_data_list(pros).to(device))
            ex = explain.explain_pair(net, mb, enc, _IDX)
            idx = _IDX
        else:
            pb = Batch.from_data_list([pros[q] for q in _IDX]).to(device)
            ex = explain.explain_pair(net, mb, pb)
            enc, idx = net.encode_proteins(pb), list(range(6))
        _spy(monkeypatch, "dot_and_global_pool2_indexed", seen)
        out, contacts = net.screen(mb, enc, idx, return_argmax=True)
        msp = ops.segment_ptr(mb.batch, mb.num_graphs)
        _check_explanation(ex, out, contacts, seen, msp, enc.sp, ops.map_plan(_sizes(msp), _sizes(enc.sp), None, idx))


def test_explain_pair_ddi(device, monkeypatch):
    net = _ddi().to(device)
    seen = []
    with torch.no_grad():
        enc = net.encode_drugs(Batch.from_data_list(_drugs()).to(device))
        ex = explain.explain_pair(net, enc, _FIRST, np.asarray(_SECOND))
        _spy(monkeypatch, "dot_and_global_pool2_gather", seen)
        out, contacts = net.score_pairs(enc, _FIRST, _SECOND, return_argmax=True)
        _check_explanation(ex, out, contacts, seen, enc.sp, enc.sp, ops.map_plan(_sizes(enc.sp), _sizes(enc.sp), _FIRST, _SECOND))


def test_explain_pair_refusals(device):
    mb, pb = synth_batch(6, seed=3).to(device), Batch.from_data_list(_proteins(2)).to(device)
    drugs = Batch.from_data_list(_drugs()).to(device)
    dti, ddi = _dti().to(device), _ddi().to(device)
    with torch.no_grad():
        enc, denc = dti.encode_proteins(pb), ddi.encode_drugs(drugs)
        with _lib.kernel_timer() as kt:
            dti.train(), ddi.train()
            for call in (lambda: explain.explain_pair(dti, mb, enc, _IDX), lambda: explain.explain_pair(dti, mb, pb),
                         lambda: explain.explain_pair(ddi, denc, _FIRST, _SECOND)):
                with pytest.raises(GlamHipError, match="explain_pair: the model is in training mode"):
                    call()
            dti.eval(), ddi.eval()
            with pytest.raises(GlamHipError, match="explain_pair: pro_flat's norm _LayerNorm"):
                explain.explain_pair(_dti(flat_norm="_LayerNorm").to(device), mb, pb)
            with pytest.raises(GlamHipError, match="explain_pair: mol1_conv's norm _GraphSizeNorm"):
                explain.explain_pair(_ddi(graph_norm="_GraphSizeNorm").to(device), denc, _FIRST, _SECOND)
            with pytest.raises(GlamHipError, match="two collated batches are not taken.*encode_drugs"):
                explain.explain_pair(ddi, drugs, drugs)
            with pytest.raises(GlamHipError, match="another model"):
                explain.explain_pair(_dti().to(device), mb, enc, _IDX)
            for stray in (denc, _IDX, None):                                     # neither a ProteinEncoding nor a batch of graphs
                with pytest.raises(GlamHipError, match="explain_pair: for an ArchitectureDTI the call is .*encode_proteins"):
                    explain.explain_pair(dti, mb, stray)
            with pytest.raises(IndexError, match=r"second must lie in \[0, 6\)"):
                explain.explain_pair(ddi, denc, _FIRST, [6] * 9)
            with pytest.raises(GlamHipError, match="ArchitectureDTI or ArchitectureDDI"):
                explain.explain_pair(torch.nn.Linear(2, 2), mb, enc)
            for net in (dti, ddi):
                with pytest.raises(GlamHipError, match="explain_pair"):
                    explain.explain(net, mb)
        assert kt.records() == [], "a refusal launched something"
    with pytest.raises(GlamHipError, match="no_grad"):
        explain.explain_pair(dti, mb, enc, _IDX)
