"""GPU (MI355X): the DDI interaction matrix — the second-side-stationary fusion with packed chunks (``glam_pair_pool_grid_fwd``:
csrc/pairgrid.hip) and ``ArchitectureDDI.score_matrix`` on top of it.

The property everything rests on: entry ``[i, j]`` of the grid is ``ops.pair_pool_gather`` on the pair ``(rows[i], cols[j])`` — the max
column and the argmax bit for bit (one ascending fmaf chain per score, ties to the smallest flattened index OF THE LANE'S OWN DRUG: a
total order, so neither the packing nor the slab can show), the whole ``[max, mean]`` within the fp64-twin bound of the oracle on
physically gathered rows, and for ``rows=None`` the bits of ``ops.pair_pool_panel`` (the same mean chain).  ``score_matrix`` is then
checked column by column against ``score_pairs`` and against the oracle's two-drug model on the expanded batches."""
import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, layer, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, Data, _mol_arrays
from tests.conftest import assert_twin_parity
from tests.test_gpu_ddi_pairs import _batch, _net, _oracle_ddi

pytestmark = pytest.mark.gpu

_S1 = [1, 2, 33, 0, 7]                                        # a lone row, one row pair, an odd last row, an empty drug
_S2 = [20, 20, 20, 20, 63, 1, 64, 65, 130, 0, 5]              # the packing case of tests/test_ddi_matrix_host.py
_ROWS = [2, 0, 4, 2, 3, 1]
_COLS = [8, 0, 0, 5, 9, 2]


def _ptr(sizes):
    return [0] + list(np.cumsum(sizes))


_CASES = {}


def _case(D, device):
    """Inputs of width ``D`` and their references, computed ONCE and shared (never written): ``ops.pair_pool_gather`` over all 5 x 11
    pairs, and the oracle in fp32 / fp64 on physically gathered rows of every non-empty pair."""
    if D not in _CASES:
        torch.manual_seed(D)
        Q1, Q2 = len(_S1), len(_S2)
        b1, b2 = _batch(_S1), _batch(_S2)
        x1, x2 = torch.randn(b1.numel(), D), torch.randn(b2.numel(), D)
        sp1, sp2 = ops.SegmentPtr(b1.to(device), Q1), ops.SegmentPtr(b2.to(device), Q2)
        d1, d2 = x1.to(device), x2.to(device)
        idx1, idx2 = np.repeat(np.arange(Q1), Q2), np.tile(np.arange(Q2), Q1)
        with torch.no_grad():
            ref, ref_arg = ops.pair_pool_gather(d1, d2, sp1, sp2, idx1, idx2, return_argmax=True)
        o1, o2 = _ptr(_S1), _ptr(_S2)
        live = [(a, q) for a in range(Q1) for q in range(Q2) if _S1[a] and _S2[q]]
        g1 = torch.cat([x1[o1[a]:o1[a + 1]] for a, _ in live])
        g2 = torch.cat([x2[o2[q]:o2[q + 1]] for _, q in live])
        gb1, gb2 = _batch([_S1[a] for a, _ in live]), _batch([_S2[q] for _, q in live])
        twin = {}
        for dt in (torch.float32, torch.float64):
            o = O.dot_and_global_pool(g1.to(dt), g2.to(dt), gb1, gb2, len(live), 2)
            full = torch.zeros(Q1, Q2, 2, dtype=dt)                       # (an empty drug on either side: 0, 0)
            for (a, q), row in zip(live, o):
                full[a, q] = row
            twin[dt] = full
        _CASES[D] = dict(x1=d1, x2=d2, sp1=sp1, sp2=sp2, ref=ref.view(Q1, Q2, 2), ref_arg=ref_arg.view(Q1, Q2, 2), twin=twin)
    return _CASES[D]


@pytest.mark.parametrize("cols", [None, _COLS], ids=["all cols", "picked cols"])
@pytest.mark.parametrize("rows", [None, _ROWS], ids=["all rows", "picked rows"])
@pytest.mark.parametrize("D", [4, 15, 16, 60, 64, 92, 128])
def test_grid_fusion_equals_the_gathered_call_pair_by_pair(device, D, rows, cols):
    """16-byte loads (4, 16, 60, 64, 92, 128) and dword loads (15); every slab gives the bits of the automatic one; two runs agree."""
    c = _case(D, device)
    plan = ops.grid_plan(_S2, cols)
    ri, ci = list(range(len(_S1))) if rows is None else rows, list(range(len(_S2))) if cols is None else cols
    R, Cs = len(ri), len(ci)
    ref_out, ref_arg = c["ref"][ri][:, ci], c["ref_arg"][ri][:, ci]
    args = (c["x1"], c["x2"], c["sp1"], c["sp2"], plan, rows)
    with torch.no_grad():
        out, arg = ops.pair_pool_grid(*args, return_argmax=True)
        out2, arg2 = ops.pair_pool_grid(*args, return_argmax=True)
        plain = ops.pair_pool_grid(*args)                                  # (argmax = NULL in the kernel)
    assert out.shape == (R, Cs, 2) and arg.shape == out.shape and arg.dtype == torch.int32
    assert torch.equal(out, out2) and torch.equal(arg, arg2) and torch.equal(out, plain), "two runs differ"
    assert torch.equal(out[..., 0], ref_out[..., 0]), "max column differs from pair_pool_gather"
    assert torch.equal(arg, ref_arg), "argmax differs from pair_pool_gather"
    assert_twin_parity(lambda dt: (c["twin"][dt][ri][:, ci], []), out, [], f"pair_pool_grid D={D}")
    sum1, sum2 = ops.segment_pool(c["x1"], c["sp1"], "sum"), ops.segment_pool(c["x2"], c["sp2"], "sum")
    with torch.no_grad():
        for slab in (0, 1, 4, R + 3):
            o, a = ops.pair_pool_grid(*args, sum1, sum2, return_argmax=True, slab=slab)
            assert torch.equal(o, out) and torch.equal(a, arg), f"slab={slab} changes the bits"
        if rows is None:                     # the panel over the same selection: the same score chain AND the same mean chain
            po, pa = ops.pair_pool_panel(c["x1"], c["x2"], c["sp1"], c["sp2"], ops.panel_plan(_S2, cols), return_argmax=True)
            assert torch.equal(out, po) and torch.equal(arg, pa), "differs from pair_pool_panel"
    if cols is not None:                     # the duplicated drug: two columns, the same bits
        assert torch.equal(out[:, 1], out[:, 2]) and torch.equal(arg[:, 1], arg[:, 2])
    if rows is not None:
        assert torch.equal(out[0], out[3]) and torch.equal(arg[0], arg[3])


def test_grid_fusion_through_the_layer_and_on_misaligned_rows(device):
    """``layer.dot_and_global_pool2_grid`` is the op; rows that start off a 16-byte boundary (D % 4 == 0) take the dword kernel: same bits."""
    c = _case(60, device)
    plan = ops.grid_plan(_S2, [1, 7, 2])
    shifted = torch.empty(c["x2"].numel() + 1, device=device)[1:].view_as(c["x2"]).copy_(c["x2"])
    assert shifted.data_ptr() % 16 == 4
    with torch.no_grad():
        out, arg = ops.pair_pool_grid(c["x1"], c["x2"], c["sp1"], c["sp2"], plan, _ROWS, return_argmax=True)
        via_layer = layer.dot_and_global_pool2_grid(c["x1"], c["x2"], c["sp1"], c["sp2"], plan, _ROWS)
        o2, a2 = ops.pair_pool_grid(c["x1"], shifted, c["sp1"], c["sp2"], plan, ops.pair_index(_ROWS, 6, 5, name="rows", over="drugs"),
                                    return_argmax=True)
    assert torch.equal(out, via_layer)
    assert torch.equal(o2[..., 0], out[..., 0]) and torch.equal(a2, arg)
    assert torch.equal(out[..., 0], c["ref"][_ROWS][:, [1, 7, 2], 0])


@pytest.mark.parametrize("D", [8, 15, 45])
def test_grid_fusion_ties_route_to_the_first_flattened_pair_of_the_lanes_own_drug(device, D):
    """The ties case of ``test_gpu_ddi_pairs.py`` on packed neighbours.  Small-integer rows (every dot product exact), every first-side row
    with a twin; the second-side drugs of 6, 5 and 4 rows share the last chunk, the first two holding the SAME duplicated rows (a tie
    across neighbours must not cross: each drug's argmax is its own first occurrence), and the 70-row drug holds duplicates in both of
    its slices — 16-byte (8) and dword (15, 45) loads, through a swapping selection."""
    s1, s2, rows, cols = [4, 3, 5], [5, 6, 70, 4], [1, 0, 2], [2, 1, 0, 3]
    b1, b2 = _batch(s1), _batch(s2)
    g = torch.Generator().manual_seed(D)
    x1 = torch.randint(-1, 2, (b1.numel(), D), generator=g).float()
    x2 = torch.randint(-1, 2, (b2.numel(), D), generator=g).float()
    for a, b in [(3, 0), (2, 1), (5, 4), (6, 4), (9, 7), (10, 8), (11, 7)]:      # every first-side row has a twin: every score occurs twice
        x1[a] = x1[b]
    for a, b in [(1, 0), (3, 2), (11 + 69, 11 + 0), (11 + 65, 11 + 3), (11 + 64, 11 + 63), (81 + 3, 81 + 1)]:
        x2[a] = x2[b]
    x2[5:10] = x2[0:5]                                                           # drug 1 = drug 0 and one row more: packed neighbours that tie
    sp1, sp2 = ops.SegmentPtr(b1.to(device), 3), ops.SegmentPtr(b2.to(device), 4)
    plan = ops.grid_plan(s2, cols)
    assert plan.lanes[0, 0, 3] == 0 and plan.lanes[1, 5, 3] == 1 and plan.lanes[2, 0, 3] == 2, "70 rows: two slices, then a packed chunk"
    assert plan.lanes[2, :15, 3].tolist() == [2] * 6 + [3] * 5 + [4] * 4
    o1, o2 = _ptr(s1), _ptr(s2)
    with torch.no_grad():
        for slab in (0, 1):
            out, arg = ops.pair_pool_grid(x1.to(device), x2.to(device), sp1, sp2, plan, rows, return_argmax=True, slab=slab)
            for i, a in enumerate(rows):
                for j, q in enumerate(cols):
                    S = x1[b1 == a].double() @ x2[b2 == q].double().T
                    flat = S.reshape(-1)
                    first = int((flat == flat.max()).nonzero()[0])
                    assert (flat == flat.max()).sum() > 1, "the case must hold a tie"
                    assert out[i, j, 0].item() == flat[first].item()
                    assert arg[i, j].tolist() == [o1[a] + first // s2[q], o2[q] + first % s2[q]]
                    assert abs(out[i, j, 1].item() - S.mean().item()) <= 1e-6
        ref, ref_arg = ops.pair_pool_gather(x1.to(device), x2.to(device), sp1, sp2, np.repeat(rows, 4), np.tile(cols, 3), return_argmax=True)
    assert torch.equal(out[..., 0], ref.view(3, 4, 2)[..., 0]) and torch.equal(arg, ref_arg.view(3, 4, 2))


def test_grid_fusion_does_not_leak_between_packed_neighbours(device):
    """Three drugs fill the 64 lanes of one chunk; the rows of the middle one are scaled by 100, so that its scores dominate every
    unsegmented reduction: its neighbours' maxima and contacts still equal ``pair_pool_gather``'s."""
    torch.manual_seed(5)
    s1, s2 = [9, 14, 3], [20, 24, 20]
    b1, b2 = _batch(s1), _batch(s2)
    x1, x2 = torch.randn(b1.numel(), 60, device=device), torch.randn(b2.numel(), 60, device=device)
    x2[20:44] *= 100
    sp1, sp2 = ops.SegmentPtr(b1.to(device), 3), ops.SegmentPtr(b2.to(device), 3)
    plan = ops.grid_plan(s2, None)
    assert plan.total_chunks == 1 and plan.fill == 1.0
    with torch.no_grad():
        out, arg = ops.pair_pool_grid(x1, x2, sp1, sp2, plan, return_argmax=True)
        ref, ref_arg = ops.pair_pool_gather(x1, x2, sp1, sp2, np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3), return_argmax=True)
    assert torch.equal(out[..., 0], ref.view(3, 3, 2)[..., 0]) and torch.equal(arg, ref_arg.view(3, 3, 2))
    assert (out[:, 1, 0] > 10 * out[:, [0, 2], 0].max()).all(), "the case must hold a dominating neighbour"
    a = arg.cpu()
    assert ((a[:, 0, 1] < 20) & (a[:, 1, 1] >= 20) & (a[:, 1, 1] < 44) & (a[:, 2, 1] >= 44)).all()


def test_grid_fusion_empty_segments_and_empty_tables(device):
    """70 one-row drugs (64 runs in one chunk); an empty drug on either side: ``0, 0`` and ``arg = -1``; a selection of empty drugs alone
    has no chunk and still writes; ``R == 0`` / ``Cs == 0`` / a side without a row return without a launch."""
    torch.manual_seed(0)
    ones = [1] * 70
    x1, x2 = torch.randn(8, 60, device=device), torch.randn(70, 60, device=device)
    sp1, sp2 = ops.SegmentPtr(_batch([3, 0, 5]).to(device), 3), ops.SegmentPtr(_batch(ones).to(device), 70)
    with torch.no_grad():
        out, arg = ops.pair_pool_grid(x1, x2, sp1, sp2, ops.grid_plan(ones), return_argmax=True)
        ref, ref_arg = ops.pair_pool_gather(x1, x2, sp1, sp2, np.repeat(np.arange(3), 70), np.tile(np.arange(70), 3), return_argmax=True)
        assert torch.equal(out[..., 0], ref.view(3, 70, 2)[..., 0]) and torch.equal(arg, ref_arg.view(3, 70, 2))
        assert out[1].abs().max().item() == 0.0 and (arg[1] == -1).all()
        assert torch.equal(arg[0, :, 1].cpu(), torch.arange(70, dtype=torch.int32)), "a one-row drug's contact is its row"
        ps = [0, 6]
        y2 = torch.randn(6, 60, device=device)
        tp2 = ops.SegmentPtr(_batch(ps).to(device), 2)
        out, arg = ops.pair_pool_grid(x1, y2, sp1, tp2, ops.grid_plan(ps), return_argmax=True)
        assert out[1].abs().max().item() == 0.0 and out[:, 0].abs().max().item() == 0.0 and (arg[1] == -1).all() and (arg[:, 0] == -1).all()
        assert abs(out[0, 1, 0].item() - (x1[:3] @ y2.T).max().item()) <= 1e-4 and abs(out[2, 1, 1].item() - (x1[3:] @ y2.T).mean().item()) <= 1e-5
        assert 0 <= arg[0, 1, 0].item() < 3 and 3 <= arg[2, 1, 0].item() < 8 and 0 <= arg[2, 1, 1].item() < 6
        none, none_arg = ops.pair_pool_grid(x1, y2, sp1, tp2, ops.grid_plan(ps, [0, 0]), return_argmax=True)
        assert none.shape == (3, 2, 2) and none.abs().max().item() == 0.0 and (none_arg == -1).all()
        with _lib.kernel_timer() as kt:
            e, ea = ops.pair_pool_grid(x1, y2, sp1, tp2, ops.grid_plan(ps, []), return_argmax=True)
            assert e.shape == (3, 0, 2) and ea.shape == (3, 0, 2) and ea.dtype == torch.int32
            assert ops.pair_pool_grid(x1, y2, sp1, tp2, ops.grid_plan(ps), rows=[]).shape == (0, 2, 2)
            no_seg = ops.SegmentPtr.from_parts(torch.zeros(1, dtype=torch.int32, device=device), 0, 0)
            assert ops.pair_pool_grid(torch.empty(0, 60, device=device), y2, no_seg, tp2, ops.grid_plan(ps)).shape == (0, 2, 2)
            no_row = ops.SegmentPtr.from_parts(torch.zeros(3, dtype=torch.int32, device=device), 0, 2)      # two drugs, no row
            z, za = ops.pair_pool_grid(torch.empty(0, 60, device=device), y2, no_row, tp2, ops.grid_plan(ps), return_argmax=True)
            assert z.shape == (2, 2, 2) and z.abs().max().item() == 0.0 and (za == -1).all()
            z, za = ops.pair_pool_grid(x1, torch.empty(0, 60, device=device), sp1, no_row, ops.grid_plan([0, 0]), return_argmax=True)
            assert z.shape == (3, 2, 2) and z.abs().max().item() == 0.0 and (za == -1).all()
        assert kt.records() == [], "an empty table launched something"


def test_grid_fusion_refusals_come_before_any_launch(device):
    s1, s2 = [3, 4, 2], [5, 6]
    b1, b2 = _batch(s1), _batch(s2)
    x1, x2 = torch.randn(b1.numel(), 60, device=device), torch.randn(b2.numel(), 60, device=device)
    sp1, sp2 = ops.SegmentPtr(b1.to(device), 3), ops.SegmentPtr(b2.to(device), 2)
    plan = ops.grid_plan(s2, [1, 0, 1])
    with _lib.kernel_timer() as kt, torch.no_grad():
        for bad in ([0, 2], [-1], [0.5]):
            with pytest.raises(IndexError):
                ops.grid_plan(s2, bad)
        with pytest.raises(GlamHipError, match="read-back"):
            ops.grid_plan(s2, torch.tensor([0, 1], device=device))
        with pytest.raises(GlamHipError, match="ops.grid_plan"):
            ops.pair_pool_grid(x1, x2, sp1, sp2, [1, 0, 1])
        with pytest.raises(GlamHipError, match="ops.grid_plan"):
            ops.pair_pool_grid(x1, x2, sp1, sp2, ops.panel_plan(s2, [1, 0, 1]))
        for bad in ([0, 3], [-1, 0]):
            with pytest.raises(IndexError, match=r"rows must lie in \[0, 3\)"):
                ops.pair_pool_grid(x1, x2, sp1, sp2, plan, bad)
        with pytest.raises(GlamHipError, match="rows lives on a device.*read-back"):
            ops.pair_pool_grid(x1, x2, sp1, sp2, plan, torch.tensor([0, 1], device=device))
        with torch.enable_grad(), pytest.raises(GlamHipError, match=r"ops\.pair_pool .*ops\.pair_pool_gather_shared"):
            ops.pair_pool_grid(x1.clone().requires_grad_(True), x2, sp1, sp2, plan)
        with torch.enable_grad(), pytest.raises(GlamHipError, match=r"ops\.pair_pool .*ops\.pair_pool_gather_shared"):
            ops.pair_pool_grid(x1, x2.clone().requires_grad_(True), sp1, sp2, plan)
        with pytest.raises(GlamHipError, match="the plan was made for"):
            ops.pair_pool_grid(x1, x2, sp1, sp2, ops.grid_plan([5, 6, 7], None))
        with pytest.raises(GlamHipError, match="the plan was made for"):
            ops.pair_pool_grid(x1, x2, sp1, sp2, ops.grid_plan([5, 7], None))
        with pytest.raises(GlamHipError, match="disagree"):
            ops.pair_pool_grid(x1[:, :56], x2, sp1, sp2, plan)
        with pytest.raises(GlamHipError, match="disagree"):
            ops.pair_pool_grid(x1[:-1], x2, sp1, sp2, plan)
        with pytest.raises(GlamHipError, match="disagree"):
            ops.pair_pool_grid(x1, x2[:-1], sp1, sp2, plan)
        with pytest.raises(GlamHipError, match="sum1 must be"):
            ops.pair_pool_grid(x1, x2, sp1, sp2, plan, sum1=torch.zeros(3, 59, device=device))
        with pytest.raises(GlamHipError, match="sum2 must be"):
            ops.pair_pool_grid(x1, x2, sp1, sp2, plan, sum2=torch.zeros(3, 60, device=device))
        with pytest.raises(GlamHipError, match="slab"):
            ops.pair_pool_grid(x1, x2, sp1, sp2, plan, slab=-1)
        wide1, wide2 = torch.zeros(b1.numel(), 132, device=device), torch.zeros(b2.numel(), 132, device=device)
        with pytest.raises(GlamHipError, match="width 132 is outside the kernel table"):
            ops.pair_pool_grid(wide1, wide2, sp1, sp2, plan)
    assert kt.records() == [], "a refusal launched something"
    with _lib.kernel_timer() as kt, torch.enable_grad():                   # grad mode alone is fine: nothing here requires grad
        sums = ops.segment_pool(x1, sp1, "sum"), ops.segment_pool(x2, sp2, "sum")
    with _lib.kernel_timer() as kt, torch.enable_grad():
        assert ops.pair_pool_grid(x1, x2, sp1, sp2, plan, None, *sums).shape == (3, 3, 2)
    assert [(n, g) for n, g, _ in kt.records()] == [("k_pair_grid", 1), ("k_pair_grid_finish", 1)], "one chunk block, one finish block"


# ---------------------------------------------------------------------------------------------
# ArchitectureDDI.score_matrix
# ---------------------------------------------------------------------------------------------
_ATOMS = [1, 70, 12, 28, 3, 40, 20, 65, 17]      # nine drugs of 1 .. 70 atoms: packed neighbours, two sliced drugs, a lone atom
_MROWS = [2, 0, 4, 2, 8, 1]                      # a duplicate
_MCOLS = [7, 1, 3, 0, 5]                         # out of order


def _drugs():
    rng = np.random.default_rng(11)
    out = []
    for n in _ATOMS:
        x, ei, ea = _mol_arrays(rng, n, n)
        out.append(Data(torch.from_numpy(x), torch.from_numpy(ei).reshape(2, -1), torch.from_numpy(ea), torch.zeros(1, 1)))
    return out


@pytest.mark.parametrize("kw", [dict(), dict(mol_readout="GlobalLAPool"), dict(hid_dim_alpha=1), dict(out_dim=3), dict(end_norm="_LayerNorm")],
                         ids=["default", "GlobalLAPool", "hid15", "out_dim3", "LayerNorm head"])
def test_score_matrix_vs_score_pairs_and_the_oracle(device, monkeypatch, kw):
    """Column ``j`` of ``score_matrix`` against ``score_pairs(enc, rows, [cols[j]] * R)`` — every step's fusion max bit-equal, the contacts
    equal — and against the oracle's two-drug model on the expanded batches: with a per-row head on the ``R * Cs`` pairs at once (its rows
    do not look at each other), with the batch-less ``_LayerNorm`` head column by column, which is how that head is DEFINED here.
    hid = 15 takes the dword kernel on compacted rows.  Head blocks of one row drug, the automatic block and one block agree."""
    drugs = _drugs()
    per_column = kw.get("end_norm", "_None") != "_None"
    net = _net(**kw)
    assert net._matrix_head_in_one_pass() is not per_column
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    R, Cs, out_dim = len(_MROWS), len(_MCOLS), kw.get("out_dim", 1)
    cast = lambda b, dt: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
    twin = {}

    def oracle(first, second, dt):
        sd = {k: v.to(dt) if v.is_floating_point() else v for k, v in sd0.items()}
        e1, e2 = Batch.from_data_list([drugs[q] for q in first]), Batch.from_data_list([drugs[q] for q in second])
        with torch.no_grad():
            return _oracle_ddi(sd, cast(e1, dt), cast(e2, dt), len(first), dt, "_NNConv", "_None", kw.get("mol_readout", "GlobalPool5"),
                               kw.get("end_norm", "_None"))

    def run(dt):                                               # the oracle's [R, Cs, out_dim], computed once per precision
        if dt not in twin:
            if per_column:
                twin[dt] = torch.stack([oracle(_MROWS, [c] * R, dt) for c in _MCOLS], 1)
            else:
                twin[dt] = oracle(np.repeat(_MROWS, Cs).tolist(), np.tile(_MCOLS, R).tolist(), dt).view(R, Cs, out_dim)
        return twin[dt], []
    net = net.to(device)
    net.graphed_call = False
    seen = {"grid": [], "pairs": []}

    def spy(name, key):
        inner = getattr(model, name)

        def f(*a, **k):
            r = inner(*a, **k)
            seen[key].append((r[0] if isinstance(r, tuple) else r).detach().clone())
            return r
        monkeypatch.setattr(model, name, f)
    spy("dot_and_global_pool2_gather", "pairs")
    spy("dot_and_global_pool2_grid", "grid")
    with torch.no_grad():
        enc = net.encode_drugs(Batch.from_data_list(drugs).to(device))
        assert enc.sizes_host is None and enc.sum1 is None and enc.sum2 is None and enc.plans == {}
        with _lib.kernel_timer() as kt:
            out, contacts = net.score_matrix(enc, _MROWS, _MCOLS, return_argmax=True)
        launches = [n for n, _, _ in kt.records() if n.startswith("k_pair_grid")]
        assert launches == ["k_pair_grid", "k_pair_grid_finish"] * 2, "one grid launch and one finish per step"
        assert out.shape == (R, Cs, out_dim) and len(contacts) == 2 and len(seen["grid"]) == 2
        assert all(c.shape == (R, Cs, 2) and c.dtype == torch.int32 for c in contacts)
        fusion = list(seen["grid"])
        sizes, sums, plan = enc.sizes_host, (enc.sum1, enc.sum2), enc.plans[tuple(_MCOLS)]
        assert sizes.tolist() == _ATOMS and len(enc.sum1) == len(enc.sum2) == 2
        for s in range(2):
            assert torch.equal(enc.sum1[s], ops.segment_pool(enc.rows1[s], enc.sp, "sum"))
            assert torch.equal(enc.sum2[s], ops.segment_pool(enc.rows2[s], enc.sp, "sum"))
        seg = enc.sp.ptr.cpu()
        for j, c in enumerate(_MCOLS):
            seen["pairs"].clear()
            o, cc = net.score_pairs(enc, _MROWS, [c] * R, return_argmax=True)
            for s in range(2):
                assert torch.equal(fusion[s][:, j, 0], seen["pairs"][s][:, 0]), f"step {s}, column {j}: the fusion max differs from score_pairs"
                assert torch.equal(contacts[s][:, j], cc[s]), f"step {s}, column {j}: the contacts differ from score_pairs"
                got = contacts[s][:, j].cpu()
                assert ((seg[_MROWS] <= got[:, 0]) & (got[:, 0] < seg[1:][_MROWS])).all() and ((seg[c] <= got[:, 1]) & (got[:, 1] < seg[c + 1])).all()
            if per_column:                                     # the per-column head IS that score_pairs call
                assert_twin_parity(lambda dt: (run(dt)[0][:, j], []), o, [], f"score_pairs, column {j}")
        what = f"score_matrix {kw}"
        assert_twin_parity(run, out, [], what)
        # the second call: no read-back, the same sums, the plan from the cache; the head blocks do not show in the fusion
        for block_pairs in (Cs, 0, 10 ** 9):
            seen["grid"].clear()
            again, con = net.score_matrix(enc, np.asarray(_MROWS), torch.tensor(_MCOLS), return_argmax=True, block_pairs=block_pairs)
            assert len(seen["grid"]) == 2 and all(torch.equal(a, b) for a, b in zip(seen["grid"], fusion)), f"block_pairs={block_pairs}: the fusion differs"
            assert all(torch.equal(a, b) for a, b in zip(con, contacts)), f"block_pairs={block_pairs}: the contacts differ"
            assert_twin_parity(run, again, [], f"{what} block_pairs={block_pairs}")
            assert enc.sizes_host is sizes and enc.sum1 is sums[0] and enc.sum2 is sums[1]
            assert list(enc.plans) == [tuple(_MCOLS)] and enc.plans[tuple(_MCOLS)] is plan
        assert torch.equal(again, net.score_matrix(enc, _MROWS, _MCOLS, block_pairs=10 ** 9)), "two runs differ"
        full = net.score_matrix(enc)                           # every drug against every drug: rows = NULL in the kernel
        assert full.shape == (9, 9, out_dim) and list(enc.plans) == [tuple(_MCOLS), None] and enc.sum1 is sums[0]
        if not per_column:
            assert_twin_parity(lambda dt: (run(dt)[0], []), full[_MROWS][:, _MCOLS], [], what + " (picked from the whole table)")
        assert net.score_matrix(enc, [], _MCOLS).shape == (0, Cs, out_dim) and net.score_matrix(enc, _MROWS, []).shape == (R, 0, out_dim)
        empty = net.score_matrix(enc, _MROWS, [], return_argmax=True)
        assert empty[0].abs().sum().item() == 0 and all(c.shape == (R, 0, 2) for c in empty[1])


def test_score_matrix_refusals_launch_nothing(device):
    drugs = Batch.from_data_list(_drugs()).to(device)
    net, other = _net().to(device), _net().to(device)
    with torch.no_grad():
        enc = net.encode_drugs(drugs)
        assert net.score_matrix(enc, [0, 1], [2]).shape == (2, 1, 1)
        with _lib.kernel_timer() as kt:
            with pytest.raises(GlamHipError, match="another model"):
                other.score_matrix(enc)
            with pytest.raises(IndexError, match=r"rows must lie in \[0, 9\)"):
                net.score_matrix(enc, [9])
            with pytest.raises(IndexError, match=r"cols must lie in \[0, 9\)"):
                net.score_matrix(enc, None, [0, 9])
            with pytest.raises(GlamHipError, match="cols lives on a device"):
                net.score_matrix(enc, None, torch.tensor([0], device=device))
            with pytest.raises(GlamHipError, match="block_pairs"):
                net.score_matrix(enc, block_pairs=-5)
            net.train()
            with pytest.raises(GlamHipError, match="training mode"):
                net.score_matrix(enc)
            net.eval()
            next(net.mol1_conv.parameters()).add_(1)
            with pytest.raises(GlamHipError, match="score_matrix: the encoding is stale"):
                net.score_matrix(enc)
        assert kt.records() == [], "a refusal launched something"
        assert net.score_matrix(net.encode_drugs(drugs), [0, 1], [2]).shape == (2, 1, 1)       # a fresh encoding is accepted again
    with pytest.raises(GlamHipError, match="no_grad"):
        net.score_matrix(enc)
