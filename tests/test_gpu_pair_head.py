"""GPU (MI355X): the factored pair head — ``ops.pair_head`` (``glam_pair_head_fwd``: csrc/pairhead.hip) and ``head="factored"`` of
``ArchitectureDDI.score_matrix`` / ``ArchitectureDTI.screen_panel`` with ``ArchitectureDDI.matrix_top`` on top of it.

The property everything rests on: over a table the head's first linear layer separates into a row part, a column part and the fusion
columns' part, and every entry of the result is ONE fixed chain of its own ``(flat_a[i], flat_b[j], f[i, j])`` — so the op sits within
the fp64-twin bound of the restatement (``tests/pair_head_restated.py``, shown equal to the listed head on the CPU), an entry's bits do
not depend on the table around it, and neither the pair rows nor the ``[pairs, e_dim]`` hidden matrix are ever allocated."""
import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch
from tests import hits_restated
from tests import pair_head_restated as H
from tests import test_gpu_panel as P
from tests.conftest import assert_fp32_parity, assert_twin_parity
from tests.test_gpu_ddi_matrix import _MCOLS, _MROWS, _drugs
from tests.test_gpu_ddi_pairs import _ACTS, _net, _oracle_ddi

pytestmark = pytest.mark.gpu

_KINDS = ("k_pair_head_side", "k_pair_head")


def _padded(t):
    """``t`` as a ``[n, C]`` view of rows padded to the next multiple of four columns (how odd hidden widths flow)."""
    wide = torch.zeros(t.size(0), (t.size(1) + 4) // 4 * 4, dtype=t.dtype, device=t.device)
    wide[:, :t.size(1)] = t
    return wide[:, :t.size(1)]


_REFS = {}


def _case(R, Cs, hid, e_dim, F, out_dim, act, slope):
    """fp64 inputs and the restatement in fp64 / fp32 on the CPU, computed ONCE per case and shared (never written)."""
    key = (R, Cs, hid, e_dim, F, out_dim, act, slope)
    if key not in _REFS:
        t = H.inputs(R, Cs, hid, e_dim, F, out_dim, seed=R * 1000 + Cs)
        t32 = tuple(None if x is None else x.float() for x in t)
        _REFS[key] = (t32, H.factored(*t32, act=act, slope=slope), H.factored(*[None if x is None else x.double() for x in t32], act=act, slope=slope))
    return _REFS[key]


def _on(t32, device, padded_rows, wide_weight=False):
    a, b, f, W0, b0, w1, b1 = [None if x is None else x.to(device) for x in t32]
    if padded_rows:
        a, b = _padded(a), _padded(b)
        assert a.stride(0) > a.size(1) and b.stride(0) > b.size(1)
    if wide_weight:                      # the weight as a view of a wider matrix: read in place through its leading dimension
        W0 = torch.cat([W0, torch.full((W0.size(0), 3), 1e6, device=device)], 1)[:, :W0.size(1)]
        assert W0.stride(0) == W0.size(1) + 3
    return a, b, f, (W0, b0), (w1, b1)


# (R, Cs): one pair; rows and a column chunk with a 3-lane tail; exactly one chunk; more than two blocks of rows on the LANES (130 x 2)
# e_dim: a multiple of 64, not one, the models' 1 024;  F: none, two steps, three;  out_dim: 1, 3, the limit 8;  hid 15: padded views
@pytest.mark.parametrize("R,Cs,hid,e_dim,F,out_dim,act,slope", [
    (1, 1, 60, 64, 0, 1, "none", 0.0), (5, 67, 15, 70, 4, 3, "relu", 0.0), (3, 64, 60, 1024, 6, 8, "leaky", 0.2),
    (130, 2, 15, 70, 6, 1, "leaky", 0.2), (5, 67, 60, 1024, 4, 1, "none", 0.0), (130, 2, 60, 64, 0, 8, "relu", 0.0),
    (3, 64, 15, 70, 4, 3, "none", 0.0), (1, 1, 15, 1024, 6, 3, "leaky", 0.2), (130, 2, 60, 1024, 4, 3, "relu", 0.0)])
def test_pair_head_matches_the_restatement_within_the_fp64_twin_bound(device, R, Cs, hid, e_dim, F, out_dim, act, slope):
    t32, ref32, ref64 = _case(R, Cs, hid, e_dim, F, out_dim, act, slope)
    args = _on(t32, device, padded_rows=hid == 15, wide_weight=e_dim == 70)
    with torch.no_grad():
        out = ops.pair_head(*args, act=act, slope=slope)
        again = ops.pair_head(*args, act=act, slope=slope)
    assert out.shape == (R, Cs, out_dim) and out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out, again), "two runs differ"
    assert_fp32_parity(out, ref64, ref32, f"pair_head {R}x{Cs} hid={hid} e_dim={e_dim} F={F} out_dim={out_dim} {act}")
    if F == 0:                            # an empty f is F = 0 too
        with torch.no_grad():
            assert torch.equal(out, ops.pair_head(args[0], args[1], torch.empty(R, Cs, 0, device=device), *args[3:], act=act, slope=slope))


def test_pair_head_linear_modules_and_the_empty_tables(device):
    """The two ``torch.nn.Linear`` are their weights and biases; ``R == 0`` / ``Cs == 0``: a zero-sized result and no launch."""
    t32, ref32, ref64 = _case(5, 67, 60, 70, 4, 3, "relu", 0.0)
    a, b, f, (W0, b0), (w1, b1) = _on(t32, device, False)
    lin0, lin1 = torch.nn.Linear(124, 70).to(device), torch.nn.Linear(70, 3).to(device)
    with torch.no_grad():
        lin0.weight.copy_(W0), lin0.bias.copy_(b0), lin1.weight.copy_(w1), lin1.bias.copy_(b1)
        out = ops.pair_head(a, b, f, lin0, lin1, "relu")
        assert torch.equal(out, ops.pair_head(a, b, f, (W0, b0), (w1, b1), "relu"))
        assert_fp32_parity(out, ref64, ref32, "pair_head on Linear modules")
        with _lib.kernel_timer() as kt:
            e = ops.pair_head(a[:0], b, f[:0], lin0, lin1, "relu")
            assert e.shape == (0, 67, 3) and e.dtype == torch.float32
            assert ops.pair_head(a, b[:0], f[:, :0], lin0, lin1).shape == (5, 0, 3)
            assert ops.pair_head(a[:0], b[:0], None, (W0[:, :120], b0), lin1).shape == (0, 0, 3)
        assert kt.records() == [], "an empty table launched something"


def test_pair_head_entries_do_not_depend_on_the_selection(device):
    """Bit for bit: the 5 x 67 table's entries are those of the same op on row subsets, on column subsets (the 3-column one puts the ROWS
    on the lanes) and on a single pair."""
    t32, _, _ = _case(5, 67, 15, 70, 4, 3, "leaky", 0.2)
    a, b, f, lin0, lin1 = _on(t32, device, padded_rows=True)
    with torch.no_grad():
        run = lambda ra, cb: ops.pair_head(a[ra], b[cb], f[ra][:, cb], lin0, lin1, "leaky", 0.2)       # noqa: E731
        whole = run(slice(0, 5), slice(0, 67))
        assert torch.equal(whole, run(slice(0, 5), slice(0, 67))), "two runs differ"
        for ra in (slice(0, 2), slice(2, 5)):
            assert torch.equal(run(ra, slice(0, 67)), whole[ra]), f"rows {ra} differ from the whole table's"
        for cb in (slice(0, 64), slice(64, 67)):
            assert torch.equal(run(slice(0, 5), cb), whole[:, cb]), f"columns {cb} differ from the whole table's"
        for i, j in ((3, 65), (0, 0), (4, 66)):
            assert torch.equal(run(slice(i, i + 1), slice(j, j + 1)), whole[i:i + 1, j:j + 1]), f"pair ({i}, {j}) alone differs"


def test_pair_head_launches_and_refusals(device):
    """One call is the side launch (both products) plus ONE ``k_pair_head``; a refusal launches nothing."""
    t32, _, _ = _case(5, 67, 60, 70, 4, 3, "relu", 0.0)
    a, b, f, lin0, lin1 = _on(t32, device, False)
    (W0, b0), (w1, b1) = lin0, lin1
    with torch.no_grad():
        with _lib.kernel_timer() as kt:
            ops.pair_head(a, b, f, lin0, lin1, "relu")
        # 5 x 67, e_dim = 70: the columns on the lanes.  A: 70 x ceil(5 / 4) threads = 1 block; Bt: 67 x ceil(70 / 4) threads = 5 blocks;
        # the head: two lane chunks x one group of 16 rows
        assert [(n, g) for n, g, _ in kt.records()] == [("k_pair_head_side", 1 + 5), ("k_pair_head", 2)]
        with _lib.kernel_timer() as kt:            # 130 x 2: the rows on the lanes — three lane chunks, one group of columns
            t130, _, _ = _case(130, 2, 60, 64, 0, 8, "relu", 0.0)
            ops.pair_head(*_on(t130, device, False), act="relu")
        assert [(n, g) for n, g, _ in kt.records()] == [("k_pair_head_side", 9 + 1), ("k_pair_head", 3)]
    with _lib.kernel_timer() as kt:
        with torch.no_grad():
            for bad in (dict(a=a.cpu()), dict(f=f.cpu()), dict(lin1=(w1.cpu(), b1.cpu()))):
                kw = dict(a=a, b=b, f=f, lin0=lin0, lin1=lin1)
                kw.update(bad)
                with pytest.raises(GlamHipError, match="CPU tensor"):
                    ops.pair_head(kw["a"], kw["b"], kw["f"], kw["lin0"], kw["lin1"])
            with pytest.raises(GlamHipError, match="the two sides disagree"):
                ops.pair_head(a, b[:, :59], f, lin0, lin1)
            with pytest.raises(GlamHipError, match=r"f must be \[5, 67, F\]"):
                ops.pair_head(a, b, f[:, :66], lin0, lin1)
            with pytest.raises(GlamHipError, match="lin0 must map 2 \\* 60 \\+ 0 = 120"):
                ops.pair_head(a, b, None, lin0, lin1)
            with pytest.raises(GlamHipError, match="lin1 must map the 70 outputs"):
                ops.pair_head(a, b, f, lin0, (w1[:, :69], b1))
            with pytest.raises(GlamHipError, match="out_dim = 9 is outside 1..8"):
                ops.pair_head(a, b, f, lin0, (torch.zeros(9, 70, device=device), torch.zeros(9, device=device)))
            with pytest.raises(GlamHipError, match="F = 17 fusion columns are outside 0..16"):
                ops.pair_head(a, b, torch.zeros(5, 67, 17, device=device), (torch.zeros(70, 137, device=device), b0), lin1)
            with pytest.raises(GlamHipError, match="act = 'celu'"):
                ops.pair_head(a, b, f, lin0, lin1, "celu")
            with pytest.raises(GlamHipError, match="expected float32"):
                ops.pair_head(a.double(), b, f, lin0, lin1)
        for grad in (dict(a=a.clone().requires_grad_(True)), dict(lin0=(W0.clone().requires_grad_(True), b0))):
            kw = dict(a=a, lin0=lin0)
            kw.update(grad)
            with pytest.raises(GlamHipError, match=r"inference only.*head=\"rows\".*forward_shared"):
                ops.pair_head(kw["a"], b, f, kw["lin0"], lin1)
    assert [n for n, _, _ in kt.records() if n in _KINDS] == [], "a refusal launched something"
    with _lib.kernel_timer() as kt, torch.enable_grad():                   # grad mode alone is fine: nothing here requires grad
        assert ops.pair_head(a, b, f, lin0, lin1).shape == (5, 67, 3)
    assert [n for n, _, _ in kt.records()] == list(_KINDS)


# ---------------------------------------------------------------------------------------------
# ArchitectureDDI.score_matrix(head="factored")
# ---------------------------------------------------------------------------------------------
def _ddi(**kw):
    """``test_gpu_ddi_pairs._net`` — and, for a keyword it sets itself (``end_act``, ``e_dim``), the same constructor call with that one
    replaced."""
    if not set(kw) & {"end_act", "e_dim"}:
        return _net(**kw)
    torch.manual_seed(12)
    return model.ArchitectureDDI(**{**dict(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()"), **_ACTS, **kw}).eval()


def _spy(monkeypatch, name, into):
    inner = getattr(model, name)

    def f(*a, **k):
        r = inner(*a, **k)
        into.append((r[0] if isinstance(r, tuple) else r).detach().clone())
        return r
    monkeypatch.setattr(model, name, f)


@pytest.mark.parametrize("kw", [dict(), dict(hid_dim_alpha=1), dict(out_dim=3), dict(end_act="LeakyReLU")],
                         ids=["default", "hid15", "out_dim3", "LeakyReLU"])
def test_score_matrix_factored_vs_the_oracle_and_the_rows_head(device, monkeypatch, kw):
    """``head="factored"`` against the oracle's two-drug model on the expanded batches (the call of
    ``test_score_matrix_vs_score_pairs_and_the_oracle``; for ``end_act="LeakyReLU"`` the same oracle with that activation in its head);
    fusions and contacts are those of ``head="rows"`` bit for bit; entries picked from the whole 9 x 9 table are the selection's bits."""
    drugs = _drugs()
    net = _ddi(**kw)
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    R, Cs, out_dim = len(_MROWS), len(_MCOLS), kw.get("out_dim", 1)
    cast = lambda b, dt: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
    first, second = np.repeat(_MROWS, Cs).tolist(), np.tile(_MCOLS, R).tolist()
    e1, e2 = Batch.from_data_list([drugs[q] for q in first]), Batch.from_data_list([drugs[q] for q in second])
    twin = {}

    def run(dt):
        if dt not in twin:
            sd = {k: v.to(dt) if v.is_floating_point() else v for k, v in sd0.items()}
            with torch.no_grad():
                if "end_act" in kw:
                    o = O.architecture_ddi(sd, cast(e1, dt), cast(e2, dt), R * Cs, message_steps=2, mol_block="_NNConv", graph_norm="_None",
                                           **{**_ACTS, "end_act": kw["end_act"]})
                else:
                    o = _oracle_ddi(sd, cast(e1, dt), cast(e2, dt), R * Cs, dt, "_NNConv", "_None", "GlobalPool5", "_None")
            twin[dt] = o.view(R, Cs, out_dim)
        return twin[dt], []
    net = net.to(device)
    net.graphed_call = False
    seen = []
    _spy(monkeypatch, "dot_and_global_pool2_grid", seen)
    with torch.no_grad():
        enc = net.encode_drugs(Batch.from_data_list(drugs).to(device))
        rows_out, rows_con = net.score_matrix(enc, _MROWS, _MCOLS, return_argmax=True, head="rows")
        rows_fusion = list(seen)
        seen.clear()
        with _lib.kernel_timer() as kt:
            out, con = net.score_matrix(enc, _MROWS, _MCOLS, return_argmax=True, head="factored")
        names = [n for n, _, _ in kt.records()]
        assert [n for n in names if n in _KINDS] == list(_KINDS), "the factored head is one side launch and one head launch"
        assert [n for n in names if n.startswith("k_pair_grid")] == ["k_pair_grid", "k_pair_grid_finish"] * 2
        assert out.shape == (R, Cs, out_dim) and len(seen) == 2
        assert all(torch.equal(x, y) for x, y in zip(seen, rows_fusion)), "the fusions differ from head=\"rows\""
        assert all(torch.equal(x, y) for x, y in zip(con, rows_con)), "the contacts differ from head=\"rows\""
        what = f"score_matrix(head=factored) {kw}"
        assert_twin_parity(run, out, [], what)
        assert_twin_parity(run, rows_out, [], what + " [head=rows on the same encoding]")
        assert torch.equal(out, net.score_matrix(enc, _MROWS, _MCOLS, head="factored")), "two runs differ"
        full = net.score_matrix(enc, head="factored")
        assert full.shape == (9, 9, out_dim)
        assert torch.equal(full[_MROWS][:, _MCOLS], out), "entries picked from the whole table are not the selection's bits"
        assert net.score_matrix(enc, [], _MCOLS, head="factored").shape == (0, Cs, out_dim)
        assert net.score_matrix(enc, _MROWS, [], head="factored").shape == (R, 0, out_dim)


def test_score_matrix_factored_refusals_launch_nothing(device):
    drugs = Batch.from_data_list(_drugs()).to(device)
    with torch.no_grad():
        nets = {k: _ddi(**kw).to(device) for k, kw in (("plain", {}), ("norm", dict(end_norm="_LayerNorm")), ("celu", dict(end_act="CELU")))}
        encs = {k: n.encode_drugs(drugs) for k, n in nets.items()}
        for k, n in nets.items():
            assert n.score_matrix(encs[k], [0, 1], [2], head="rows").shape == (2, 1, 1)
        with _lib.kernel_timer() as kt:
            with pytest.raises(GlamHipError, match=r"lin_out0's norm is _LayerNorm.*head=\"rows\""):
                nets["norm"].score_matrix(encs["norm"], head="factored")
            with pytest.raises(GlamHipError, match=r"not CELU.*head=\"rows\""):
                nets["celu"].score_matrix(encs["celu"], head="factored")
            with pytest.raises(GlamHipError, match=r"block_pairs = 5.*head=\"rows\""):
                nets["plain"].score_matrix(encs["plain"], head="factored", block_pairs=5)
            with pytest.raises(GlamHipError, match="head = 'blocks' is not"):
                nets["plain"].score_matrix(encs["plain"], head="blocks")
            for k in ("norm", "celu"):                                         # matrix_top's default head is the factored one
                with pytest.raises(GlamHipError, match=r"score_matrix: head=\"factored\".*head=\"rows\""):
                    nets[k].matrix_top(encs[k])
        assert kt.records() == [], "a refusal launched something"
        assert nets["plain"].score_matrix(encs["plain"], [0, 1], [2], head="factored").shape == (2, 1, 1)


# ---------------------------------------------------------------------------------------------
# ArchitectureDTI.screen_panel(head="factored")
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [4, 1], ids=["hid60", "hid15"])
def test_screen_panel_factored_vs_the_oracle_and_the_rows_head(device, monkeypatch, alpha):
    """Column ``j`` against the oracle's two-tower model on that column's expanded batch (``test_gpu_panel._oracle_dti``, the panel
    test's reference); hid = 15: the ligands' flat rows reach the head as views of padded rows.  Fusions and contacts are those of
    ``head="rows"``; a column picked from the whole panel is the selection's bits; ``screen_top`` passes the keyword through."""
    mols, pros = P._graphs()
    mb = Batch.from_data_list(mols)
    net = P._net(hid_dim_alpha=alpha)
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    cast = lambda b, dt: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
    twin = {}

    def column(q, dt):
        if (q, dt) not in twin:
            sd = {k: v.to(dt) for k, v in sd0.items()}
            with torch.no_grad():
                twin[q, dt] = P._oracle_dti(sd, cast(mb, dt), cast(Batch.from_data_list([pros[q]] * P._L), dt), P._L, "_NNConv", "_GCNConv",
                                            "_None", "_None")
        return twin[q, dt]
    net = net.to(device)
    net.graphed_call = False
    seen = []
    _spy(monkeypatch, "dot_and_global_pool2_panel", seen)
    mol_dev = mb.to(device)
    sel = [2, 0]
    with torch.no_grad():
        enc = net.encode_proteins(Batch.from_data_list(pros).to(device))
        rows_out, rows_con = net.screen_panel(mol_dev, enc, sel, return_argmax=True)
        rows_fusion = list(seen)
        seen.clear()
        with _lib.kernel_timer() as kt:
            out, con = net.screen_panel(mol_dev, enc, sel, return_argmax=True, head="factored")
        assert [n for n, _, _ in kt.records() if n in _KINDS] == list(_KINDS)
        assert out.shape == (P._L, 2, 1) and len(seen) == 2
        assert all(torch.equal(x, y) for x, y in zip(seen, rows_fusion)) and all(torch.equal(x, y) for x, y in zip(con, rows_con))
        ref = lambda dt: (torch.stack([column(q, dt) for q in sel], 1), [])                        # noqa: E731
        assert_twin_parity(ref, out, [], f"screen_panel(head=factored) alpha={alpha}")
        assert_twin_parity(ref, rows_out, [], f"screen_panel(head=rows) alpha={alpha}")
        assert torch.equal(net.screen_panel(mol_dev, enc, head="factored")[:, sel], out), "columns picked from the whole panel differ"
        assert net.screen_panel(mol_dev, enc, [], head="factored").shape == (P._L, 0, 1)
        top = net.screen_top([mol_dev], enc, sel, k=3, head="factored")
        want = hits_restated.top([(out[..., 0].cpu().numpy(), None)], 3, True)
        assert hits_restated.same(top.result(), want), "screen_top(head=factored) is not the top of the factored panel"
        with _lib.kernel_timer() as kt:
            with pytest.raises(GlamHipError, match="head = 'x' is not"):
                net.screen_panel(mol_dev, enc, sel, head="x")
            with pytest.raises(GlamHipError, match="head = 'x' is not"):
                net.screen_top([mol_dev], enc, sel, head="x")
        assert kt.records() == [], "a refusal launched something"


# ---------------------------------------------------------------------------------------------
# memory: the hidden matrix is never allocated
# ---------------------------------------------------------------------------------------------
def test_factored_head_never_allocates_the_hidden_matrix(device):
    """e_dim = 1 024, 64 x 64 pairs: the hidden matrix of the listed head is 4 096 x 1 024 x 4 B = 16 MiB.  A condition, not a
    measurement: the factored call's peak above the starting allocation stays under 4 MiB (``A`` + ``Bt`` 0.5 MiB, ``f`` + ``out`` +
    the fusions under 0.2 MiB, the rest slack for the allocator's rounding); the same probe on ``head="rows"`` sees the 16 MiB."""
    rng = np.random.default_rng(3)
    rows, cols = rng.integers(0, 9, 64).tolist(), rng.integers(0, 9, 64).tolist()
    net = _ddi(e_dim=1024).to(device)
    MiB = 1 << 20
    with torch.no_grad():
        enc = net.encode_drugs(Batch.from_data_list(_drugs()).to(device))
        peaks = {}
        for head in ("factored", "rows", "factored"):                          # (the first call plans, sums and stages; the others are measured)
            torch.cuda.synchronize()
            start = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = net.score_matrix(enc, rows, cols, head=head)
            torch.cuda.synchronize()
            peaks[head] = torch.cuda.max_memory_allocated() - start
            assert out.shape == (64, 64, 1)
            del out
    print(f"peak above the start: factored {peaks['factored'] / MiB:.2f} MiB, rows {peaks['rows'] / MiB:.2f} MiB")
    assert peaks["factored"] < 4 * MiB, f"head=\"factored\" peaked {peaks['factored'] / MiB:.2f} MiB above its start"
    assert peaks["rows"] >= 16 * MiB, f"the probe does not see the hidden matrix of head=\"rows\": {peaks['rows'] / MiB:.2f} MiB"


# ---------------------------------------------------------------------------------------------
# ArchitectureDDI.matrix_top
# ---------------------------------------------------------------------------------------------
def test_matrix_top_is_the_top_of_the_factored_table(device):
    """``k = 3`` row drugs per column drug, blocks of one row drug, of four and the automatic block: the lists are ``hits_restated.top`` of
    the factored table's task column — exactly, because a block's entries are the table's bits — under the drug ids of ``rows``, the
    duplicate included; an empty ``rows`` gives empty lists."""
    net = _ddi(out_dim=3).to(device)
    task = 2
    with torch.no_grad():
        enc = net.encode_drugs(Batch.from_data_list(_drugs()).to(device))
        table = net.score_matrix(enc, _MROWS, _MCOLS, head="factored")
        want = hits_restated.top([(table[..., task].cpu().numpy(), _MROWS)], 3, True)
        assert set(want[1].reshape(-1).tolist()) <= set(_MROWS) and want[2].tolist() == [3] * len(_MCOLS)
        for block_rows in (1, 4, 0):
            top = net.matrix_top(enc, _MROWS, _MCOLS, k=3, task=task, block_rows=block_rows)
            assert top.queries == len(_MCOLS) and top.offered == len(_MROWS)
            assert hits_restated.same(top.result(), want), f"block_rows={block_rows}: not the top of the table"
        low = net.matrix_top(enc, np.asarray(_MROWS), torch.tensor(_MCOLS), k=3, task=task, largest=False, block_rows=4)
        assert hits_restated.same(low.result(), hits_restated.top([(table[..., task].cpu().numpy(), _MROWS)], 3, False))
        whole = net.matrix_top(enc, k=3, task=task)                            # every drug against every drug
        full = net.score_matrix(enc, head="factored")
        assert hits_restated.same(whole.result(), hits_restated.top([(full[..., task].cpu().numpy(), None)], 3, True))
        by_rows = net.matrix_top(enc, _MROWS, _MCOLS, k=3, task=task, head="rows")                   # the listed head: a list, not these bits
        assert by_rows.offered == len(_MROWS) and (by_rows.result()[2] == 3).all()
        with _lib.kernel_timer() as kt:
            empty = net.matrix_top(enc, [], _MCOLS, k=3, task=task)
        s, i, c = empty.result()
        assert empty.queries == len(_MCOLS) and empty.offered == 0 and (i == -1).all() and c.tolist() == [0] * len(_MCOLS) and torch.isnan(s).all()
        assert [n for n, _, _ in kt.records() if n.startswith("k_pair")] == [], "an empty rows scored something"
        assert net.matrix_top(enc, _MROWS, [], k=3).queries == 0
