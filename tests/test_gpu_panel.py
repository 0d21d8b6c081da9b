"""GPU (MI355X): panel screening — the protein-stationary fusion (``glam_pair_pool_panel_fwd``: csrc/pairpanel.hip) and
``ArchitectureDTI.screen_panel`` on top of it.

The property everything rests on: column ``j`` of the panel is ``ops.pair_pool_indexed`` with ``pro_of_pair = [sel[j]] * L`` — the max
column and the argmax bit for bit (one ascending fmaf chain per score, ties to the smallest flattened index: a total order, so the grid
cannot show), the whole ``[max, mean]`` within the fp64-twin bound of the oracle on physically replicated rows.  ``screen_panel`` is then
checked column by column against ``screen`` and against the oracle's two-tower model on the expanded batch."""
import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, layer, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_molecule, synth_protein
from tests.conftest import assert_twin_parity

pytestmark = pytest.mark.gpu

_MS = [1, 7, 40, 33, 12, 0, 2]             # an odd count (the two-rows-a-round tail), an empty ligand, more than 32 rows
_PS = [1, 70, 1030, 9, 0, 64, 65]          # one chunk exactly, one row over, 17 chunks, an empty protein
_SLABS = [0, 1, 3, 100]                    # a slab boundary inside the ligand list, a slab larger than it


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


def _ptr(sizes):
    return [0] + list(np.cumsum(sizes))


_CASES = {}


def _case(D, device):
    """Inputs of width ``D`` and their references, computed ONCE and shared (never written): ``ops.pair_pool_indexed`` of every ligand
    against each of the 7 proteins, and the oracle in fp32 / fp64 on physically replicated rows of every non-empty (ligand, protein)."""
    if D not in _CASES:
        torch.manual_seed(D)
        L, Q = len(_MS), len(_PS)
        mb, pb = _batch(_MS), _batch(_PS)
        mol, pro = torch.randn(mb.numel(), D), torch.randn(pb.numel(), D)
        msp, psp = ops.SegmentPtr(mb.to(device), L), ops.SegmentPtr(pb.to(device), Q)
        m, p = mol.to(device), pro.to(device)
        with torch.no_grad():
            cols = [ops.pair_pool_indexed(m, p, msp, psp, [q] * L, return_argmax=True) for q in range(Q)]
        ref = torch.stack([c[0] for c in cols], 1), torch.stack([c[1] for c in cols], 1)          # [L, Q, 2] each
        mo, po = _ptr(_MS), _ptr(_PS)
        live = [(l, q) for l in range(L) for q in range(Q) if _MS[l] and _PS[q]]
        mol_rep = torch.cat([mol[mo[l]:mo[l + 1]] for l, _ in live])
        pro_rep = torch.cat([pro[po[q]:po[q + 1]] for _, q in live])
        mb_rep, pb_rep = _batch([_MS[l] for l, _ in live]), _batch([_PS[q] for _, q in live])
        twin = {}
        for dt in (torch.float32, torch.float64):
            o = O.dot_and_global_pool(mol_rep.to(dt), pro_rep.to(dt), mb_rep, pb_rep, len(live), 2)
            full = torch.zeros(L, Q, 2, dtype=dt)                        # (an empty ligand or protein: 0, 0)
            for (l, q), row in zip(live, o):
                full[l, q] = row
            twin[dt] = full
        _CASES[D] = dict(m=m, p=p, msp=msp, psp=psp, ref=ref, twin=twin)
    return _CASES[D]


@pytest.mark.parametrize("sel", [None, [2, 0, 5, 2, 4]], ids=["all", "picked"])
@pytest.mark.parametrize("D", [60, 64, 16, 15, 92, 128])
def test_panel_fusion_equals_the_indexed_call_column_by_column(device, D, sel):
    """16-byte loads (60, 64, 16, 92, 128) and dword loads (15); every slab gives the bits of the automatic one; two runs agree."""
    c = _case(D, device)
    plan = ops.panel_plan(_PS, sel)
    cols = list(range(len(_PS))) if sel is None else sel
    ref_out, ref_arg = c["ref"][0][:, cols], c["ref"][1][:, cols]
    with torch.no_grad():
        out, arg = ops.pair_pool_panel(c["m"], c["p"], c["msp"], c["psp"], plan, return_argmax=True)
        out2, arg2 = ops.pair_pool_panel(c["m"], c["p"], c["msp"], c["psp"], plan, return_argmax=True)
        plain = ops.pair_pool_panel(c["m"], c["p"], c["msp"], c["psp"], plan)                      # (argmax = NULL in the kernel)
    assert out.shape == (len(_MS), len(cols), 2) and arg.shape == out.shape and arg.dtype == torch.int32
    assert torch.equal(out, out2) and torch.equal(arg, arg2) and torch.equal(out, plain), "two runs differ"
    assert torch.equal(out[..., 0], ref_out[..., 0]), "max column differs from pair_pool_indexed"
    assert torch.equal(arg, ref_arg), "argmax differs from pair_pool_indexed"
    assert_twin_parity(lambda dt: (c["twin"][dt][:, cols], []), out, [], f"pair_pool_panel D={D}")
    molsum, prosum = ops.segment_pool(c["m"], c["msp"], "sum"), ops.segment_pool(c["p"], c["psp"], "sum")
    with torch.no_grad():
        for slab in _SLABS:
            o, a = ops.pair_pool_panel(c["m"], c["p"], c["msp"], c["psp"], plan, molsum, prosum, return_argmax=True, slab=slab)
            assert torch.equal(o, out) and torch.equal(a, arg), f"slab={slab} changes the bits"
    if sel is not None:                      # the duplicated protein: two columns, the same bits
        assert torch.equal(out[:, 0], out[:, 3]) and torch.equal(arg[:, 0], arg[:, 3])


def test_panel_fusion_through_the_layer_and_on_misaligned_rows(device):
    """``layer.dot_and_global_pool2_panel`` is the op; rows that start off a 16-byte boundary (D % 4 == 0) take the dword kernel: same bits."""
    c = _case(60, device)
    plan = ops.panel_plan(_PS, [1, 2])
    mb = _batch(_MS).to(device)
    shifted = torch.empty(c["m"].numel() + 1, device=device)[1:].view_as(c["m"]).copy_(c["m"])
    assert shifted.data_ptr() % 16 == 4
    with torch.no_grad():
        out, arg = ops.pair_pool_panel(c["m"], c["p"], c["msp"], c["psp"], plan, return_argmax=True)
        via_layer = layer.dot_and_global_pool2_panel(c["m"], c["p"], mb, c["psp"], plan)
        o2, a2 = ops.pair_pool_panel(shifted, c["p"], c["msp"], c["psp"], plan, return_argmax=True)
    assert torch.equal(out, via_layer)
    assert torch.equal(o2[..., 0], out[..., 0]) and torch.equal(a2, arg)
    assert torch.equal(out[..., 0], c["ref"][0][:, [1, 2], 0])


@pytest.mark.parametrize("D", [8, 12, 45])
def test_panel_fusion_ties_route_to_the_first_flattened_pair(device, D):
    """Small-integer rows (every dot product exact).  Ligand row 1 has no zero and residue rows 3 and 66 of the 70-row protein repeat it:
    the maximum ``D`` occurs on BOTH sides of the 64-row chunk boundary (and again through the repeated ligand row 3), and ``arg`` is its
    first flattened occurrence ``a * n_res + b`` — through a swapping selection, 16-byte (8, 12) and dword (45) loads."""
    ms, ps, sel = [4, 3], [6, 70], [1, 0]
    mb, pb = _batch(ms), _batch(ps)
    g = torch.Generator().manual_seed(D)
    mol = torch.randint(-1, 2, (mb.numel(), D), generator=g).float()
    pro = torch.randint(-1, 2, (pb.numel(), D), generator=g).float()
    mol[1] = torch.where(mol[1] == 0, torch.ones(()), mol[1])
    mol[3], mol[6] = mol[1], mol[4]
    pro[6 + 3] = pro[6 + 66] = mol[1]
    for a, b in [(1, 0), (3, 2), (4, 0)]:
        pro[a] = pro[b]
    msp, psp = ops.SegmentPtr(mb.to(device), 2), ops.SegmentPtr(pb.to(device), 2)
    plan = ops.panel_plan(ps, sel)
    m_off, p_off = _ptr(ms), _ptr(ps)
    with torch.no_grad():
        for slab in (0, 1):
            out, arg = ops.pair_pool_panel(mol.to(device), pro.to(device), msp, psp, plan, return_argmax=True, slab=slab)
            for l in range(2):
                for j, q in enumerate(sel):
                    S = mol[mb == l].double() @ pro[pb == q].double().T
                    flat = S.reshape(-1)
                    first = int(torch.nonzero(flat == flat.max())[0])              # the FIRST occurrence of the maximum
                    assert (l, j) != (0, 0) or (flat == flat.max()).sum() >= 4, "the case must hold the tie"
                    assert out[l, j, 0].item() == flat[first].item()
                    assert arg[l, j].tolist() == [m_off[l] + first // ps[q], p_off[q] + first % ps[q]]
                    assert abs(out[l, j, 1].item() - S.mean().item()) <= 1e-6
            assert out[0, 0, 0].item() == D and arg[0, 0].tolist() == [1, 6 + 3], "rows 3 and 66 tie: the one before the chunk boundary wins"
            ref, ref_arg = ops.pair_pool_indexed(mol.to(device), pro.to(device), msp, psp, [1, 1], return_argmax=True)
            assert torch.equal(out[:, 0, 0], ref[:, 0]) and torch.equal(arg[:, 0], ref_arg)


def test_panel_fusion_empty_segments_and_empty_panels(device):
    """An empty ligand or an empty (selected) protein: ``0, 0`` and ``arg = -1``, as ``pair_pool``; a selection of empty proteins alone
    has no chunk and still writes; ``L == 0`` / ``Qs == 0`` return empty tensors without a launch."""
    torch.manual_seed(0)
    ms, ps = [3, 0, 5], [0, 6]
    mb, pb = _batch(ms), _batch(ps)
    mol, pro = torch.randn(mb.numel(), 60, device=device), torch.randn(pb.numel(), 60, device=device)
    msp, psp = ops.SegmentPtr(mb.to(device), 3), ops.SegmentPtr(pb.to(device), 2)
    with torch.no_grad():
        out, arg = ops.pair_pool_panel(mol, pro, msp, psp, ops.panel_plan(ps, None), return_argmax=True)
        assert out[1].abs().max().item() == 0.0 and out[:, 0].abs().max().item() == 0.0 and (arg[1] == -1).all() and (arg[:, 0] == -1).all()
        assert abs(out[0, 1, 0].item() - (mol[:3] @ pro.T).max().item()) <= 1e-4 and abs(out[2, 1, 1].item() - (mol[3:] @ pro.T).mean().item()) <= 1e-5
        assert 0 <= arg[0, 1, 0].item() < 3 and 3 <= arg[2, 1, 0].item() < 8 and 0 <= arg[2, 1, 1].item() < 6
        none, none_arg = ops.pair_pool_panel(mol, pro, msp, psp, ops.panel_plan(ps, [0, 0]), return_argmax=True)
        assert none.shape == (3, 2, 2) and none.abs().max().item() == 0.0 and (none_arg == -1).all()
        with _lib.kernel_timer() as kt:
            e, ea = ops.pair_pool_panel(mol, pro, msp, psp, ops.panel_plan(ps, []), return_argmax=True)
            assert e.shape == (3, 0, 2) and ea.shape == (3, 0, 2) and ea.dtype == torch.int32
            no_lig = ops.SegmentPtr.from_parts(torch.zeros(1, dtype=torch.int32, device=device), 0, 0)
            z = ops.pair_pool_panel(torch.empty(0, 60, device=device), pro, no_lig, psp, ops.panel_plan(ps, None))
            assert z.shape == (0, 2, 2)
        assert kt.records() == [], "an empty panel launched something"


def test_panel_fusion_refusals_come_before_any_launch(device):
    ms, ps = [3, 4, 2], [5, 6]
    mb, pb = _batch(ms), _batch(ps)
    mol, pro = torch.randn(mb.numel(), 60, device=device), torch.randn(pb.numel(), 60, device=device)
    msp, psp = ops.SegmentPtr(mb.to(device), 3), ops.SegmentPtr(pb.to(device), 2)
    plan = ops.panel_plan(ps, [1, 0, 1])
    with _lib.kernel_timer() as kt, torch.no_grad():
        for bad in ([0, 2], [-1], [0.5]):
            with pytest.raises(IndexError):
                ops.panel_plan(ps, bad)
        with pytest.raises(GlamHipError, match="read-back"):
            ops.panel_plan(ps, torch.tensor([0, 1], device=device))
        with pytest.raises(GlamHipError, match="ops.panel_plan"):
            ops.pair_pool_panel(mol, pro, msp, psp, [1, 0, 1])
        with torch.enable_grad(), pytest.raises(GlamHipError, match=r"ops\.pair_pool .*ops\.pair_pool_shared"):
            ops.pair_pool_panel(mol.clone().requires_grad_(True), pro, msp, psp, plan)
        with torch.enable_grad(), pytest.raises(GlamHipError, match=r"ops\.pair_pool .*ops\.pair_pool_shared"):
            ops.pair_pool_panel(mol, pro.clone().requires_grad_(True), msp, psp, plan)
        with pytest.raises(GlamHipError, match="the plan was made for"):
            ops.pair_pool_panel(mol, pro, msp, psp, ops.panel_plan([5, 6, 7], None))
        with pytest.raises(GlamHipError, match="the plan was made for"):
            ops.pair_pool_panel(mol, pro, msp, psp, ops.panel_plan([5, 7], None))
        with pytest.raises(GlamHipError, match="disagree"):
            ops.pair_pool_panel(mol[:, :56], pro, msp, psp, plan)
        with pytest.raises(GlamHipError, match="disagree"):
            ops.pair_pool_panel(mol[:-1], pro, msp, psp, plan)
        with pytest.raises(GlamHipError, match="disagree"):
            ops.pair_pool_panel(mol, pro[:-1], msp, psp, plan)
        with pytest.raises(GlamHipError, match="molsum must be"):
            ops.pair_pool_panel(mol, pro, msp, psp, plan, molsum=torch.zeros(3, 59, device=device))
        with pytest.raises(GlamHipError, match="prosum must be"):
            ops.pair_pool_panel(mol, pro, msp, psp, plan, prosum=torch.zeros(3, 60, device=device))
        with pytest.raises(GlamHipError, match="slab"):
            ops.pair_pool_panel(mol, pro, msp, psp, plan, slab=-1)
        wide_m, wide_p = torch.zeros(mb.numel(), 132, device=device), torch.zeros(pb.numel(), 132, device=device)
        with pytest.raises(GlamHipError, match="width 132 is outside the kernel table"):
            ops.pair_pool_panel(wide_m, wide_p, msp, psp, plan)
    assert kt.records() == [], "a refusal launched something"
    with torch.enable_grad():                                  # grad mode alone is fine: nothing here requires grad
        assert ops.pair_pool_panel(mol, pro, msp, psp, plan).shape == (3, 3, 2)


# ---------------------------------------------------------------------------------------------
# ArchitectureDTI.screen_panel
# ---------------------------------------------------------------------------------------------
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU")
_L = 5


def _graphs():
    rng = np.random.default_rng(7)
    return [synth_molecule(rng) for _ in range(_L)], [synth_protein(rng, 40, 130) for _ in range(3)]


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDTI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **_ACTS, **kw).eval()


def _head_block(sd, prefix, x, act, end_norm):
    """``LinearBlock`` of the head: its norm (no ``batch``: statistics over the whole [P, .] matrix) in front of the linear layer."""
    if end_norm == "_LayerNorm":
        x = O.graph_layer_norm(x, sd[prefix + "norm.norm.weight"], sd[prefix + "norm.norm.bias"])
    return O.linear_block(sd, prefix, x, act)


def _oracle_dti(sd, mol, pro, P, mol_block, pro_block, graph_norm, end_norm):
    """``O.architecture_dti`` where it can express the configuration; for a normed head the same assembly, line for line, out of the
    oracle's own pieces."""
    if end_norm == "_None":
        return O.architecture_dti(sd, mol, pro, P, message_steps=2, mol_block=mol_block, pro_block=pro_block, graph_norm=graph_norm, **_ACTS)
    xm, xp = O.linear_block(sd, "mol_lin0.", mol.x, "ReLU"), O.linear_block(sd, "pro_lin0.", pro.x, "ReLU")
    hm = hp = None
    fusion = []
    for _ in range(2):
        xm, hm = O.message_block(sd, "mol_conv.", xm, mol.edge_index, mol.edge_attr, hm, mol.batch, P, conv=mol_block, norm=graph_norm, act="ReLU")
        xp, hp = O.message_block(sd, "pro_conv.", xp, pro.edge_index, pro.edge_attr, hp, pro.batch, P, conv=pro_block, norm=graph_norm, act="ReLU")
        fusion.append(O.dot_and_global_pool(xm, xp, mol.batch, pro.batch, P, stats=2))
    outm = O.linear_block(sd, "mol_flat.", O.global_pool5(xm, mol.batch, P), "ReLU")
    outp = O.linear_block(sd, "pro_flat.", O.global_pool5(xp, pro.batch, P), "ReLU")
    out = torch.cat([outm, outp, torch.cat(fusion, dim=-1)], dim=-1)
    return _head_block(sd, "lin_out1.", _head_block(sd, "lin_out0.", out, "ReLU", end_norm), "_None", end_norm)


@pytest.mark.parametrize("mol_block,pro_block,norm,alpha,end_norm", [
    ("_NNConv", "_GCNConv", "_None", 4, "_None"), ("_TripletMessage", "_TripletMessage", "_PairNorm", 4, "_None"),
    ("_NNConv", "_GATConv", "_LayerNorm", 4, "_None"), ("_NNConv", "_GCNConv", "_None", 1, "_None"),
    ("_NNConv", "_GCNConv", "_None", 4, "_LayerNorm")])
def test_screen_panel_vs_screen_and_the_oracle(device, monkeypatch, mol_block, pro_block, norm, alpha, end_norm):
    """Column ``j`` of ``screen_panel`` against ``screen(ligands, enc, [sel[j]] * L)`` — every step's fusion max bit-equal, the contacts
    equal — and against the oracle's two-tower model on that column's expanded batch (every ligand with a copy of protein ``sel[j]``; a
    per-row head gives the same rows on the ``L * Qs`` batch, the batch-less ``_LayerNorm`` head is DEFINED per column: it is what
    ``screen`` computes).  The configurations of ``test_screen_vs_oracle_on_the_expanded_batch`` (hid = 15 among them: rows that flow
    padded, dword loads) plus a ``_LayerNorm`` head (the per-column route); selections ``[2, 0]`` and all three."""
    mols, pros = _graphs()
    mb = Batch.from_data_list(mols)
    net = _net(mol_block=mol_block, pro_block=pro_block, graph_norm=norm, hid_dim_alpha=alpha, end_norm=end_norm)
    assert net._panel_head_in_one_pass() is (end_norm == "_None")
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    cast = lambda b, dt: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
    twin = {}                                                  # protein -> dtype -> the oracle's [L, 1] column, computed once

    def column(q, dt):
        if (q, dt) not in twin:
            sd = {k: v.to(dt) for k, v in sd0.items()}
            with torch.no_grad():
                twin[q, dt] = _oracle_dti(sd, cast(mb, dt), cast(Batch.from_data_list([pros[q]] * _L), dt), _L, mol_block, pro_block, norm, end_norm)
        return twin[q, dt]
    net = net.to(device)
    net.graphed_call = False
    seen = {"panel": [], "screen": []}

    def spy(name, key):
        inner = getattr(model, name)

        def f(*a, **k):
            r = inner(*a, **k)
            seen[key].append(r[0].detach().clone())
            return r
        monkeypatch.setattr(model, name, f)
    spy("dot_and_global_pool2_indexed", "screen")
    spy("dot_and_global_pool2_panel", "panel")
    mol_dev = mb.to(device)
    lig = ops.segment_ptr(mol_dev.batch).ptr.cpu()
    with torch.no_grad():
        enc = net.encode_proteins(Batch.from_data_list(pros).to(device))
        assert enc.sizes_host is None and enc.prosum is None and enc.plans == {}
        res = enc.sp.ptr.cpu()
        per_protein = {}
        for q in range(3):
            seen["screen"].clear()
            o, c = net.screen(mol_dev, enc, [q] * _L, return_argmax=True)
            per_protein[q] = (o, c, list(seen["screen"]))
        for sel in ([2, 0], None):
            cols = [0, 1, 2] if sel is None else sel
            seen["panel"].clear()
            out, contacts = net.screen_panel(mol_dev, enc, sel, return_argmax=True)
            assert out.shape == (_L, len(cols), 1) and len(contacts) == 2 and len(seen["panel"]) == 2
            assert all(c.shape == (_L, len(cols), 2) and c.dtype == torch.int32 for c in contacts)
            assert torch.equal(out, net.screen_panel(mol_dev, enc, sel))
            for j, q in enumerate(cols):
                o, c, fus = per_protein[q]
                for s in range(2):
                    assert torch.equal(seen["panel"][s][:, j, 0], fus[s][:, 0]), f"step {s}, column {j}: the fusion max differs from screen"
                    assert torch.equal(contacts[s][:, j], c[s]), f"step {s}, column {j}: the contacts differ from screen"
                    cc = contacts[s][:, j].cpu()
                    assert ((lig[:-1] <= cc[:, 0]) & (cc[:, 0] < lig[1:])).all() and ((res[q] <= cc[:, 1]) & (cc[:, 1] < res[q + 1])).all()
                assert_twin_parity(lambda dt: (column(q, dt), []), o, [], f"screen, protein {q}")
            what = f"screen_panel {mol_block}/{pro_block}/{norm}/alpha={alpha}/end={end_norm}/sel={sel}"
            assert_twin_parity(lambda dt: (torch.stack([column(q, dt) for q in cols], 1), []), out, [], what)
    assert enc.sizes_host.tolist() == [p.x.size(0) for p in pros] and len(enc.prosum) == 2 and set(enc.plans) == {(2, 0), None}


def test_screen_panel_reuses_the_encodings_sums_and_plan_and_refuses_a_stale_one(device):
    mols, pros = _graphs()
    mol_dev, pro_dev = Batch.from_data_list(mols).to(device), Batch.from_data_list(pros).to(device)
    net = _net().to(device)
    with torch.no_grad():
        enc = net.encode_proteins(pro_dev)
        first = net.screen_panel(mol_dev, enc, [2, 0])
        sizes, sums, plan = enc.sizes_host, enc.prosum, enc.plans[(2, 0)]
        staged = plan.on(device)
        for s, r in zip(sums, enc.rows):
            assert torch.equal(s, ops.segment_pool(r, enc.sp, "sum"))
        again = net.screen_panel(mol_dev, enc, np.asarray([2, 0]))             # the same selection in another container
        assert torch.equal(first, again)
        assert enc.sizes_host is sizes and enc.prosum is sums and all(a is b for a, b in zip(enc.prosum, sums))
        assert list(enc.plans) == [(2, 0)] and enc.plans[(2, 0)] is plan and all(a is b for a, b in zip(plan.on(device), staged))
        net.screen_panel(mol_dev, enc)                                         # another selection: another plan, the same sums
        assert list(enc.plans) == [(2, 0), None] and enc.prosum is sums and enc.sizes_host is sizes
        assert net.screen_panel(mol_dev, enc, []).shape == (_L, 0, 1)
        with _lib.kernel_timer() as kt:
            with pytest.raises(IndexError, match=r"proteins must lie in \[0, 3\)"):
                net.screen_panel(mol_dev, enc, [0, 3])
            with pytest.raises(GlamHipError, match="another model"):
                _net().to(device).screen_panel(mol_dev, enc)
            next(net.pro_conv.parameters()).add_(1)
            with pytest.raises(GlamHipError, match="screen_panel: the encoding is stale"):
                net.screen_panel(mol_dev, enc, [2, 0])
        assert kt.records() == [], "a refusal launched something"
        assert net.screen_panel(mol_dev, net.encode_proteins(pro_dev), [2, 0]).shape == (_L, 2, 1)     # a fresh encoding is accepted again
    with pytest.raises(GlamHipError, match="no_grad"):
        net.screen_panel(mol_dev, enc)
