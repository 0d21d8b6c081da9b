"""CPU: the host side of DTI training on a label table (csrc/pairpanel_bwd.hip, ``ops.pair_pool_panel_shared``,
``ArchitectureDTI.forward_panel``) — the backward restated in numpy in the kernel's order against the autograd twin on the expanded pair
list (and six wrong variants of it that the twin bound must catch), the selection grouped by protein, the C prototype against its ctypes
row, the entry point's argument checks by status code, and the refusals that come before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, layer, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_batch, synth_protein
from tests import panel_train_restated as R
from tests.conftest import assert_twin_parity
from tests.test_host_logic import _header_prototypes, _table_type

BWD = "glam_pair_pool_panel_bwd"
_KW = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")

# ligand 1 and protein 1 are empty (protein 1 is selected), protein 2 is named twice, protein 3 never
_MS, _PS, _SEL, _D = [3, 0, 5, 17], [6, 0, 20, 4], [2, 0, 2, 1], 12


def _case(seed=0):
    torch.manual_seed(seed)
    mol, pro = torch.randn(sum(_MS), _D), torch.randn(sum(_PS), _D)
    d_out = torch.randn(len(_MS), len(_SEL), 2)
    out, arg = R.panel_fwd(mol.numpy(), pro.numpy(), _MS, _PS, _SEL)
    return mol, pro, d_out, torch.from_numpy(out).float(), arg


def _restated(mol, pro, d_out, arg, dtype=np.float32, **kw):
    return [torch.from_numpy(np.ascontiguousarray(t)) for t in R.panel_bwd(mol.numpy(), pro.numpy(), _MS, _PS, _SEL, arg, d_out.numpy(),
                                                                           dtype=dtype, **kw)]


def test_restated_backward_sits_within_the_twin_bound():
    """fp32 in the kernel's order against the oracle's fusion on the expanded pair list under autograd (fp32 and fp64), and fp64 against
    fp64 almost to the bit; with a second use of both matrices added last."""
    mol, pro, d_out, out, arg = _case()
    run = R.twin_on_expanded(O.dot_and_global_pool, mol, pro, _MS, _PS, _SEL, d_out, skip_empty=True)
    assert_twin_parity(run, out, _restated(mol, pro, d_out, arg), "restated", names=["mol", "pro"])
    g64 = _restated(mol, pro, d_out, arg, dtype=np.float64)
    for got, ref in zip(g64, run(torch.float64)[1]):
        assert (got - ref).abs().max().item() < 1e-12
    assert g64[1][sum(_PS[:3]):].abs().max().item() == 0.0, "a protein the selection does not name gets exact zeros"
    assert arg[1].max() == -1 and arg[:, 3].max() == -1 and arg[0, :3].min() >= 0, "the empty ligand and the empty protein carry the flag"
    am, ap = torch.randn_like(mol), torch.randn_like(pro)
    extra = lambda m, p: (m * am.to(m)).sum() + (p * ap.to(p)).sum()      # noqa: E731
    assert_twin_parity(R.twin_on_expanded(O.dot_and_global_pool, mol, pro, _MS, _PS, _SEL, d_out, extra, skip_empty=True), out,
                       _restated(mol, pro, d_out, arg, add_mol=am.numpy(), add_pro=ap.numpy()), "restated + add", names=["mol", "pro"])


@pytest.mark.parametrize("wrong", R.WRONG)
def test_the_twin_bound_catches_a_wrong_backward(wrong):
    mol, pro, d_out, out, arg = _case()
    run = R.twin_on_expanded(O.dot_and_global_pool, mol, pro, _MS, _PS, _SEL, d_out, skip_empty=True)
    with pytest.raises(AssertionError, match="fp64-twin noise floor"):
        assert_twin_parity(run, out, _restated(mol, pro, d_out, arg, wrong=wrong), wrong, names=["mol", "pro"])


def test_by_protein_is_a_stable_sort_of_the_selection():
    for sizes, sel in (([4, 0, 9, 2], [2, 0, 2, 1]), ([3, 3, 3], None), ([5, 6], []), ([1, 2, 3, 4, 5], [4, 4, 0, 4, 2, 0, 2, 2])):
        plan = ops.panel_plan(sizes, sel)
        lists = plan.by_protein()
        assert lists is plan.by_protein() and isinstance(lists, ops._Staged)
        order, ptr = R.by_protein(plan.sel, len(sizes))
        assert lists.order.dtype == np.int32 and lists.ptr.dtype == np.int32
        assert np.array_equal(lists.order, order) and np.array_equal(lists.ptr, ptr)
        assert np.array_equal(lists.order, np.argsort(plan.sel, kind="stable"))
        for q in range(len(sizes)):
            assert np.array_equal(lists.order[lists.ptr[q]:lists.ptr[q + 1]], np.flatnonzero(plan.sel == q))
        assert len(plan._parts) == 2 and plan._parts[0] is plan.sel and plan._parts[1] is plan.work      # plan.on() stays (sel, work)
    plan = ops.panel_plan([4, 0, 9, 2], [2, 0, 2, 1])
    lig, col = plan.row_index(3)
    assert (lig, col) == plan.row_index(3) and lig.host.tolist() == [0] * 4 + [1] * 4 + [2] * 4 and col.host.tolist() == [2, 0, 2, 1] * 3
    assert (lig.P, lig.Q, col.P, col.Q) == (12, 3, 12, 4)


def test_prototype_matches_the_signature_table():
    """Header and ``SIGNATURES`` type for type; a STATUS return that ``api()`` checks; the ABI version stays 4 (additive) and the forward
    keeps its signature."""
    protos = _header_prototypes()
    p, i64, i32 = "pointer", ctypes.c_int64, ctypes.c_int
    res, args = _lib.SIGNATURES[BWD]
    assert (_table_type(res), [_table_type(a) for a in args]) == protos[BWD]
    assert protos[BWD] == (i32, [p] * 11 + [i64, i64, i64, i32, p, p, p, p, p])
    assert BWD not in _lib.VALUE_RETURNS
    assert getattr(_lib.api(), BWD).errcheck is not None and getattr(_lib.load(), BWD).errcheck is None
    assert protos["glam_pair_pool_panel_fwd"] == (i32, [p] * 5 + [i64, p, i64, i64, i64, i32, p, p, i32, p, p, p, ctypes.c_size_t, p])
    assert _lib.load().glam_abi_version() == _lib.ABI_VERSION == 4


def test_entry_point_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    one = ctypes.c_void_p(4096)          # a non-null, aligned address nothing dereferences: the checks come first
    bwd = lambda Qs, L, Q, D, p=one: lib.glam_pair_pool_panel_bwd(*([p] * 11), Qs, L, Q, D, None, None, p, p, None)      # noqa: E731
    assert bwd(0, 0, 0, 60) == 0 and bwd(0, 5, 3, 128, None) == 0 and bwd(4, 0, 3, 1, None) == 0      # an empty table: before any pointer
    for D in (0, 129, 132, -4, 256):
        assert bwd(4, 2, 2, D) == _lib.GLAM_E_UNSUPPORTED, D
        assert bwd(4, 2, 2, D, None) == _lib.GLAM_E_UNSUPPORTED, D            # ... before the pointers are looked at
    assert bwd(4, 2, 2, 129) == _lib.GLAM_E_UNSUPPORTED and b"129" in lib.glam_last_error() and BWD.encode() in lib.glam_last_error()
    assert bwd(4, 2, 2, 60, None) == _lib.GLAM_E_INVALID and b"null" in lib.glam_last_error()
    assert bwd(4, 2, 0, 60) == _lib.GLAM_E_INVALID and b"no protein segment" in lib.glam_last_error()
    assert bwd(-1, 2, 2, 60) == _lib.GLAM_E_INVALID and bwd(4, -1, 2, 60) == _lib.GLAM_E_INVALID and bwd(4, 2, -1, 60) == _lib.GLAM_E_INVALID
    assert bwd(1 << 16, 1 << 16, 2, 60) == _lib.GLAM_E_INVALID and b"L * Qs" in lib.glam_last_error()
    assert bwd(4, 2, 2, 60, ctypes.c_void_p(4098)) == _lib.GLAM_E_INVALID and b"aligned" in lib.glam_last_error()
    for hole in list(range(11)) + [17, 18]:          # every operand, list and output; add_mol / add_pro (15, 16) may be NULL
        a = [one] * 11 + [4, 2, 2, 60, None, None, one, one, None]
        a[hole] = None
        assert lib.glam_pair_pool_panel_bwd(*a) == _lib.GLAM_E_INVALID and b"null" in lib.glam_last_error(), hole
    with pytest.raises(GlamHipError, match=f"{BWD} failed"):
        _lib.api().glam_pair_pool_panel_bwd(*[None] * 11, 4, 4, 4, 60, *[None] * 5)


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDTI(**_KW, **kw).eval()


def _proteins(n, seed=4):
    rng = np.random.default_rng(seed)
    return Batch.from_data_list([synth_protein(rng, 40, 130) for _ in range(n)])


def test_forward_panel_refuses_on_the_host():
    mb, pros = synth_batch(4, seed=3), _proteins(2)
    for slot, norm, where in (("graph_norm", "_GraphSizeNorm", "mol_conv"), ("pre_norm", "_GraphSizeNorm", "mol_lin0"),
                              ("flat_norm", "_LayerNorm", "mol_flat"), ("flat_norm", "_PairNorm", "mol_flat")):
        with pytest.raises(GlamHipError, match=f"forward_panel: {where}'s norm {norm}.*depends on how often each graph"):
            _net(**{slot: norm}).forward_panel(mb, pros)
    for tower in ("mol", "pro"):                                                       # either tower alone
        odd = _net()
        getattr(odd, tower + "_conv").norm = getattr(_net(graph_norm="_GraphSizeNorm"), tower + "_conv").norm
        with pytest.raises(GlamHipError, match=f"forward_panel: {tower}_conv's norm _GraphSizeNorm"):
            odd.forward_panel(mb, pros)
        odd = _net()
        getattr(odd, tower + "_flat").norm = getattr(_net(flat_norm="_LayerNorm"), tower + "_flat").norm
        with pytest.raises(GlamHipError, match=f"forward_panel: {tower}_flat's norm _LayerNorm"):
            odd.forward_panel(mb, pros)
        odd = _net().train()
        getattr(odd, tower + "_lin0").norm = getattr(_net(pre_norm="_BatchNorm"), tower + "_lin0").norm
        with pytest.raises(GlamHipError, match=f"forward_panel: {tower}_lin0's norm _BatchNorm .* how often it is repeated"):
            odd.forward_panel(mb, pros)
    net = _net()
    sizes = (pros.ptr[1:] - pros.ptr[:-1]).numpy()
    with pytest.raises(GlamHipError, match="forward_panel: the plan was made for 3 proteins"):
        net.forward_panel(mb, pros, plan=ops.panel_plan(list(sizes) + [5]))
    with pytest.raises(GlamHipError, match="forward_panel: the plan was made for 2 proteins of"):
        net.forward_panel(mb, pros, plan=ops.panel_plan(sizes + 1))
    with pytest.raises(GlamHipError, match="plan must come from ops.panel_plan"):
        net.forward_panel(mb, pros, plan=[0, 1])
    with pytest.raises(GlamHipError, match="not both"):
        net.forward_panel(mb, pros, [0, 1], plan=ops.panel_plan(sizes))
    # what passes the guards goes on to the device — and a CPU batch fails there, loudly (no CPU fallback); the head's norms are free
    for ok in (_net(pre_norm="_BatchNorm"), _net(graph_norm="_PairNorm").train(), _net(end_norm="_LayerNorm").train(), _net()):
        with pytest.raises(GlamHipError, match="HIP device only"):
            ok.forward_panel(mb, pros, plan=ops.panel_plan(sizes, [1, 0, 1]))
    # forward_shared keeps its own words
    with pytest.raises(GlamHipError, match="forward_shared: pro_conv's norm _GraphSizeNorm.*how often each protein"):
        _net(graph_norm="_GraphSizeNorm").forward_shared(mb, pros, [0, 1, 1, 0])


def test_op_refuses_on_the_host_and_pair_pool_panel_still_refuses_grad():
    class _SP:
        def __init__(self, B, N):
            self.B, self.N = B, N
    mol, pro = torch.randn(4, 8, requires_grad=True), torch.randn(6, 8)
    plan = ops.panel_plan([2, 4], [1, 0, 1])
    with pytest.raises(GlamHipError, match="pair_pool_panel is inference only"):
        ops.pair_pool_panel(mol, pro, _SP(2, 4), _SP(2, 6), plan)
    with pytest.raises(GlamHipError, match="plan must come from ops.panel_plan"):
        ops.pair_pool_panel_shared(mol, pro, _SP(2, 4), _SP(2, 6), [1, 0, 1])
    with pytest.raises(GlamHipError, match="the plan was made for 2 proteins of 6 residue rows, the operands hold 3 of 6"):
        ops.pair_pool_panel_shared(mol, pro, _SP(2, 4), _SP(3, 6), plan)
    with pytest.raises(GlamHipError, match="width 132 is outside the kernel table"):
        ops.pair_pool_panel_shared(torch.randn(4, 132), torch.randn(6, 132), _SP(2, 4), _SP(2, 6), plan)
    with pytest.raises(GlamHipError, match="HIP device only"):
        ops.pair_pool_panel_shared(mol, pro, _SP(2, 4), _SP(2, 6), plan)
    assert "pair_pool_panel_shared" in ops.__dict__ and hasattr(layer, "dot_and_global_pool2_panel_shared")
