"""The host side of refillable protein batches (``glam_amd.data.ResidentDTIRefillBatch``), no GPU: the slot and key
arithmetic against the plain-Python restatement of tests/protein_refill_restated.py, its refusals, the filler order on ties, the
capacity check, ``load_many``'s tables, every refusal of ``graphs.dti_refill_admission`` by module name, and the C ABI of csrc/gcn.hip."""
import ctypes
import types

import numpy as np
import pytest
import torch

from glam_amd import _lib, data, graphs, layer, model
from tests import protein_refill_restated as R
from tests.test_host_logic import _header_prototypes, _table_type

_KW = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")


def _world(seed, n_lig=40, n_pro=13, n_pairs=200):
    rng = np.random.default_rng(seed)
    lig_ns = rng.integers(12, 29, n_lig)
    pro_ns = rng.integers(20, 71, n_pro)
    pro_ns[rng.integers(0, n_pro)] = 130
    pro_ns[[2, 5, 9]] = int(pro_ns.min())                      # ties among the smallest: the filler order must break them by id
    first, second = rng.integers(0, n_lig, n_pairs).astype(np.int32), rng.integers(0, n_pro, n_pairs).astype(np.int32)
    return rng, lig_ns, 2 * lig_ns, pro_ns, 6 * pro_ns, first, second


# ---------------------------------------------------------------------------------------------
# slots and keys
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_slots_and_keys_against_the_restatement(seed):
    rng, _ln, _le, pro_ns, _pe, _f, second = _world(seed)
    for Qb in (1, 4, 8, 13):
        for _ in range(20):
            sec = second[rng.integers(0, second.size, 8)]
            if rng.random() < 0.3:
                sec = np.full(8, sec[0])                       # U = 1
            try:
                want = R.slots_and_keys(sec, pro_ns, Qb)
            except ValueError:
                with pytest.raises(ValueError, match=f"distinct proteins, the batch holds protein_slots = {Qb}"):
                    data.protein_slot_ids(sec, pro_ns, Qb)
                continue
            slots, keys, U = data.protein_slot_ids(sec, pro_ns, Qb)
            assert (slots.tolist(), keys.tolist(), U) == want
            assert slots.dtype == np.int64 and keys.dtype == np.int32
            assert len(set(slots.tolist())) == Qb and sorted(slots[:U].tolist()) == slots[:U].tolist()
            assert [int(slots[k]) for k in keys] == sec.tolist()                          # a key names the slot of its pair's protein


def test_more_distinct_proteins_than_slots_is_refused():
    ns = np.array([30, 20, 50, 40])
    with pytest.raises(ValueError, match=r"name 3 distinct proteins, the batch holds protein_slots = 2.*eagerly on proteins\.collate\(u\)"):
        data.protein_slot_ids([0, 3, 3, 2], ns, 2)
    slots, keys, U = data.protein_slot_ids([3, 0, 3, 2], ns, 3)                           # U == Qb: no filler
    assert (slots.tolist(), keys.tolist(), U) == ([0, 2, 3], [2, 0, 2, 1], 3)


def test_fillers_are_the_smallest_by_size_then_id():
    ns = np.array([25, 20, 90, 20, 20, 60])
    slots, keys, U = data.protein_slot_ids([2, 2, 2], ns, 4)
    assert (slots.tolist(), keys.tolist(), U) == ([2, 1, 3, 4], [0, 0, 0], 1)             # three of 20 nodes: by id
    slots, _k, U = data.protein_slot_ids([3, 5], ns, 4)
    assert (slots.tolist(), U) == ([3, 5, 1, 4], 2)                                       # 3 is in u: skipped among the fillers
    slots, _k, _U = data.protein_slot_ids([1, 3, 4], ns, 5)
    assert slots.tolist() == [1, 3, 4, 0, 5]                                              # beyond the ties: the next sizes


# ---------------------------------------------------------------------------------------------
# the table of one load, and the capacity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_table_against_the_restatement(seed):
    rng, lig_ns, lig_es, pro_ns, pro_es, first, second = _world(seed)
    B, Qb, K = 8, 8, 3
    for _ in range(10):
        ids = rng.integers(0, first.size, B)
        table, (N, E), (Np, Ep) = data.dti_refill_tables(ids, first, second, lig_ns, lig_es, pro_ns, pro_es, B, Qb, K)
        assert table.dtype == np.int32 and table.tolist() == R.refill_table(ids, first, second, lig_ns, lig_es, pro_ns, pro_es, Qb, K)
        slots, _keys, _U = R.slots_and_keys(second[ids], pro_ns, Qb)
        assert (N, E) == (int(lig_ns[first[ids]].sum()), int(lig_es[first[ids]].sum()))
        assert (Np, Ep) == (int(pro_ns[slots].sum()), int(pro_es[slots].sum()))
    with pytest.raises(ValueError, match="exactly 8 pairs"):
        data.dti_refill_tables(np.arange(7), first, second, lig_ns, lig_es, pro_ns, pro_es, B, Qb, K)
    with pytest.raises(IndexError):
        data.dti_refill_tables(np.full(8, first.size), first, second, lig_ns, lig_es, pro_ns, pro_es, B, Qb, K)


@pytest.mark.parametrize("seed", range(3))
def test_slots_always_fit_the_computed_capacity_and_a_smaller_one_is_refused(seed):
    """``Qb`` distinct graphs are the case ``padded_capacity`` guarantees: with ``phantom_rows = ns.max()`` every load's slots pass
    ``padded_fit``; a capacity cut below a load's totals is refused with the bucket's message."""
    rng, _ln, _le, pro_ns, pro_es, _f, second = _world(seed, n_pro=30)
    m = int(pro_ns.max())
    for Qb in (1, 4, 9):
        n_cap, e_cap = data.padded_capacity(pro_ns, pro_es, Qb, False, m)
        K = data.phantom_graphs(pro_ns, Qb, n_cap, m)
        for _ in range(40):
            sec = second[rng.integers(0, second.size, 8)][:int(rng.integers(1, 9))]
            try:
                slots, _keys, _U = data.protein_slot_ids(sec, pro_ns, Qb)
            except ValueError:
                continue
            data.padded_fit(Qb, Qb, int(pro_ns[slots].sum()), int(pro_es[slots].sum()), n_cap, e_cap, False, K, m)
    slots, _k, _U = data.protein_slot_ids([int(np.argmax(pro_ns))], pro_ns, 4)
    N, E = int(pro_ns[slots].sum()), int(pro_es[slots].sum())
    with pytest.raises(ValueError, match="exceed the capacity"):
        data.padded_fit(4, 4, N, E, N, E, False, 1, None)                                 # no room for the phantom node
    with pytest.raises(ValueError, match="surplus nodes exceed"):
        data.padded_fit(4, 4, N, E, N + 2 * m + 1, E, False, 2, m)


class _Side:
    """What ``_host_table`` reads of a ``PaddedBatch``: the dataset's counts and the capacity check."""

    def __init__(self, ns, es, K=1):
        self._ds = types.SimpleNamespace(ns=ns, es=es)
        self.num_phantom_graphs, self.fits = K, []

    def _fit(self, B, N, E):
        self.fits.append((B, N, E))


def _host_batch(seed, B=8, Qb=4, K=2):
    rng, lig_ns, lig_es, pro_ns, pro_es, first, second = _world(seed)
    second = np.sort(second)                                   # (runs of one protein: most windows of 8 pairs hold <= 4 distinct ones)
    b = data.ResidentDTIRefillBatch.__new__(data.ResidentDTIRefillBatch)
    b.pairs = types.SimpleNamespace(first_host=first, second_host=second)
    b.mol, b.pro = _Side(lig_ns, lig_es, K), _Side(pro_ns, pro_es)
    b.num_real_graphs, b.protein_slots = B, Qb
    b._cuts = np.cumsum([0, 4 * (B + 1), B, 4 * (Qb + 1), B + K]).tolist()
    return b, rng, (first, second, lig_ns, lig_es, pro_ns, pro_es)


def test_host_table_checks_both_capacities_and_keeps_slots_and_keys():
    b, _rng, (first, second, lig_ns, lig_es, pro_ns, pro_es) = _host_batch(1)
    ids = np.arange(16, 24)
    table = b._host_table(ids)
    assert table.tolist() == R.refill_table(ids, first, second, lig_ns, lig_es, pro_ns, pro_es, 4, 2) and table.size == b._cuts[-1]
    slots, keys, U = R.slots_and_keys(second[ids], pro_ns, 4)
    assert (b.slots.tolist(), b.keys.tolist(), b.distinct) == (slots, keys, U)
    assert b.mol.fits == [(8, int(lig_ns[first[ids]].sum()), int(lig_es[first[ids]].sum()))]
    assert b.pro.fits == [(4, int(pro_ns[slots].sum()), int(pro_es[slots].sum()))]


def test_load_many_stacks_the_tables_of_load(monkeypatch):
    """``load_many`` is ``_ResidentPairBatch``'s: one ``_host_table`` per list, stacked — the tables ``load`` uploads one by one; a list
    with too many distinct proteins refuses the whole epoch before anything is uploaded."""
    assert data.ResidentDTIRefillBatch.load_many is data._ResidentPairBatch.load_many
    assert data.ResidentDTIRefillBatch.load is data._ResidentPairBatch.load
    b, _rng, world = _host_batch(2)
    lists = [np.arange(s, s + 8) for s in (0, 40, 96, 150)]
    want = [b._host_table(ids).copy() for ids in lists]
    seen = []

    class _Pinned:
        def __init__(self, shape):
            self._a = np.zeros(shape, dtype=np.int32)

        def numpy(self):
            return self._a

        def to(self, device, non_blocking=False):
            seen.append(self._a.copy())
            return "tables"

    monkeypatch.setattr(data.torch, "empty", lambda shape, dtype=None, pin_memory=False: _Pinned(shape))
    b._table = types.SimpleNamespace(device="dev", numel=lambda: b._cuts[-1])
    assert b.load_many(lists) == 4 and b._tables == "tables"
    assert len(seen) == 1 and seen[0].tolist() == np.stack(want).tolist()
    unsorted_second = np.arange(200, dtype=np.int32) % 13                                  # 8 consecutive pairs: 8 distinct proteins
    b.pairs.second_host = unsorted_second
    seen.clear()
    with pytest.raises(ValueError, match="distinct proteins"):
        b.load_many(lists)
    assert not seen


# ---------------------------------------------------------------------------------------------
# admission
# ---------------------------------------------------------------------------------------------
def _with_protein_part(net, donor_kw, part):
    """``net`` with the protein-side block ``part`` of a model built with ``donor_kw`` (the ligand side and the head stay admitted)."""
    setattr(net, part, getattr(model.ArchitectureDTI(**dict(_KW, **donor_kw)), part))
    return net


def test_the_default_model_is_admitted():
    net = model.ArchitectureDTI()
    assert type(net.pro_conv.conv) is layer._GCNConv and type(net.mol_conv.conv) is layer._NNConv
    with graphs.dti_refill_admission(net):
        pass
    with graphs.dti_refill_admission(model.ArchitectureDTI(**dict(_KW, pro_block="_NNConv"))):
        pass
    batch = data.ResidentDTIRefillBatch.__new__(data.ResidentDTIRefillBatch)
    assert isinstance(batch.glam_admission(model.SharedStep(net)), graphs.dti_refill_admission)
    assert isinstance(batch.glam_admission(net), graphs.dti_admission)


@pytest.mark.parametrize("donor,part,named", [
    (dict(pro_block="_GATConv"), "pro_conv", r"pro_conv\.conv \(_GATConv\)"),
    (dict(graph_norm="_BatchNorm"), "pro_conv", r"pro_conv\.norm \(_BatchNorm\)"),
    (dict(pre_norm="_BatchNorm"), "pro_lin0", r"pro_lin0\.norm \(_BatchNorm\)"),
    (dict(flat_norm="_BatchNorm"), "pro_flat", r"pro_flat\.norm \(_BatchNorm\)"),
    (dict(graph_norm="_GraphSizeNorm"), "pro_conv", r"pro_conv\.norm \(_GraphSizeNorm\)"),
    (dict(pre_norm="_GraphSizeNorm"), "pro_lin0", r"pro_lin0\.norm \(_GraphSizeNorm\)"),
    (dict(flat_norm="_LayerNorm"), "pro_flat", r"pro_flat\.norm \(_LayerNorm\) is called without a batch vector"),
    (dict(flat_norm="_PairNorm"), "pro_flat", r"pro_flat\.norm \(_PairNorm\) is called without a batch vector"),
])
def test_protein_side_refusals_name_the_module(donor, part, named):
    net = _with_protein_part(model.ArchitectureDTI(**_KW), donor, part)
    with graphs.dti_admission(net):                            # (the fixed-protein batch admits it: its protein tower is exempt)
        pass
    with pytest.raises(ValueError, match="refilled protein batches: " + named):
        graphs.dti_refill_admission(net)
    batch = data.ResidentDTIRefillBatch.__new__(data.ResidentDTIRefillBatch)
    with pytest.raises(ValueError, match=named):
        batch.glam_admission(model.SharedStep(net))


def test_ligand_side_and_head_rules_are_dti_admissions():
    for extra, named in ((dict(end_norm="_BatchNorm"), r"lin_out0\.norm"), (dict(mol_block="_GCNConv"), r"mol_conv\.conv"),
                         (dict(flat_norm="_LayerNorm"), r"mol_flat\.norm")):
        with pytest.raises(ValueError, match=named):
            graphs.dti_refill_admission(model.ArchitectureDTI(**dict(_KW, **extra)))


def test_per_graph_norms_of_the_protein_tower_are_watched_at_their_call():
    net = model.ArchitectureDTI(**dict(_KW, graph_norm="_PairNorm", pre_norm="_LayerNorm"))
    with graphs.dti_refill_admission(net) as adm:
        assert sorted(n for n, _ in adm._norms) == ["mol_conv.norm", "mol_lin0.norm", "pro_conv.norm", "pro_lin0.norm"]
        assert len(net.pro_conv.norm._forward_pre_hooks) == 1
        with pytest.raises(ValueError, match=r"pro_conv\.norm \(_PairNorm\) is called without its batch vector"):
            net.pro_conv.norm(torch.zeros(3, 60))
    assert not net.pro_conv.norm._forward_pre_hooks
    # the two older checks are what they were
    with pytest.raises(ValueError, match=r"pro_conv\.conv"):
        graphs.padded_admission(model.ArchitectureDTI(**_KW))
    assert graphs.dti_admission.PARTS == ("mol_lin0", "mol_conv", "mol_readout", "mol_flat", "lin_out0", "lin_out1")


# ---------------------------------------------------------------------------------------------
# the C ABI, dti_batch's keywords
# ---------------------------------------------------------------------------------------------
def test_abi_version_and_the_new_symbols():
    protos = _header_prototypes()
    p, i64, i32 = "pointer", ctypes.c_int64, ctypes.c_int
    want = {"glam_gcn_scale": (i32, [p, p, i64, p, p]),
            "glam_gcn_fwd": (i32, [p, i64, p, p, p, i64, i32, p, p]),
            "glam_gcn_bwd": (i32, [p, p, p, p, i64, i32, p, p])}
    for name, proto in want.items():
        res, args = _lib.SIGNATURES[name]
        assert (_table_type(res), [_table_type(a) for a in args]) == protos[name] == proto, name
        assert hasattr(_lib.load(), name), f"{name} is not exported"
        assert name not in _lib.VALUE_RETURNS and getattr(_lib.api(), name).errcheck is not None
    assert _lib.ABI_VERSION == 4 and _lib.load().glam_abi_version() == 4
    # every older signature is what it was: glam_pair_list_load serves the keys and the label gather unchanged
    assert protos["glam_pair_list_load"] == (i32, [p, p, p, p, i32, i64, i64, i64, i64, i32, i32] + [p] * 8)


def test_gcn_entry_points_refuse_bad_arguments_on_the_host():
    lib, one = _lib.load(), ctypes.c_void_p(16)
    assert lib.glam_gcn_fwd(one, 129, one, one, one, 4, 129, one, None) == _lib.GLAM_E_UNSUPPORTED
    assert lib.glam_gcn_fwd(one, 3, one, one, one, 4, 4, one, None) == _lib.GLAM_E_INVALID        # ld < D
    assert lib.glam_gcn_bwd(None, one, one, one, 4, 4, one, None) == _lib.GLAM_E_INVALID
    assert lib.glam_gcn_scale(None, None, -1, None, None) == _lib.GLAM_E_INVALID
    assert lib.glam_gcn_scale(None, None, 0, None, None) == 0 and lib.glam_gcn_fwd(None, 4, None, None, None, 0, 4, None, None) == 0


def test_dti_batch_keywords_go_with_a_device_dataset():
    pairs = data.ResidentPairs.__new__(data.ResidentPairs)
    for kw in (dict(protein_slots=4), dict(protein_phantom_rows=70), dict(protein_capacity=(100, 100))):
        with pytest.raises(ValueError, match="go with a DeviceDataset of proteins"):
            pairs.dti_batch(None, data.Batch(), 8, **kw)
    ds = data.DeviceDataset.__new__(data.DeviceDataset)
    with pytest.raises(ValueError, match="needs protein_slots"):
        pairs.dti_batch(None, ds, 8)
