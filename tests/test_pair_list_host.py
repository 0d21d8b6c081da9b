"""CPU: the host side of refillable pair lists (``ops.PairList``, ``data.ResidentPairs``, ``model.SharedStep``; csrc/pairlist.hip) — the C
prototypes against their ctypes rows, the entry point's argument checks by status code, the numpy restatement of the kernel against
``ops.PairsByProtein`` (with six wrong restatements that must fail), the table builders of the DTI / DDI batches against theirs, every
refusal that runs before anything is enqueued, and the admission check a ``GraphedTrainStep`` asks a pair batch for."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from glam_amd import _lib, data, graphs, model, ops, ops_pair
from glam_amd._lib import GlamHipError
from tests.pair_list_restated import (WRONG, cases, ddi_table_restated, dti_table_restated, labels_restated, pair_list_restated,
                                      reference_lists)
from tests.test_host_logic import _header_prototypes, _table_type

_ALL = ("glam_pair_list_supported", "glam_pair_list_load")
_KW = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")
_CASES = cases()


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_pair_list_prototypes_match_their_signature_rows_and_are_exported():
    protos = _header_prototypes()
    for name in _ALL:
        res, args = _lib.SIGNATURES[name]
        assert (_table_type(res), [_table_type(a) for a in args]) == protos[name], name
        assert hasattr(_lib.load(), name), f"{name} is not exported"
        assert name not in _lib.VALUE_RETURNS                                    # both return a STATUS
        assert getattr(_lib.api(), name).errcheck is not None and getattr(_lib.load(), name).errcheck is None
    p, i64, i32 = "pointer", ctypes.c_int64, ctypes.c_int
    assert protos["glam_pair_list_supported"] == (i32, [i64, i64])
    assert protos["glam_pair_list_load"] == (i32, [p, p, p, p, i32, i64, i64, i64, i64, i32, i32] + [p] * 8)
    assert _lib.ABI_VERSION == 4


def test_pair_list_supported_is_the_documented_bound():
    f = _lib.load().glam_pair_list_supported
    assert [f(P, Q) for P, Q in ((1, 1), (1056, 8), (1024, 1024), (4096, 1700), (65536, 1024), (1024, 65536), (8192, 8192))] == [0] * 7
    bad = ((65537, 1), (1, 65537), (65536, 1025), (8193, 8192), (1 << 40, 1 << 40))
    assert [f(P, Q) for P, Q in bad] == [_lib.GLAM_E_UNSUPPORTED] * len(bad)
    with pytest.raises(GlamHipError, match=r"P \* Q <= 67108864"):
        _lib.api().glam_pair_list_supported(65536, 1025)


def test_pair_list_entry_point_rejects_bad_arguments_without_a_gpu():
    f = _lib.load().glam_pair_list_load
    fake = ctypes.c_void_p(4096)                                                # (never dereferenced: each call fails a check first)

    def call(ids=fake, ca=fake, cb=fake, y=fake, rb=12, B=5, P=8, Qa=3, Qb=4, pa=0, pb=3, ia=fake, oa=fake, pta=fake, ib=fake, ob=fake,
             ptb=fake, yo=fake):
        return f(ids, ca, cb, y, rb, B, P, Qa, Qb, pa, pb, ia, oa, pta, ib, ob, ptb, yo, None)
    for bad in (dict(P=0), dict(B=-1), dict(B=9), dict(Qa=-1), dict(Qa=0), dict(pa=3), dict(pb=-1), dict(pb=4), dict(ia=None), dict(oa=None),
                dict(pta=None), dict(ib=None), dict(ob=None), dict(ptb=None), dict(yo=None), dict(y=None), dict(rb=0), dict(rb=6),
                dict(y=ctypes.c_void_p(4098)), dict(ca=None, cb=None, y=None, yo=None)):
        assert call(**bad) == _lib.GLAM_E_INVALID, bad
    for bad in (dict(P=65537, B=1), dict(Qa=65537), dict(P=65536, Qb=1025)):
        assert call(**bad) == _lib.GLAM_E_UNSUPPORTED, bad
        assert call(**bad, ia=None, oa=None, ib=None, yo=None) == _lib.GLAM_E_UNSUPPORTED       # ... before the pointers are looked at
    with pytest.raises(GlamHipError, match="glam_pair_list_load"):
        _lib.api().glam_pair_list_load(*[None] * 4, 0, 1, 0, 0, 0, 0, 0, *[None] * 8)


# ---------------------------------------------------------------------------------------------
# the kernel restated, against PairsByProtein and numpy
# ---------------------------------------------------------------------------------------------
def _checks(case, got, ids, previous=None):
    """Whether ``got = (idx, order, ptr, y_out)`` is what the issue defines for this load: the lists ``PairsByProtein`` builds, numpy's
    stable argsort / cumulative bincount, the padded index and the gathered labels."""
    idx, order, ptr, y_out = got
    want_idx = np.full(case["P"], case["pad"], dtype=np.int32)
    want_idx[:case["B"]] = case["col"][ids]
    by = ops.PairsByProtein(want_idx, case["Q"])
    ref_order, ref_ptr = reference_lists(want_idx, case["Q"])
    assert np.array_equal(by.order, ref_order) and np.array_equal(by.ptr, ref_ptr)
    return (np.array_equal(idx, want_idx) and idx.dtype == np.int32 and np.array_equal(order, by.order) and order.dtype == np.int32
            and np.array_equal(ptr, by.ptr) and ptr.dtype == np.int32 and np.array_equal(y_out, case["y"][ids]))


def _restated(case, ids, wrong=None, previous=None):
    idx, order, ptr = pair_list_restated(ids, case["col"], case["B"], case["P"], case["Q"], case["pad"], wrong, previous)
    return idx, order, ptr, labels_restated(ids, case["y"], case["B"], wrong)


@pytest.mark.parametrize("case", _CASES, ids=[c["name"] for c in _CASES])
def test_restated_kernel_equals_pairs_by_protein(case):
    assert len(case["loads"]) >= 2 and not np.array_equal(case["loads"][0], case["loads"][1])
    previous = None
    for ids in case["loads"]:
        got = _restated(case, ids, previous=previous)
        assert _checks(case, got, ids)
        assert got[2][-1] == case["P"] and got[2][0] == 0
        previous = got[0]
    # the identity form (ids = NULL): the column itself is the step's index
    B = min(case["B"], case["col"].shape[0])
    ident = dict(case, B=B)
    assert _checks(ident, _restated(ident, None), np.arange(B))


@pytest.mark.parametrize("wrong", WRONG)
def test_wrong_restatements_fail_on_these_cases(wrong):
    """Each mistake the kernel's shape invites is seen by the comparison on at least one case of the list — and on the case made for it."""
    caught = {}
    for case in _CASES:
        previous = np.roll(np.arange(case["P"]) % case["Q"], 1).astype(np.int32)          # what a load before left in idx
        ok = True
        for ids in case["loads"]:
            got = _restated(case, ids, wrong, previous)
            ok = ok and _checks(case, got, ids)
            previous = got[0]
        caught[case["name"]] = not ok
    assert any(caught.values()), f"the wrong restatement '{wrong}' passes every case"
    made_for = {"unstable": "one segment owns every pair, five rounds", "stale_phantom": "padding slots, Q beyond a block of waves, most segments empty",
                "open_ptr": "one pair", "pad_ignored": "padding behind a short load, pad = Q - 1",
                "ghost_run": "padding slots, Q beyond a block of waves, most segments empty", "y_by_slot": "a second key round"}
    assert caught[made_for[wrong]], (wrong, caught)


# ---------------------------------------------------------------------------------------------
# the table builders of the DTI / DDI batches
# ---------------------------------------------------------------------------------------------
def _dti_world():
    g = np.random.default_rng(5)
    ns, es = g.integers(12, 29, 40), g.integers(20, 60, 40)
    first, second = g.integers(0, 40, 120).astype(np.int32), g.integers(0, 3, 120).astype(np.int32)
    return g, ns, es, first, second


def test_table_builders_equal_their_restatements():
    g, ns, es, first, _second = _dti_world()
    for ids in (g.permutation(120)[:8], g.integers(0, 120, 8), torch.from_numpy(g.permutation(120)[:8]), list(range(8)),
                g.permutation(120)[:8].astype(np.uint16)):
        table, N, E = data.dti_tables(ids, first, ns, es, 8)
        want, wN, wE = dti_table_restated(np.asarray(ids), first, ns, es)
        assert table.dtype == np.int32 and np.array_equal(table, want) and (N, E) == (wN, wE)
        assert np.array_equal(table[:4 * 9].reshape(4, 9), data.resident_table(first[np.asarray(ids)], ns, es, np.zeros(40, dtype=np.int64))[0])
        got = data.ddi_table(ids, 120, 8)
        assert got.dtype == np.int32 and np.array_equal(got, ddi_table_restated(np.asarray(ids)))


def test_loads_are_refused_on_the_host_before_any_device_work():
    _g, ns, es, first, _second = _dti_world()
    for builder in (lambda ids: data.dti_tables(ids, first, ns, es, 8), lambda ids: data.ddi_table(ids, 120, 8),
                    lambda ids: data.pair_ids_table(ids, 120, 8)):
        for n in (7, 9, 0):
            with pytest.raises(ValueError, match="holds exactly 8 pairs"):
                builder(list(range(n)))
        for bad in ([0, 1, 2, 3, 4, 5, 6, 120], [-1, 1, 2, 3, 4, 5, 6, 7]):
            with pytest.raises(IndexError, match=r"pair ids must lie in \[0, 120\)"):
                builder(bad)
        with pytest.raises(IndexError, match="pair ids must hold integers"):
            builder(np.arange(8, dtype=np.float32))
        with pytest.raises(IndexError, match="pair ids must hold integers"):
            builder(torch.zeros(8, dtype=torch.bool))
        with pytest.raises(IndexError, match="pair ids must be a vector"):
            builder(np.zeros((2, 4), dtype=np.int64))
        with pytest.raises(GlamHipError, match="pair ids lives on a device.*read-back"):
            builder(torch.zeros(8, dtype=torch.int64, device="meta"))


def test_pair_list_bounds_are_refused_before_any_copy():
    assert ops.pair_list_bounds(1056, 8) == (1056, 8, 0) and ops.pair_list_bounds(4096, 1700, 5) == (4096, 1700, 5)
    for P, Q in ((65536, 1025), (65537, 1), (2, 65537)):
        with pytest.raises(GlamHipError, match=r"P \* Q <= 2\^26.*ops\.pair_index"):
            ops.pair_list_bounds(P, Q)
        with pytest.raises(GlamHipError, match=r"P \* Q <= 2\^26"):           # ... before the device is looked at
            ops.PairList(P, Q, "cpu")
    for P, Q, pad in ((0, 3, 0), (4, 0, 0), (4, 3, 3), (4, 3, -1)):
        with pytest.raises(ValueError, match="padding segment"):
            ops.PairList(P, Q, "cpu", pad=pad)
    with pytest.raises(GlamHipError, match="PairList lives on an MI355X HIP device"):
        ops.PairList(8, 3, "cpu")
    assert ops.PairList is ops_pair.PairList and issubclass(ops.PairList, ops.PairIndex)


def _host_list(P, Q, pad=0, name="pro_of_pair"):
    """A ``PairList`` without its device tensors: what the host-side callers look at."""
    lst = ops.PairList.__new__(ops.PairList)
    lst.P, lst.Q, lst.pad, lst.host, lst.name, lst.over = P, Q, pad, None, name, "proteins"
    return lst


def test_pair_list_index_is_checked_on_the_host():
    lst = _host_list(6, 4, pad=2)
    assert lst.check([3, 0, 1]).tolist() == [3, 0, 1, 2, 2, 2] and lst.check([]).tolist() == [2] * 6
    assert lst.check(torch.tensor([1, 1, 1, 1, 1, 1])).dtype == np.int32
    with pytest.raises(IndexError, match=r"pro_of_pair must lie in \[0, 4\)"):
        lst.check([0, 4])
    with pytest.raises(IndexError, match="at most the 6 pairs"):
        lst.check([0] * 7)
    with pytest.raises(IndexError, match="must hold integers"):
        lst.check([0.5])
    with pytest.raises(GlamHipError, match="lives on a device"):
        lst.check(torch.zeros(3, dtype=torch.int64, device="meta"))
    # pair_index takes it under its P / Q check, as it takes a PairIndex
    assert ops.pair_index(lst, 6, 4) is lst
    with pytest.raises(IndexError, match="validated for 6 pairs over 4 proteins, not 6 over 5"):
        ops.pair_index(lst, 6, 5)
    assert ops.pair_count(lst) == 6


def test_host_table_callers_refuse_a_pair_list():
    lst = _host_list(3, 3, name="idx1")
    with pytest.raises(GlamHipError, match="map_plan builds its tables on the host.*pass the host integers that were loaded"):
        ops.map_plan([4, 5, 6], [1, 2, 3], lst, None)
    with pytest.raises(GlamHipError, match="map_plan builds its tables on the host"):
        ops.map_plan([4, 5, 6], [1, 2, 3], [0, 1, 2], lst)
    assert ops.map_plan([4, 5, 6], [1, 2, 3], ops.pair_index([0, 1, 2], 3, 3), None).P == 3          # a host PairIndex passes, as before

    class _Sp:
        B, N, ptr = 3, 10, None
    net = model.ArchitectureDDI(**_KW).eval()
    enc = model.DrugEncoding(net, [None, None], [None, None], _Sp(), None, None, net._drug_stamp())
    with torch.no_grad(), pytest.raises(GlamHipError, match="matrix_top builds its tables on the host.*rows as the host integers"):
        net.matrix_top(enc, rows=lst, k=2)


# ---------------------------------------------------------------------------------------------
# ResidentPairs: validated once, on the host
# ---------------------------------------------------------------------------------------------
def test_resident_pairs_validates_before_it_asks_for_a_device():
    y = np.zeros((4, 1), dtype=np.float32)
    with pytest.raises(IndexError, match="first must hold integers"):
        data.ResidentPairs([0.0, 1.0, 2.0, 3.0], [0, 0, 0, 0], y, "cpu")
    with pytest.raises(IndexError, match=r"second must lie in \[0, 2147483647\): got -1"):
        data.ResidentPairs([0, 1, 2, 3], [0, -1, 0, 0], y, "cpu")
    with pytest.raises(ValueError, match="the two columns disagree"):
        data.ResidentPairs([0, 1, 2, 3], [0, 0, 0], y, "cpu")
    with pytest.raises(ValueError, match="4 pairs but 3 label rows"):
        data.ResidentPairs([0, 1, 2, 3], [0, 0, 0, 0], y[:3], "cpu")
    with pytest.raises(ValueError, match="no positive multiple of 4 bytes"):
        data.ResidentPairs([0, 1, 2, 3], [0, 0, 0, 0], np.zeros((4, 1), dtype=np.float16), "cpu")
    with pytest.raises(GlamHipError, match="first lives on a device"):
        data.ResidentPairs(torch.zeros(4, dtype=torch.int64, device="meta"), [0, 0, 0, 0], y, "cpu")
    with pytest.raises(GlamHipError, match="ResidentPairs lives on an MI355X HIP device"):
        data.ResidentPairs([0, 1, 2, 3], [0, 0, 0, 0], y, "cpu")
    # a padded batch of graphs without labels exists only where it is asked for
    with pytest.raises(ValueError, match="same number"):
        data.padded_bucket(np.full(4, 10), np.full(4, 20), np.zeros(0), 2, None, True)
    assert data.padded_bucket(np.full(4, 10), np.full(4, 20), np.zeros(0), 2, None, True, labels=False) == (21, 40, 0)


# ---------------------------------------------------------------------------------------------
# the stepper's glue
# ---------------------------------------------------------------------------------------------
def test_shared_step_registers_the_model_under_one_prefix():
    net = model.ArchitectureDTI(**_KW)
    step = model.SharedStep(net)
    assert step.model is net and list(step.children()) == [net]
    assert sorted(step.state_dict()) == sorted("model." + k for k in net.state_dict())
    assert [p is q for p, q in zip(step.parameters(), net.parameters())] == [True] * len(list(net.parameters()))
    with pytest.raises(GlamHipError, match="SharedStep wraps a model with forward_shared"):
        model.SharedStep(model.Architecture())
    calls = []

    class _Dti:
        mol, pro, index = "m", "p", "i"

    class _Ddi:
        mol1, mol2, first, second = "a", "b", "f", "s"
    net.forward_shared = lambda *a: calls.append(a)
    step(_Dti())
    ddi = model.ArchitectureDDI(**_KW)
    ddi.forward_shared = lambda *a: calls.append(a)
    model.SharedStep(ddi)(_Ddi())
    assert calls == [("m", "p", "i"), ("a", "b", "f", "s")]


def test_dti_admission_checks_the_ligand_tower_and_the_head_and_exempts_the_protein_tower():
    kw = dict(_KW, mol_block="_TripletMessage")
    adm = graphs.dti_admission(model.ArchitectureDTI(**kw))                      # the default pro_block="_GCNConv": admitted
    with adm:
        pass
    assert type(model.ArchitectureDTI(**kw).pro_conv.conv).__name__ == "_GCNConv"
    for extra, named in ((dict(end_norm="_BatchNorm"), "lin_out0.norm"), (dict(flat_norm="_LayerNorm"), "mol_flat.norm"),
                         (dict(end_norm="_PairNorm"), "lin_out0.norm"), (dict(mol_block="_GCNConv"), "mol_conv.conv"),
                         (dict(graph_norm="_GraphSizeNorm"), "mol_conv.norm")):
        with pytest.raises(ValueError, match=named.replace(".", r"\.")):
            graphs.dti_admission(model.ArchitectureDTI(**dict(kw, **extra)))
    # a per-graph norm of the ligand tower is admitted and watched; the protein tower's is not looked at
    net = model.ArchitectureDTI(**dict(kw, graph_norm="_PairNorm"))
    with graphs.dti_admission(net) as adm:
        assert [n for n, _ in adm._norms] == ["mol_conv.norm"]
        assert len(net.mol_conv.norm._forward_pre_hooks) == 1 and not net.pro_conv.norm._forward_pre_hooks
    assert not net.mol_conv.norm._forward_pre_hooks
    # padded_admission itself is unchanged for the whole tree
    with pytest.raises(ValueError, match=r"pro_conv\.conv"):
        graphs.padded_admission(model.ArchitectureDTI(**kw))


def test_batches_hand_the_stepper_their_own_admission():
    dti = model.ArchitectureDTI(**dict(_KW, mol_block="_TripletMessage", end_norm="_BatchNorm"))
    batch = data.ResidentDTIBatch.__new__(data.ResidentDTIBatch)
    for m in (dti, model.SharedStep(dti)):
        with pytest.raises(ValueError, match=r"lin_out0\.norm"):
            batch.glam_admission(m)
    ddi = model.ArchitectureDDI(**dict(_KW, end_norm="_BatchNorm"))
    guard = data.ResidentDDIBatch.__new__(data.ResidentDDIBatch).glam_admission(model.SharedStep(ddi))
    assert isinstance(guard, contextlib.nullcontext)
    assert not hasattr(data.PaddedBatch, "glam_admission")                       # its path through the stepper is the old one


def test_stepper_asks_the_batch_for_its_admission_before_anything_runs():
    seen = []

    class _Batch:
        def glam_reload(self):
            seen.append("reload")

        def glam_admission(self, m):
            seen.append(("admission", m))
            raise ValueError("refused by the batch")

    class _Opt:
        param_groups = [dict(capturable=True, lr=0.0, params=[torch.zeros(1)])]

        def zero_grad(self, set_to_none=True):
            seen.append("zero_grad")
    net = torch.nn.Linear(2, 2)
    stepper = graphs.GraphedTrainStep(net, _Opt(), lambda out, b: out.sum())
    with pytest.raises(ValueError, match="refused by the batch"):
        stepper._step(_Batch())
    assert seen == [("admission", net)] and not stepper._admitted and stepper.graphs() == 0
