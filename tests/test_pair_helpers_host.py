"""CPU: the helpers the pair-fusion family shares (``glam_amd/ops_pair.py``, ``glam_amd/model.py``) — the host-vector validator at each of
its three call sites, the one staged-copy holder, "P of whichever index is given", the model guards built from slots against the
methods that call them, and what the table calls share: the plan cache, the listed head over a table, the fusion columns and the one
launch site of the panel forward."""
import numpy as np
import pytest
import torch

from glam_amd import model, ops, ops_pair
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_batch, synth_protein

_Q = 4      # proteins / upper bound of an entry
_SIZES_WRONG = "panel_plan: the proteins' sizes must be a vector of non-negative integers"
_SIZES_ON_DEVICE = "panel_plan: the proteins' sizes live on a device: the plan is built on the host — pass their host copy"


def _sizes_of(plan):
    """The sizes a plan over every protein was made from: the rows of its chunks, summed per protein."""
    out = np.zeros(plan.Q, dtype=np.int64)
    np.add.at(out, plan.sel[plan.chunks[:, 0]], plan.chunks[:, 2])
    return out


# site -> (the validator with that caller's words, the public function's view of the same array)
_SITES = {
    "pair_index": (lambda v: ops.host_ints(v, "pro_of_pair", "have one entry per pair", n=3, below=_Q),
                   lambda v: ops.pair_index(v, 3, _Q).host),
    "panel selection": (lambda v: ops.host_ints(v, "proteins", "be a vector of protein numbers", below=_Q),
                        lambda v: ops.panel_plan([5, 6, 7, 8], v).sel),
    "panel sizes": (lambda v: ops.host_ints(v, "sizes", None, wrong=_SIZES_WRONG, on_device=_SIZES_ON_DEVICE),
                    lambda v: _sizes_of(ops.panel_plan(v))),
}


_OK, _INTS, _RANGE, _DEVICE = "ok", "must hold integers", r"must lie in \[0, 4\)", "read-back"
# input -> what each site makes of it: "ok", or (exception class, the fragment the existing tests match)
_I, _G = IndexError, GlamHipError
_TABLE = [
    # name,            input,                                             pair_index,                    selection,                     sizes
    ("list",           [2, 0, 3],                                         _OK,                           _OK,                           _OK),
    ("int32",          np.array([2, 0, 3], dtype=np.int32),               _OK,                           _OK,                           _OK),
    ("int64",          np.array([2, 0, 3], dtype=np.int64),               _OK,                           _OK,                           _OK),
    ("uint8",          np.array([2, 0, 3], dtype=np.uint8),               _OK,                           _OK,                           _OK),
    ("float",          np.array([2.0, 0.0, 3.0]),                         (_I, _INTS),                   (_I, _INTS),                   (_I, "non-negative integers")),
    ("bool",           np.array([True, False, True]),                     (_I, _INTS),                   (_I, _INTS),                   (_I, "non-negative integers")),
    ("2-D",            np.zeros((3, 2), dtype=np.int64),                  (_I, "one entry per pair"),    (_I, "vector of protein numbers"), (_I, "non-negative integers")),
    ("empty",          [],                                                (_I, "one entry per pair"),    _OK,                           _OK),
    ("CPU tensor",     torch.tensor([2, 0, 3]),                           _OK,                           _OK,                           _OK),
    ("wrong length",   [2, 0],                                            (_I, "one entry per pair"),    _OK,                           _OK),
    ("entry -1",       [2, -1, 3],                                        (_I, _RANGE),                  (_I, _RANGE),                  (_I, "non-negative integers")),
    ("entry Q",        [2, _Q, 3],                                        (_I, _RANGE),                  (_I, _RANGE),                  _OK),
    ("device tensor",  torch.zeros(3, dtype=torch.int64, device="meta"),  (_G, _DEVICE),                 (_G, _DEVICE),                 (_G, "live on a device")),
]


@pytest.mark.parametrize("site", list(_SITES))
def test_host_vector_validator_at_each_call_site(site):
    helper, public = _SITES[site]
    col = 2 + list(_SITES).index(site)
    for row in _TABLE:
        name, v, want = row[0], row[1], row[col]
        if want == _OK:
            got = helper(v)
            assert isinstance(got, np.ndarray) and got.ndim == 1 and got.dtype.kind in "iu", (site, name)
            ref = v.numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.int64 if len(v) == 0 else None)
            assert np.array_equal(got, ref), (site, name)
            assert np.array_equal(public(v), ref), (site, name)
        else:
            for f in (helper, public):
                with pytest.raises(want[0], match=want[1]) as e:
                    f(v)
                assert type(e.value) is want[0], (site, name)


def test_validator_messages_are_the_callers():
    with pytest.raises(IndexError, match=r"idx2 must have one entry per pair: shape \(2,\) for 3 pairs"):
        ops.pair_index([0, 1], 3, 4, name="idx2", over="segments of x2")
    with pytest.raises(IndexError, match=r"proteins must be a vector of protein numbers: shape \(1, 2\)$"):
        ops.panel_plan([5, 6], [[0, 1]])
    with pytest.raises(IndexError, match=r"first must lie in \[0, 4\): got -2 \.\. 3"):
        ops.pair_index([3, -2, 0], 3, 4, name="first", over="drugs")
    with pytest.raises(GlamHipError, match="^proteins lives on a device: it is validated on the host before the launch"):
        ops.panel_plan([5, 6], torch.zeros(1, dtype=torch.int64, device="meta"))
    empty = ops.host_ints(np.zeros((0, 3)), "v", "be a vector")          # nothing in it: int64[0], whatever it was
    assert empty.dtype == np.int64 and empty.shape == (0,)
    assert ops.pair_index([], 0, 0).host.dtype == np.int32 and ops.panel_plan([]).Q == 0


def test_one_staged_copy_holder():
    """The three classes take ``on`` — and with it the per-device cache — from one place (asserted on the classes: a copy needs pinned
    memory, that is a device); the by-protein lists are built once."""
    holder = ops_pair._Staged
    for cls in (ops.PairIndex, ops.PairsByProtein, ops.PanelPlan):
        assert issubclass(cls, holder) and "on" not in vars(cls) and cls.on is holder.on, cls
    ix = ops.pair_index([1, 0, 1], 3, 2)
    assert ix.by_protein() is ix.by_protein() and ix._dev == {} and ix.by_protein()._dev == {}
    assert [p.tolist() for p in ix._parts] == [[1, 0, 1]]
    assert [p.tolist() for p in ix.by_protein()._parts] == [[1, 0, 2], [0, 1, 3]]              # order | ptr: one copy, cut at len(order)
    plan = ops.panel_plan([70, 3], [1, 0])
    assert plan._parts[0] is plan.sel and plan._parts[1] is plan.work and plan._dev == {}


def test_pair_count_of_whichever_index_is_given():
    ix = ops.pair_index([0, 1, 1, 0], 4, 2)
    assert ops.pair_count(None, None) is None and ops.pair_count(None, None, 7) == 7
    assert ops.pair_count([0, 1, 2], None) == 3 and ops.pair_count(None, np.zeros(5, dtype=np.int64), 7) == 5
    assert ops.pair_count(ix, None) == 4 and ops.pair_count(None, ix, 7) == 4
    assert ops.pair_count([0, 1], ix) == 2, "the first one given decides; pair_index then refuses the other"
    assert ops.pair_count(ix) == 4 and ops.pair_count(None) is None


_KW = dict(e_dim=64, message_steps=2, pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU", graph_do="_None()", end_do="_None()")
_SLOTS = ("pre_norm", "graph_norm", "flat_norm", "end_norm")
_NORMS = ("_None", "_BatchNorm", "_LayerNorm", "_PairNorm", "_GraphSizeNorm")
# the refusals test_screen_host / test_ddi_pairs_host (inference) and test_dti_shared_host / test_ddi_shared_host (forward_shared) list
_REFUSED = {("flat_norm", "_LayerNorm"), ("flat_norm", "_PairNorm"), ("flat_norm", "_GraphSizeNorm"), ("graph_norm", "_GraphSizeNorm"),
            ("pre_norm", "_GraphSizeNorm")}
_REFUSED_TRAINING = {("pre_norm", "_BatchNorm"), ("graph_norm", "_BatchNorm"), ("flat_norm", "_BatchNorm")}


def _outcome(f):
    try:
        f()
    except GlamHipError as e:
        return str(e)
    return None


@pytest.mark.parametrize("cls,words,guard", [(model.ArchitectureDTI, model._DTI_WORDS, "_screen_guard"),
                                             (model.ArchitectureDDI, model._DDI_WORDS, "_pairs_guard")])
def test_model_guards_built_from_slots_agree_with_the_methods(cls, words, guard):
    rng = np.random.default_rng(4)
    mb = synth_batch(4, seed=3)
    if cls is model.ArchitectureDTI:
        pros = Batch.from_data_list([synth_protein(rng, 40, 60) for _ in range(2)])
        shared = lambda net: net.forward_shared(mb, pros, [0, 1, 1, 0])       # noqa: E731
    else:
        shared = lambda net: net.forward_shared(mb, mb, [0, 1, 3, 2], [1, 1, 0, 2])       # noqa: E731
    for slot in _SLOTS:
        for norm in _NORMS:
            net = cls(**_KW, **{slot: norm}).eval()
            with torch.no_grad():
                direct = _outcome(lambda: model._inference_guard(net, "encode", words))
                assert direct == _outcome(lambda: getattr(net, guard)("encode")), (slot, norm)
            assert (direct is not None) == ((slot, norm) in _REFUSED), (slot, norm)
            if direct is not None:
                assert f"norm {norm}" in direct and f"depends on how often each {words['thing']}" in direct and words["call"] in direct
            for training in (False, True):
                net.train(training)
                direct = _outcome(lambda: model._shared_guard(net, words))
                refused = (slot, norm) in _REFUSED or (training and (slot, norm) in _REFUSED_TRAINING)
                assert (direct is not None) == refused, (slot, norm, training)
                called = _outcome(lambda: shared(net))
                assert called == direct if refused else "HIP device only" in called, (slot, norm, training)
    net = cls(**_KW)
    with torch.no_grad():
        assert "training mode" in _outcome(lambda: model._inference_guard(net, "encode", words))
    assert "no_grad" in _outcome(lambda: model._inference_guard(net.eval(), "encode", words))
    with torch.no_grad():
        stale = _outcome(lambda: model._check_encoding(net, "call", object(), model.ProteinEncoding, None, "rows", words))
        assert stale.startswith("call: the encoding was made by another model") and f"{words['encode']}() on this one" in stale


# ---- the table calls: one plan cache, one rows head, one panel launch ------------------------------------------------------------
class _Sp:
    B, N = 4, 87
    ptr = torch.tensor([0, 5, 75, 78, 87], dtype=torch.int32)


def _counting_sizes():
    calls = []

    def sizes():
        calls.append(1)
        return np.asarray([5, 70, 3, 9])
    return sizes, calls


@pytest.mark.parametrize("make_plan", [ops.panel_plan, ops.grid_plan])
def test_plan_cache_keys_laziness_and_eviction(make_plan):
    sizes, calls = _counting_sizes()
    plans = {}
    every = model._cached_plan(plans, make_plan, _Q, None, sizes, 16)
    some = model._cached_plan(plans, make_plan, _Q, [2, 0, 2], sizes, 16)
    assert list(plans) == [None, (2, 0, 2)] and plans[None] is every and plans[(2, 0, 2)] is some
    assert every.sel.tolist() == [0, 1, 2, 3] and some.sel.tolist() == [2, 0, 2] and some.Q == _Q and some.N == 87
    sizes, calls = _counting_sizes()
    plans = {}
    first = model._cached_plan(plans, make_plan, _Q, [2, 0, 2], sizes, 16)
    assert model._cached_plan(plans, make_plan, _Q, np.asarray([2, 0, 2]), sizes, 16) is first and len(calls) == 1 and len(plans) == 1
    # a selection that is refused: before the sizes are asked for, and nothing is kept
    sizes, calls = _counting_sizes()
    plans = {}
    with pytest.raises(IndexError, match=r"must lie in \[0, 4\)"):
        model._cached_plan(plans, make_plan, _Q, [1, 4], sizes, 16)
    assert calls == [] and plans == {}
    # first in, first out at the bound; no bound, no eviction
    for bound, left in ((16, 16), (None, 17)):
        plans = {}
        for n in range(17):
            model._cached_plan(plans, make_plan, _Q, [0] * (n + 1), sizes, bound)
        assert len(plans) == left and ((0,) in plans) is (bound is None) and list(plans)[-1] == (0,) * 17
    # a plan the caller calls stale is made again, under its key
    old = plans[(0,)]
    assert model._cached_plan(plans, make_plan, _Q, [0], sizes, None, stale=lambda p: False) is old
    new = model._cached_plan(plans, make_plan, _Q, [0], sizes, None, stale=lambda p: p is old)
    assert new is not old and plans[(0,)] is new and len(plans) == 17


def test_the_three_plan_caches_go_through_the_helper(monkeypatch):
    import types
    dti, ddi = model.ArchitectureDTI(**_KW), model.ArchitectureDDI(**_KW)
    penc = model.ProteinEncoding(dti, [None, None], _Sp(), None, dti._protein_stamp())
    denc = model.DrugEncoding(ddi, [None, None], [None, None], _Sp(), None, None, ddi._drug_stamp())
    penc.prosum, denc.sum1, denc.sum2 = [], [], []          # (filled: no segment sum on this machine)
    data_pro = types.SimpleNamespace()
    # for real: the keys, the one read-back per holder, the batch's unbounded dict and its re-validation
    assert penc.panel([2, 0, 2]) is penc.plans[(2, 0, 2)] and penc.panel(None) is penc.plans[None] and list(penc.plans) == [(2, 0, 2), None]
    assert denc.grid([1]) is denc.plans[(1,)] and denc.grid([1]).N == 87
    assert penc.sizes_host.tolist() == denc.sizes_host.tolist() == [5, 70, 3, 9]
    plan = dti._panel_plan(data_pro, _Sp(), [3, 3])
    kept = data_pro.__dict__["_glam_panel_plans"]
    assert kept["plans"] == {(3, 3): plan} and kept["sizes"].tolist() == [5, 70, 3, 9] and dti._panel_plan(data_pro, _Sp(), [3, 3]) is plan
    other = _Sp()
    other.ptr, other.N = torch.tensor([0, 5, 75, 78, 90], dtype=torch.int32), 90
    again = dti._panel_plan(data_pro, other, [3, 3])
    assert again is not plan and again.N == 90 and kept["plans"] == {(3, 3): again} and kept["sizes"].tolist() == [5, 70, 3, 12]
    # ... and all three through the one function
    seen = []

    def spy(plans, make_plan, Q, selection, sizes, bound=None, stale=None):
        seen.append((plans, make_plan, Q, selection, bound))
        return "the plan"
    monkeypatch.setattr(model, "_cached_plan", spy)
    assert penc.panel([1]) == denc.grid([2]) == dti._panel_plan(data_pro, _Sp(), [0]) == "the plan"
    assert seen[0] == (penc.plans, ops.panel_plan, 4, [1], 16) and seen[0][0] is penc.plans
    assert seen[1] == (denc.plans, ops.grid_plan, 4, [2], 16) and seen[1][0] is denc.plans
    assert seen[2] == (kept["plans"], ops.panel_plan, 4, [0], None) and seen[2][0] is kept["plans"]


class _Block:
    """What the rows head sees of a ``LinearBlock``: a call and ``.linear`` — here the bare ``torch.nn.Linear``, counted."""

    def __init__(self, n_in, n_out, gen):
        self.linear = torch.nn.Linear(n_in, n_out).double()
        with torch.no_grad():
            self.linear.weight.copy_(torch.randint(-3, 4, (n_out, n_in), generator=gen))
            self.linear.bias.copy_(torch.randint(-3, 4, (n_out,), generator=gen))
        self.outputs = []

    def __call__(self, x):
        self.outputs.append(self.linear(x))
        return self.outputs[-1]


def _integer_table(R, Cs, steps=2, hid=3, e_dim=5, out_dim=2):
    """Integer-valued fp64 operands (every sum is exact, in any order) and the head entry by entry."""
    gen = torch.Generator().manual_seed(R * 10 + Cs)
    net = type("Head", (), {})()
    net.lin_out0, net.lin_out1 = _Block(2 * hid + 2 * steps, e_dim, gen), _Block(e_dim, out_dim, gen)
    a = torch.randint(-4, 5, (R, hid), generator=gen).double()
    b = torch.randint(-4, 5, (Cs, hid), generator=gen).double()
    fusion = [torch.randint(-4, 5, (R, Cs, 2), generator=gen).double() for _ in range(steps)]
    want = torch.zeros(R, Cs, out_dim, dtype=torch.float64)
    with torch.no_grad():
        for i in range(R):
            for j in range(Cs):
                want[i, j] = net.lin_out1.linear(net.lin_out0.linear(torch.cat([a[i], b[j]] + [f[i, j] for f in fusion])))
    return net, a, b, fusion, want


@pytest.mark.parametrize("per_block", [1, 2, 5, 7, 0])          # 0: once per column
def test_rows_head_over_a_table_entry_by_entry(per_block):
    R, Cs = 5, 3
    net, a, b, fusion, want = _integer_table(R, Cs)
    with torch.no_grad():
        out = model._table_head_rows(net, a, b, fusion, R, Cs, per_block)
    assert out.shape == want.shape and out.dtype == want.dtype and torch.equal(out, want)
    calls = Cs if per_block == 0 else -(-R // per_block)
    assert len(net.lin_out0.outputs) == len(net.lin_out1.outputs) == calls
    if per_block >= R:          # one block covers the table: what the head wrote, not a copy of it
        assert out.untyped_storage().data_ptr() == net.lin_out1.outputs[0].untyped_storage().data_ptr()


@pytest.mark.parametrize("R,Cs", [(0, 3), (5, 0), (0, 0)])
@pytest.mark.parametrize("per_block", [0, 4])
def test_rows_head_of_an_empty_table(R, Cs, per_block):
    net, a, b, fusion, _ = _integer_table(R, Cs)
    out = model._table_head_rows(net, a, b, fusion, R, Cs, per_block)
    assert out.shape == (R, Cs, 2) and out.dtype == torch.float64 and not out.any()
    assert net.lin_out0.outputs == [] and net.lin_out1.outputs == []


def test_fusion_columns_side_by_side():
    R, Cs, steps = 2, 3, 3
    fusion = [torch.arange(R * Cs * 2, dtype=torch.float32).view(R, Cs, 2) + 100 * s for s in range(steps)]
    cols = model._fusion_columns(fusion, R, Cs, fusion[0])
    assert cols.shape == (R, Cs, 2 * steps)
    for s in range(steps):
        for i in range(R):
            for j in range(Cs):
                for c in range(2):
                    assert cols[i, j, 2 * s + c] == fusion[s][i, j, c]
    like = torch.zeros(1, dtype=torch.float64)
    for r, c in ((0, 3), (2, 0)):
        empty = model._fusion_columns([f[:r, :c] for f in fusion], r, c, like)
        assert empty.shape == (r, c, 2 * steps) and empty.dtype == torch.float64
    assert model._fusion_columns([], R, Cs, like) is None


def test_panel_forward_has_one_launch_site(monkeypatch):
    import inspect
    assert inspect.getsource(ops_pair).count("glam_pair_pool_panel_fwd(") == 1
    assert "glam_pair_pool_panel_fwd(" in inspect.getsource(ops_pair._panel_fwd)
    seen = []

    def spy(mol, pro, msp, psp, plan, molsum, prosum, slab, want_arg):
        seen.append((slab, want_arg))
        return torch.zeros(msp.B, plan.Qs, 2), torch.zeros(msp.B, plan.Qs, 2, dtype=torch.int32) if want_arg else None, None, None
    monkeypatch.setattr(ops_pair, "_panel_fwd", spy)
    monkeypatch.setattr(ops_pair, "_operands", lambda who, a, b, *rest: (a, b))       # (the refusal of a CPU matrix)
    plan = ops.panel_plan([5, 70, 3, 9], [2, 0, 2])
    for staged in (plan, plan.by_protein()):                                       # (a copy out of pinned memory needs a device)
        staged._dev[torch.device("cpu")] = tuple(torch.from_numpy(p) for p in staged._parts)
    msp = type("Msp", (), {"B": 2, "N": 6})()
    mol, pro = torch.zeros(6, 15), torch.zeros(87, 15)
    with torch.no_grad():
        assert ops.pair_pool_panel(mol, pro, msp, _Sp(), plan, slab=3).shape == (2, 3, 2)
        assert ops.pair_pool_panel_shared(mol, pro, msp, _Sp(), plan).shape == (2, 3, 2)
    assert seen == [(3, False), (0, True)]
