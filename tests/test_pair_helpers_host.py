"""CPU: the helpers the pair-fusion family shares (``glam_amd/ops_pair.py``, ``glam_amd/model.py``) — the host-vector validator at each of
its three call sites, the one staged-copy holder, "P of whichever index is given", and the model guards built from slots against the
methods that call them."""
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
