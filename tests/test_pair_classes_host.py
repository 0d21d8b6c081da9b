"""CPU: the host side of the class table (``ops.pair_head_classes`` / ``glam_pair_head_classes_fwd``, csrc/pairhead.hip;
``ArchitectureDDI.classify_matrix`` / ``ArchitectureDTI.classify_panel``; ``score="logp"`` of ``matrix_top`` / ``screen_top``) — the C
prototypes against their ctypes rows, the entry point's argument checks by status code, the restatement the GPU tests compare against
(``tests/pair_classes_restated.py``) against the listed head + ``torch.log_softmax`` / ``argmax`` in fp64 (with five wrong restatements
that must fail on inputs built for them), and the refusals of the operator and the model calls: everything that runs before anything is
launched and needs no device."""
import ctypes

import pytest
import torch

from glam_amd import _lib, model, ops, ops_pair
from glam_amd._lib import GlamHipError
from tests import pair_classes_restated as C
from tests import pair_head_restated as H
from tests.test_ddi_matrix_host import _KW, _fake_encoding
from tests.test_host_logic import _header_prototypes, _table_type
from tests.test_panel_host import _fake_encoding as _fake_protein_encoding

NAME = "glam_pair_head_classes_fwd"
WS = "glam_pair_head_classes_workspace_bytes"
_SHAPE = dict(R=5, Cs=7, hid=15, e_dim=70, F=4, out_dim=11)
_SEL = [3, 0, 10, 3]


def test_class_table_prototypes_match_their_signature_rows_and_are_exported():
    protos = _header_prototypes()
    for name in (NAME, WS):
        res, args = _lib.SIGNATURES[name]
        assert (_table_type(res), [_table_type(a) for a in args]) == protos[name], name
        assert hasattr(_lib.load(), name), f"{name} is not exported"
    p, i64, i32, f32, sz = "pointer", ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    head = [p, i64, p, i64, p, i64, i64, i32, i32, p, i64, p, i32, p, p, i32, i32, f32]          # glam_pair_head_fwd's, up to slope
    assert protos["glam_pair_head_fwd"][1][:len(head)] == head
    assert protos[NAME] == (i32, head + [p, i32, p, sz, p, p, p, p, p])
    assert protos[WS] == (sz, [i64, i64, i32, i32])
    assert _lib.ABI_VERSION == 4 and _lib.load().glam_abi_version() == 4
    assert NAME not in _lib.VALUE_RETURNS
    assert getattr(_lib.api(), NAME).errcheck is not None and getattr(_lib.load(), NAME).errcheck is None
    assert ops.pair_head_classes is ops_pair.pair_head_classes and ops.ClassTable is ops_pair.ClassTable
    assert (ops.HEAD_CLASS_TILE, ops.HEAD_MAX_CLASSES, ops.HEAD_MAX_SEL, ops.HEAD_MAX_OUT) == (16, 1024, 8, 8)
    assert ops.ClassTable._fields == ("cls", "logp", "sel", "logits")


def test_class_table_workspace_query():
    """``A`` + ``B`` as for ``glam_pair_head_fwd``, then ``[e_dim + 1, out_dim rounded up to the tile]`` floats: the transposed weight, its bias."""
    ws, T = getattr(_lib.load(), WS), ops.HEAD_CLASS_TILE
    pad = lambda n: (n + T - 1) // T * T                                        # noqa: E731
    for R, Cs, e, o in ((5, 7, 70, 11), (1, 1, 1, 2), (3, 64, 1024, T), (3, 64, 1024, T + 1), (130, 2, 64, 1024)):
        assert ws(R, Cs, e, o) == ((R + Cs) * e + (e + 1) * pad(o)) * 4, (R, Cs, e, o)
    assert ws(5, 7, 70, 11) == _lib.load().glam_pair_head_workspace_bytes(5, 7, 70) + 71 * T * 4
    assert ws(0, 7, 70, 11) == 0 and ws(5, 0, 70, 11) == 0 and ws(5, 7, 0, 11) == 0 and ws(5, 7, 70, 0) == 0 and ws(-1, 7, 70, 11) == 0
    assert ws(1 << 30, 1 << 30, 1024, 2) == (8 << 40) + 1025 * T * 4            # (a size_t product, not an int one)


def test_class_table_entry_point_rejects_bad_arguments_without_a_gpu():
    f = getattr(_lib.load(), NAME)
    fake = ctypes.c_void_p(4096)                                                # (never dereferenced: each call fails a check first)
    need = getattr(_lib.load(), WS)(5, 7, 70, 11)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                               # noqa: E731

    def call(a=fake, lda=15, b=fake, ldb=15, fus=fake, R=5, Cs=7, hid=15, F=4, W0=fake, ldw=34, b0=fake, e_dim=70, w1=fake, b1=fake,
             out_dim=11, act=0, slope=0.0, classes=ints(3, 0, 10, 3), n_sel=4, ws=fake, wsb=need, cls=fake, logp=fake, sel=fake, logits=fake):
        return f(a, lda, b, ldb, fus, R, Cs, hid, F, W0, ldw, b0, e_dim, w1, b1, out_dim, act, slope, classes, n_sel, ws, wsb, cls, logp,
                 sel, logits, None)
    nothing = dict(a=None, b=None, fus=None, W0=None, b0=None, w1=None, b1=None, ws=None, wsb=0, cls=None, logp=None, sel=None, logits=None)
    assert call(R=0, **nothing) == 0 and call(Cs=0, **nothing) == 0             # nothing to do, no device pointer looked at
    assert call(R=0, n_sel=0, classes=None, **nothing) == 0
    limits = (dict(out_dim=1), dict(out_dim=1025), dict(out_dim=0), dict(F=17), dict(F=-1), dict(n_sel=9), dict(n_sel=-1),
              dict(classes=ints(3, 11)), dict(classes=ints(-1, 3)), dict(out_dim=3), dict(classes=None), dict(e_dim=0), dict(hid=0),
              dict(act=3), dict(act=-1))
    for bad in limits + (dict(R=-1), dict(Cs=-1), dict(R=2 ** 31), dict(R=1 << 20, Cs=1 << 20), dict(R=46341, Cs=46341), dict(lda=14),
                         dict(ldb=14), dict(ldw=33)):
        kw = dict(bad)
        if "classes" in kw and kw["classes"] is not None:
            kw["n_sel"] = 2
        assert call(**kw) == _lib.GLAM_E_INVALID, bad
        assert call(**{**nothing, **kw}) == _lib.GLAM_E_INVALID, bad              # ... before the device pointers are looked at
    for bad in limits:                                                          # the limits hold for an empty table too
        kw = dict(bad)
        if "classes" in kw and kw["classes"] is not None:
            kw["n_sel"] = 2
        assert call(R=0, **kw) == _lib.GLAM_E_INVALID, bad
    for name in ("a", "b", "fus", "W0", "b0", "w1", "b1", "ws", "cls", "logp", "sel"):
        assert call(**{name: None}) == _lib.GLAM_E_INVALID, name
    for name in ("a", "b", "fus", "W0", "b0", "w1", "b1", "ws", "cls", "logp", "sel", "logits"):
        assert call(**{name: ctypes.c_void_p(4098)}) == _lib.GLAM_E_INVALID, name                      # not a dword boundary
    assert call(wsb=need - 1) == _lib.GLAM_E_INVALID                            # one byte short
    assert call(wsb=_lib.load().glam_pair_head_workspace_bytes(5, 7, 70)) == _lib.GLAM_E_INVALID        # the factored head's is too small
    api = getattr(_lib.api(), NAME)
    none18 = (None, 15, None, 15, None, 5, 7, 15, 4, None, 34, None, 70, None, None)
    with pytest.raises(GlamHipError, match=NAME + ".*null pointer"):
        api(*none18, 11, 0, 0.0, None, 0, None, 0, None, None, None, None, None)
    with pytest.raises(GlamHipError, match="out_dim=1025 not in 2..1024"):
        api(*none18, 1025, 0, 0.0, None, 0, None, 0, None, None, None, None, None)
    with pytest.raises(GlamHipError, match="n_sel=9 selected classes not in 0..8"):
        api(*none18, 11, 0, 0.0, None, 9, None, 0, None, None, None, None, None)
    with pytest.raises(GlamHipError, match=r"classes\[1\]=11 not in \[0, 11\)"):
        api(*none18, 11, 0, 0.0, ints(3, 11), 2, None, 0, None, None, None, None, None)


# ---------------------------------------------------------------------------------------------
# the restatement against the listed head + log_softmax / argmax
# ---------------------------------------------------------------------------------------------
def _max_err(a, b):
    return (a - b).abs().max().item()


@pytest.mark.parametrize("act", ["none", "relu", "leaky"])
def test_restated_class_table_equals_the_listed_head_in_fp64(act):
    """5 x 7 pairs, hid = 15, e_dim = 70, F = 4, out_dim = 11: ``log_softmax`` / ``argmax`` of ``lin_out1(lin_out0(cat rows))``."""
    t = H.inputs(**_SHAPE)
    cls, logp, sel, logits = C.classes(*t, act=act, slope=H.ACTS[act][1], classes=_SEL)
    want = H.listed(*t, act=act)
    assert logits.dtype == torch.float64 and logits.shape == (5, 7, 11) and _max_err(logits, want) <= 1e-12
    lsm = torch.log_softmax(want, -1)
    assert cls.shape == (5, 7) and torch.equal(cls, torch.argmax(want, -1))
    assert logp.shape == (5, 7) and _max_err(logp, lsm.max(-1).values) <= 1e-12
    assert sel.shape == (5, 7, 4) and _max_err(sel, lsm[..., _SEL]) <= 1e-12
    assert torch.equal(sel[..., 0], sel[..., 3]), "a class named twice is the same column twice"
    l_cls, l_logp, l_sel, _ = C.listed(*t, act=act, classes=_SEL)
    assert torch.equal(l_cls, cls) and _max_err(l_logp, logp) <= 1e-12 and _max_err(l_sel, sel) <= 1e-12
    assert len(set(cls.reshape(-1).tolist())) >= 4, "the case must call several classes"
    assert (logp < 0).all() and _max_err(torch.logsumexp(lsm, -1), torch.zeros(5, 7, dtype=torch.float64)) <= 1e-12
    empty = C.classes(*t, act=act, slope=H.ACTS[act][1])
    assert empty[2].shape == (5, 7, 0)


def _differs(got, want):
    """Which of ``cls`` / ``logp`` / ``sel`` of a restatement differ from the reference's (NaN equals NaN)."""
    out = []
    if not torch.equal(got[0], want[0]):
        out.append("cls")
    for name, g, w in (("logp", got[1], want[1]), ("sel", got[2], want[2])):
        if not (torch.isnan(g) == torch.isnan(w)).all() or _max_err(torch.nan_to_num(g), torch.nan_to_num(w)) > 1e-6:
            out.append(name)
    return out


@pytest.mark.parametrize("wrong", C.WRONG)
def test_wrong_class_restatements_fail_on_inputs_built_for_them(wrong):
    """Last index on ties (two ``lin1`` rows duplicated with the largest bias); the softmax normalised over the selected classes only;
    ``logp`` of class 0 instead of the called class; ``sel`` as raw logits; NaN as the smallest (one ``f`` entry NaN: that pair's logits
    are all NaN, ``cls`` is 0 either way and the mistake shows as a finite ``logp``; one NaN bias: it shows in ``cls`` too).  The correct
    restatement passes on each of these inputs."""
    t = H.inputs(**_SHAPE)
    if wrong == "last_on_ties":
        t = C.with_tie(t, 2, 9)
    elif wrong == "nan_smallest":
        t = C.with_nan(t, 3, 5)
    want = C.listed(*t, act="relu", classes=_SEL)
    assert _differs(C.classes(*t, act="relu", classes=_SEL), want) == []
    if wrong == "last_on_ties":
        logits = want[3]
        assert torch.equal(logits[..., 2], logits[..., 9]) and (want[0] == 2).all(), "the tie must be exact and the called class"
    if wrong == "nan_smallest":
        assert want[0][3, 5] == 0 and torch.isnan(want[1][3, 5]) and torch.isnan(want[2][3, 5]).all()
        assert torch.isnan(want[1]).sum() == 1, "one pair is NaN, no other"
        # ... and one NaN CLASS (b1[4]): torch.argmax calls it at every pair
        tc = C.with_nan_class(H.inputs(**_SHAPE), 4)
        want_c = C.listed(*tc, act="relu", classes=_SEL)
        assert (want_c[0] == 4).all() and torch.isnan(want_c[1]).all()
        assert _differs(C.classes(*tc, act="relu", classes=_SEL), want_c) == []
        assert _differs(C.classes(*tc, act="relu", classes=_SEL, wrong=wrong), want_c) == ["cls", "logp", "sel"]
    differs = _differs(C.classes(*t, act="relu", classes=_SEL, wrong=wrong), want)
    expected = {"last_on_ties": ["cls"], "softmax_over_selected": ["sel"], "logp_of_class_0": ["logp"], "sel_raw_logits": ["sel"],
                "nan_smallest": ["logp", "sel"]}[wrong]
    assert differs == expected, f"the wrong restatement '{wrong}' shows in {differs}, expected {expected}"


# ---------------------------------------------------------------------------------------------
# ops.pair_head_classes: refused on the host
# ---------------------------------------------------------------------------------------------
def test_pair_head_classes_op_refusals_that_need_no_device():
    a, b, f, W0, b0, w1, b1 = H.inputs(**_SHAPE, dtype=torch.float32)
    with torch.no_grad():
        with pytest.raises(GlamHipError, match="CPU tensor"):
            ops.pair_head_classes(a, b, f, (W0, b0), (w1, b1), classes=_SEL)
        with pytest.raises(GlamHipError, match="pair_head_classes: lin0 must be a torch.nn.Linear"):
            ops.pair_head_classes(a, b, f, W0, (w1, b1))
        with pytest.raises(GlamHipError, match="pair_head_classes: both linear layers must have a bias"):
            ops.pair_head_classes(a, b, f, torch.nn.Linear(34, 70, bias=False), (w1, b1))
        # the selection is looked at before anything needs a device
        with pytest.raises(IndexError, match=r"classes must lie in \[0, 11\)"):
            ops.pair_head_classes(a, b, f, (W0, b0), (w1, b1), classes=[0, 11])
        with pytest.raises(IndexError, match=r"classes must lie in \[0, 11\)"):
            ops.pair_head_classes(a, b, f, (W0, b0), (w1, b1), classes=[-1])
        with pytest.raises(IndexError, match="classes must hold integers"):
            ops.pair_head_classes(a, b, f, (W0, b0), (w1, b1), classes=[1.0])
        with pytest.raises(IndexError, match="classes must be a vector"):
            ops.pair_head_classes(a, b, f, (W0, b0), (w1, b1), classes=[[1, 2]])
        with pytest.raises(GlamHipError, match="9 selected classes.*at most 8"):
            ops.pair_head_classes(a, b, f, (W0, b0), (w1, b1), classes=list(range(9)))
        with pytest.raises(GlamHipError, match="CPU tensor"):                     # eight, a duplicate among them: accepted
            ops.pair_head_classes(a, b, f, (W0, b0), (w1, b1), classes=torch.tensor([0, 1, 2, 3, 4, 5, 6, 0]))
    with pytest.raises(GlamHipError, match=r"pair_head_classes is inference only.*head=\"rows\".*forward_shared"):
        ops.pair_head_classes(a, b, f, torch.nn.Linear(34, 70), (w1, b1))
    with pytest.raises(GlamHipError, match=r"pair_head_classes is inference only"):
        ops.pair_head_classes(a.clone().requires_grad_(True), b, f, (W0, b0), (w1, b1))
    assert ops.class_selection((), 2) == [] and ops.class_selection([1, 0, 1], 2) == [1, 0, 1]


# ---------------------------------------------------------------------------------------------
# the model calls: refused on the host
# ---------------------------------------------------------------------------------------------
def _class_refusals(call, what, make):
    """``call(net)`` on CPU models made by ``make(**kw)``: every refusal of the class route, under the caller's name."""
    with torch.no_grad():
        for end_norm in ("_LayerNorm", "_BatchNorm", "_PairNorm"):
            with pytest.raises(GlamHipError, match=rf"{what}: the class head has no norm.*lin_out0's norm is {end_norm}.*log_softmax"):
                call(make(end_norm=end_norm))
        for end_act in ("CELU", "PReLU", "Sigmoid"):
            with pytest.raises(GlamHipError, match=rf"{what}: the class head applies end_act.*not {end_act}.*head=\"rows\""):
                call(make(end_act=end_act))
        with pytest.raises(GlamHipError, match=rf"{what}: the class head calls one of 2..1024 classes.*out_dim = 1 .*score=\"logit\""):
            call(make(out_dim=1))
        with pytest.raises(GlamHipError, match=rf"{what}: the class head calls one of 2..1024 classes.*out_dim = 1025"):
            call(make(out_dim=1025))
        with pytest.raises(GlamHipError, match=f"{what}: the model is in training mode"):
            call(make().train())
        with pytest.raises(GlamHipError, match=f"{what}: .*another model"):
            call(make(), other=True)
    with pytest.raises(GlamHipError, match=f"{what} is inference only.*no_grad"):
        call(make())


def _ddi(**kw):
    return model.ArchitectureDDI(**{**_KW, "out_dim": 11, **kw}).eval()


def _dti(**kw):
    return model.ArchitectureDTI(**{**_KW, "out_dim": 2, **kw}).eval()


def test_classify_matrix_and_matrix_top_logp_refusals_come_before_any_device_work():
    def enc_of(net, other):
        return _fake_encoding(_ddi() if other else net)

    def matrix(net, other=False, **kw):
        enc = enc_of(net, other)
        try:
            return net.classify_matrix(enc, **kw)
        finally:
            assert enc.sizes_host is None and enc.sum1 is None and enc.plans == {}

    def top(net, other=False, **kw):
        return net.matrix_top(enc_of(net, other), score="logp", **kw)
    _class_refusals(matrix, "classify_matrix", _ddi)
    _class_refusals(top, "matrix_top", _ddi)
    with torch.no_grad():
        net = _ddi()                                                            # out_dim = 11: no head="factored", but a class head
        with pytest.raises(IndexError, match=r"rows must lie in \[0, 3\)"):      # an accepted head goes on to the selections
            matrix(net, rows=[3])
        with pytest.raises(IndexError, match=r"cols must lie in \[0, 3\)"):
            top(net, cols=[3])
        with pytest.raises(IndexError, match=r"classes must lie in \[0, 11\)"):
            matrix(net, classes=[11])
        with pytest.raises(GlamHipError, match="classify_matrix: 9 selected classes"):
            matrix(net, classes=range(9))
        for bad in ("prob", "Logp", "", None, 0):
            with pytest.raises(GlamHipError, match=r"matrix_top: score = .* is not \"logit\""):
                net.matrix_top(_fake_encoding(net), score=bad)
        with pytest.raises(GlamHipError, match="matrix_top: task = 11 is not one of the model's 11 task"):
            top(net, task=11)
        with pytest.raises(GlamHipError, match="matrix_top: k = .* outside the kernels' lists"):
            top(net, k=0)
        # head="factored" at out_dim = 9 still refuses with today's message, on both calls; score="logit" is the default route
        nine = _ddi(out_dim=9)
        for kw in (dict(), dict(score="logit")):
            with pytest.raises(GlamHipError, match=r"score_matrix: head=\"factored\" keeps out_dim accumulators per pair in registers, at "
                                                   r"most 8; this model has out_dim = 9: use head=\"rows\""):
                nine.matrix_top(_fake_encoding(nine), **kw)
        with pytest.raises(GlamHipError, match=r"score_matrix: head=\"factored\" keeps out_dim.*at most 8.*out_dim = 9.*head=\"rows\""):
            nine.score_matrix(_fake_encoding(nine), head="factored")
        with pytest.raises(IndexError, match=r"rows must lie in \[0, 3\)"):      # ... where the class route takes it
            nine.classify_matrix(_fake_encoding(nine), rows=[5])


def test_classify_panel_and_screen_top_logp_refusals_come_before_any_device_work():
    def enc_of(net, other):
        return _fake_protein_encoding(_dti() if other else net)

    def panel(net, other=False, **kw):
        enc = enc_of(net, other)
        try:
            return net.classify_panel(None, enc, **kw)
        finally:
            assert enc.sizes_host is None and enc.prosum is None and enc.plans == {}

    def top_first(net, other=False, **kw):
        return net.screen_top([None], enc_of(net, other), score="logp", **kw)

    def top_empty(net, other=False, **kw):
        return net.screen_top([], enc_of(net, other), score="logp", **kw)
    _class_refusals(panel, "classify_panel", _dti)
    _class_refusals(top_first, "screen_top", _dti)
    _class_refusals(top_empty, "screen_top", _dti)
    with torch.no_grad():
        net = _dti()
        for call in (panel, top_first, top_empty):
            with pytest.raises(IndexError, match=r"proteins must lie in \[0, 3\)"):      # an accepted head goes on to the selection
                call(net, proteins=[3])
        with pytest.raises(IndexError, match=r"classes must lie in \[0, 2\)"):
            panel(net, classes=[2])
        for bad in ("prob", None):
            with pytest.raises(GlamHipError, match=r"screen_top: score = .* is not \"logit\""):
                net.screen_top([None], _fake_protein_encoding(net), score=bad)
        nine = _dti(out_dim=9)
        for kw in (dict(), dict(score="logit")):
            with pytest.raises(GlamHipError, match=r"screen_panel: head=\"factored\" keeps out_dim.*at most 8.*out_dim = 9.*head=\"rows\""):
                nine.screen_top([None], _fake_protein_encoding(nine), head="factored", **kw)


def test_class_head_reads_the_activation_off_the_block():
    for end_act, want in (("_None", ("none", 0.0)), ("ReLU", ("relu", 0.0)), ("LeakyReLU", ("leaky", 0.01)),
                          ("RReLU", ("leaky", (1 / 8 + 1 / 3) / 2))):
        net = _ddi(end_act=end_act, out_dim=86)
        name, slope = model._class_head(net, "classify_matrix")
        assert name == want[0] and slope == pytest.approx(want[1]), end_act
        assert model._class_head(_ddi(end_act=end_act, out_dim=8), "x") == model._factored_head(_ddi(end_act=end_act, out_dim=8), "x")
    with pytest.raises(GlamHipError, match="dropout slot idle"):
        model._class_head(model.ArchitectureDDI(**{**_KW, "out_dim": 11, "end_do": "Dropout(0.2)"}), "classify_matrix")
    with pytest.raises(GlamHipError, match=r"classify_matrix: the class head keeps the 2 \* message_steps.*at most 16"):
        model._class_head(_ddi(message_steps=9), "classify_matrix")
