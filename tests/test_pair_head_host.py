"""CPU: the host side of the factored pair head (``ops.pair_head`` / ``glam_pair_head_fwd``, csrc/pairhead.hip; ``head="factored"`` of
``ArchitectureDDI.score_matrix`` / ``ArchitectureDTI.screen_panel``, ``ArchitectureDDI.matrix_top``) — the C prototypes against their
ctypes rows, the entry point's argument checks by status code, the restatement the GPU tests compare against
(``tests/pair_head_restated.py``) against the listed head of the oracle's ``linear_block`` assembly in fp64 (with four wrong restatements
that must fail), and the refusals of the model calls: everything that runs before anything is launched and needs no device."""
import ctypes

import pytest
import torch

from glam_amd import _lib, model, ops, ops_pair
from glam_amd._lib import GlamHipError
from tests import pair_head_restated as H
from tests.test_ddi_matrix_host import _KW, _fake_encoding
from tests.test_host_logic import _header_prototypes, _table_type
from tests.test_panel_host import _fake_encoding as _fake_protein_encoding

NAME = "glam_pair_head_fwd"
_SHAPE = dict(R=5, Cs=7, hid=15, e_dim=70, F=4, out_dim=3)


def test_pair_head_prototypes_match_their_signature_rows_and_are_exported():
    """Header and ``SIGNATURES`` type for type; a STATUS return that ``api()`` checks; the ABI version stays 4; the library has them."""
    protos = _header_prototypes()
    for name in (NAME, "glam_pair_head_workspace_bytes"):
        res, args = _lib.SIGNATURES[name]
        assert (_table_type(res), [_table_type(a) for a in args]) == protos[name], name
        assert hasattr(_lib.load(), name), f"{name} is not exported"
    p, i64, i32, f32, sz = "pointer", ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert protos[NAME] == (i32, [p, i64, p, i64, p, i64, i64, i32, i32, p, i64, p, i32, p, p, i32, i32, f32, p, sz, p, p])
    assert protos["glam_pair_head_workspace_bytes"] == (sz, [i64, i64, i32])
    assert _lib.ABI_VERSION == 4
    assert NAME not in _lib.VALUE_RETURNS
    assert getattr(_lib.api(), NAME).errcheck is not None and getattr(_lib.load(), NAME).errcheck is None
    assert ops.pair_head is ops_pair.pair_head


def test_pair_head_workspace_query():
    ws = _lib.load().glam_pair_head_workspace_bytes
    assert ws(5, 7, 70) == (5 + 7) * 70 * 4 and ws(1, 1, 1) == 8
    assert ws(0, 7, 70) == 0 and ws(5, 0, 70) == 0 and ws(5, 7, 0) == 0 and ws(-1, 7, 70) == 0
    assert ws(1 << 30, 1 << 30, 1024) == 8 << 40                               # (a size_t product, not an int one)


def test_pair_head_entry_point_rejects_bad_arguments_without_a_gpu():
    f = _lib.load().glam_pair_head_fwd
    fake = ctypes.c_void_p(4096)                                                # (never dereferenced: each call fails a check first)

    def call(a=fake, lda=15, b=fake, ldb=15, fus=fake, R=5, Cs=7, hid=15, F=4, W0=fake, ldw=34, b0=fake, e_dim=70, w1=fake, b1=fake,
             out_dim=3, act=0, slope=0.0, ws=fake, wsb=(5 + 7) * 70 * 4, out=fake):
        return f(a, lda, b, ldb, fus, R, Cs, hid, F, W0, ldw, b0, e_dim, w1, b1, out_dim, act, slope, ws, wsb, out, None)
    nothing = dict(a=None, b=None, fus=None, W0=None, b0=None, w1=None, b1=None, ws=None, wsb=0, out=None)
    assert call(R=0, **nothing) == 0 and call(Cs=0, **nothing) == 0             # nothing to do, nothing dereferenced
    for bad in (dict(out_dim=0), dict(out_dim=9), dict(out_dim=-1), dict(F=17), dict(F=-1), dict(e_dim=0), dict(hid=0), dict(act=3),
                dict(act=-1), dict(R=-1), dict(Cs=-1), dict(R=2 ** 31), dict(R=1 << 20, Cs=1 << 20), dict(R=46341, Cs=46341),
                dict(lda=14), dict(ldb=14), dict(ldw=33)):
        assert call(**bad) == _lib.GLAM_E_INVALID, bad
        assert call(**bad, **nothing) == _lib.GLAM_E_INVALID, bad               # ... before the pointers are looked at
    for bad in (dict(out_dim=9), dict(F=17)):                                   # the limits hold for an empty table too
        assert call(R=0, **bad) == _lib.GLAM_E_INVALID, bad
    for name in ("a", "b", "fus", "W0", "b0", "w1", "b1", "ws", "out"):
        assert call(**{name: None}) == _lib.GLAM_E_INVALID, name
    for name in ("a", "b", "fus", "W0", "b0", "w1", "b1", "ws", "out"):
        assert call(**{name: ctypes.c_void_p(4098)}) == _lib.GLAM_E_INVALID, name                      # not a dword boundary
    assert call(wsb=(5 + 7) * 70 * 4 - 1) == _lib.GLAM_E_INVALID               # one byte short
    with pytest.raises(GlamHipError, match=NAME + ".*null pointer"):
        _lib.api().glam_pair_head_fwd(None, 15, None, 15, None, 5, 7, 15, 4, None, 34, None, 70, None, None, 3, 0, 0.0, None, 0, None, None)
    with pytest.raises(GlamHipError, match="out_dim=9 not in 1..8"):
        _lib.api().glam_pair_head_fwd(None, 15, None, 15, None, 5, 7, 15, 4, None, 34, None, 70, None, None, 9, 0, 0.0, None, 0, None, None)
    with pytest.raises(GlamHipError, match="F=17 fusion columns not in 0..16"):
        _lib.api().glam_pair_head_fwd(None, 15, None, 15, None, 5, 7, 15, 17, None, 47, None, 70, None, None, 3, 0, 0.0, None, 0, None, None)


# ---------------------------------------------------------------------------------------------
# the restatement against the listed head
# ---------------------------------------------------------------------------------------------
def _max_err(a, b):
    return (a - b).abs().max().item()


@pytest.mark.parametrize("act", ["none", "relu", "leaky"])
def test_restated_factored_head_equals_the_listed_head_in_fp64(act):
    """5 x 7 pairs, hid = 15, e_dim = 70, F = 4, out_dim = 3: ``lin_out1(lin_out0(cat rows))`` of the oracle's ``linear_block``."""
    t = H.inputs(**_SHAPE)
    want = H.listed(*t, act=act)
    got = H.factored(*t, act=act, slope=H.ACTS[act][1])
    assert got.shape == want.shape == (5, 7, 3) and got.dtype == torch.float64
    assert _max_err(got, want) <= 1e-12
    hidden = H.pair_rows(*t[:3]) @ t[3].T + t[4]
    assert (hidden > 0).any() and (hidden < 0).any(), "the case must take both branches of the activation"
    no_f = H.inputs(**{**_SHAPE, "F": 0})
    assert no_f[2] is None and _max_err(H.factored(*no_f, act=act, slope=H.ACTS[act][1]), H.listed(*no_f, act=act)) <= 1e-12


@pytest.mark.parametrize("act", ["none", "relu", "leaky"])
@pytest.mark.parametrize("wrong", H.WRONG)
def test_wrong_restatements_fail_on_these_inputs(wrong, act):
    """The comparison above sees each mistake the factoring invites: the activation applied before ``B`` is added, the fusion term
    dropped, ``Wf`` read from column ``hid`` instead of ``2 * hid``, the bias added on both sides."""
    t = H.inputs(**_SHAPE)
    err = _max_err(H.factored(*t, act=act, slope=H.ACTS[act][1], wrong=wrong), H.listed(*t, act=act))
    if wrong == "act_before_b" and act == "none":
        assert err <= 1e-12, "without an activation there is nothing to misplace"
    else:
        assert err > 1e-6, f"the wrong restatement '{wrong}' passes with act = {act} (max|d| = {err:.1e})"


# ---------------------------------------------------------------------------------------------
# ops.pair_head: refused on the host
# ---------------------------------------------------------------------------------------------
def test_pair_head_op_refusals_that_need_no_device():
    a, b, f, W0, b0, w1, b1 = H.inputs(**_SHAPE, dtype=torch.float32)
    with torch.no_grad():
        with pytest.raises(GlamHipError, match="CPU tensor"):
            ops.pair_head(a, b, f, (W0, b0), (w1, b1))
        with pytest.raises(GlamHipError, match="lin0 must be a torch.nn.Linear"):
            ops.pair_head(a, b, f, W0, (w1, b1))
        with pytest.raises(GlamHipError, match="must have a bias"):
            ops.pair_head(a, b, f, torch.nn.Linear(34, 70, bias=False), (w1, b1))
    lin0 = torch.nn.Linear(34, 70)
    with pytest.raises(GlamHipError, match=r"inference only.*head=\"rows\".*forward_shared"):
        ops.pair_head(a, b, f, lin0, (w1, b1))
    with pytest.raises(GlamHipError, match=r"inference only.*head=\"rows\""):
        ops.pair_head(a.clone().requires_grad_(True), b, f, (W0, b0), (w1, b1))


# ---------------------------------------------------------------------------------------------
# the model calls: head= refused on the host
# ---------------------------------------------------------------------------------------------
def _refusals(call, what, make, out9):
    """``call(net, **kw)`` on CPU models made by ``make(**kw)``: every ``head=`` refusal, with a message that names ``head="rows"``."""
    with torch.no_grad():
        for end_norm in ("_LayerNorm", "_BatchNorm", "_PairNorm"):
            with pytest.raises(GlamHipError, match=rf"{what}: head=\"factored\" has no norm.*lin_out0's norm is {end_norm}.*head=\"rows\""):
                call(make(end_norm=end_norm), head="factored")
        for end_act in ("CELU", "PReLU", "Sigmoid"):
            with pytest.raises(GlamHipError, match=rf"{what}: head=\"factored\" applies end_act.*not {end_act}.*head=\"rows\""):
                call(make(end_act=end_act), head="factored")
        with pytest.raises(GlamHipError, match=rf"{what}: head=\"factored\" keeps out_dim.*at most 8.*out_dim = 9.*head=\"rows\""):
            call(out9, head="factored")
        for bad in ("Rows", "", None, 1, "factor"):
            with pytest.raises(GlamHipError, match=rf"{what}: head = .* is not \"rows\""):
                call(make(), head=bad)


def test_score_matrix_and_matrix_top_head_refusals_come_before_any_device_work():
    def make(**kw):
        return model.ArchitectureDDI(**{**_KW, **kw}).eval()

    def matrix(net, **kw):
        enc = _fake_encoding(net)
        try:
            return net.score_matrix(enc, **kw)
        finally:
            assert enc.sizes_host is None and enc.sum1 is None and enc.plans == {}

    def top(net, **kw):
        return net.matrix_top(_fake_encoding(net), **kw)
    for call in (matrix, top):
        _refusals(call, "score_matrix", make, make(out_dim=9))
    with torch.no_grad():
        for bad in (5, -1, 2.5, True):
            with pytest.raises(GlamHipError, match="block_pairs"):
                matrix(make(), head="factored", block_pairs=bad)
        with pytest.raises(GlamHipError, match=r"score_matrix: block_pairs = 5 .*head=\"rows\".*no blocks"):
            matrix(make(), head="factored", block_pairs=5)
        with pytest.raises(IndexError, match=r"rows must lie in \[0, 3\)"):      # an accepted head goes on to the selections
            matrix(make(), head="factored", rows=[3])
        for end_act in ("_None", "ReLU", "LeakyReLU", "RReLU"):
            with pytest.raises(IndexError, match=r"cols must lie in \[0, 3\)"):
                matrix(make(end_act=end_act), head="factored", cols=[3])
        # matrix_top: its own checks, then score_matrix's guards with their own messages
        net = make(out_dim=2)
        for k in (0, 1025):
            with pytest.raises(GlamHipError, match="matrix_top: k = .* outside the kernels' lists"):
                top(net, k=k)
        with pytest.raises(GlamHipError, match="matrix_top: k must be an integer"):
            top(net, k=10.5)
        for task in (2, -1, 1.0, None, True):
            with pytest.raises(GlamHipError, match="matrix_top: task = .* not one of the model's 2 task"):
                top(net, task=task)
        for bad in (-1, 2.5, True):
            with pytest.raises(GlamHipError, match="matrix_top: block_rows"):
                top(net, block_rows=bad)
        for head in ("factored", "rows"):
            with pytest.raises(IndexError, match=r"rows must lie in \[0, 3\)"):
                top(net, rows=[0, 3], head=head)
            with pytest.raises(IndexError, match=r"cols must lie in \[0, 3\)"):
                top(net, cols=[-1], head=head)
            with pytest.raises(GlamHipError, match="score_matrix: .*another model"):
                make(out_dim=2).matrix_top(_fake_encoding(net), head=head)
        with pytest.raises(GlamHipError, match="score_matrix: the model is in training mode"):
            top(model.ArchitectureDDI(**_KW))
    with pytest.raises(GlamHipError, match="score_matrix is inference only.*no_grad"):
        top(make())


def test_screen_panel_and_screen_top_head_refusals_come_before_any_device_work():
    def make(**kw):
        return model.ArchitectureDTI(**{**_KW, **kw}).eval()

    def panel(net, **kw):
        enc = _fake_protein_encoding(net)
        try:
            return net.screen_panel(None, enc, **kw)
        finally:
            assert enc.sizes_host is None and enc.prosum is None and enc.plans == {}

    def top_first(net, **kw):
        return net.screen_top([None], _fake_protein_encoding(net), **kw)

    def top_empty(net, **kw):
        return net.screen_top([], _fake_protein_encoding(net), **kw)
    for call in (panel, top_first, top_empty):
        _refusals(call, "screen_panel", make, make(out_dim=9))
    with torch.no_grad():
        for call in (panel, top_first, top_empty):
            with pytest.raises(IndexError, match=r"proteins must lie in \[0, 3\)"):      # an accepted head goes on to the selection
                call(make(), proteins=[3], head="factored")


def test_factored_head_reads_the_activation_off_the_block():
    for end_act, want in (("_None", ("none", 0.0)), ("ReLU", ("relu", 0.0)), ("LeakyReLU", ("leaky", 0.01)),
                          ("RReLU", ("leaky", (1 / 8 + 1 / 3) / 2))):
        net = model.ArchitectureDDI(**{**_KW, "end_act": end_act}).eval()
        name, slope = model._factored_head(net, "score_matrix")
        assert name == want[0] and slope == pytest.approx(want[1]), end_act
    net = model.ArchitectureDDI(**{**_KW, "end_act": "RReLU"})                  # a training-mode RReLU draws its slopes
    with pytest.raises(GlamHipError, match="not RReLU"):
        model._factored_head(net, "score_matrix")
    net = model.ArchitectureDDI(**{**_KW, "end_do": "Dropout(0.2)"})
    with pytest.raises(GlamHipError, match="dropout slot idle"):
        model._factored_head(net, "score_matrix")
    assert model._factored_head(net.eval(), "score_matrix") == ("relu", 0.0)    # ... and is idle in eval()
    with pytest.raises(GlamHipError, match="at most 16"):
        model._factored_head(model.ArchitectureDDI(**{**_KW, "message_steps": 9}).eval(), "score_matrix")
