"""GPU (MI355X): the training-mode kernels — every entry point that draws from the device-side Philox stream (csrc/rng.h) — against
fp64 references UNDER THE NOISE THAT WAS ACTUALLY DRAWN.

The stream is public (tests/philox_twin.py restates it on the host): element ``i`` of the tensor as stored draws word ``i % 4`` of
``philox4(i / 4)`` at the ``(seed, offset)`` the launch recorded in ``eff``; the RReLU slope comes from the word's high half, the
Dropout decision from its low half.  So the slope and the mask of every element of every launch are known exactly, and RReLU / Dropout
become ordinary deterministic functions with fp64 references, like the eval-mode forms.

Every test owns its state tensor, writes seed and starting offset straight into it, and after each forward checks ``eff``, the advanced
offset and the ticket words.  Outputs start as NaN and none may stay.  No element is excluded from any comparison: where the side of
zero matters the twin takes it from the device's own ``out`` (``out > 0`` iff the pre-activation is, because ``lower > 0``), and the test
asserts that this side agrees with the fp64 pre-activation wherever that exceeds the case's tolerance.

Which case calls which entry point:

  (a) test_elementwise_*                   glam_bias_res_act_rng_fwd / _bwd
  (b) test_gru_tail                        glam_gru_tail_rng_fwd / _bwd
  (c) test_gru_step                        glam_gru_fused_rng_fwd, glam_gru_ws_rng_fwd, _xc, _pre, _pre_node, glam_gru_bwd_ws_rng, _rng_pre
  (d) test_embedding_epilogues             glam_ts_gemm_rrelu, glam_ts_gemm_act_node (+ glam_bias_res_act_rng_bwd)
  (e) test_head                            glam_linear_narrow_act_fwd / _bwd
  (f) test_graph_norm_dropout              glam_graph_norm_drop_fwd / _bwd
  (g) test_one_launch_sequence             eight launches of six kinds on one state
  (h) test_python_surface_*                ops.rrelu, ops.dropout, ops.linear_rrelu, ops.rrelu_dropout_linear_narrow, layer.MessageBlock
"""
import os

import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, layer, ops
from glam_amd.data import synth_batch
from tests import graph_norm_cases as GC
from tests import philox_twin as pt
from tests.conftest import EPS32, assert_fp32_parity, assert_twin_parity

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
M64 = 2 ** 64 - 1
LO, HI = 0.125, 1.0 / 3
# (seed, starting offset): a small pair, and one with bit 31 set in both halves of the seed (so the seed is negative as the int64 the
# state holds) and an offset whose high word is not 0
STREAMS = [(1234, 0), (0x9E3779B9F4A7C159, 2 ** 32 + 5)]
STREAM_IDS = ["small", "high-bits"]
ELEMENT_TOL = 4 * EPS32          # relative: three or four single roundings of one element (see the assertions)


def _s64(v):
    v &= M64
    return v - 2 ** 64 if v >= 2 ** 63 else v


def new_state(stream, device):
    seed, off = stream
    st = torch.zeros(ops.RNG_STATE_WORDS, dtype=torch.int64)
    st[0], st[1] = _s64(seed), _s64(off)
    return st.to(device), torch.full((2,), -1, dtype=torch.int64, device=device)


def check_state(state, eff, stream, k=0, what=""):
    """After forward launch number ``k`` (from 0) on this state: eff == (seed, offset + k), the seed untouched, the offset advanced
    to offset + k + 1, every ticket word — and every other word of the state — back to 0."""
    seed, off = stream
    s, e = [v & M64 for v in state.cpu().tolist()], [v & M64 for v in eff.cpu().tolist()]
    assert e == [seed, off + k], f"{what}: eff {e} != {(seed, off + k)}"
    assert s[0] == seed, f"{what}: seed changed"
    assert s[1] == off + k + 1, f"{what}: offset {s[1]} != {off + k + 1}"
    assert s[16] == 0 and all(s[32 + 16 * j] == 0 for j in range(16)), f"{what}: a ticket word is not back to 0"
    assert not any(s[2:]), f"{what}: a word of the state beyond (seed, offset) is not 0"


def noise(stream, k, shape, p, lo=LO, hi=HI):
    """``(slopes fp32, keep mask, fl(1 / (1 - p)))`` of launch ``k`` on this stream for a tensor of this shape as stored."""
    w = pt.words(stream[0], stream[1] + k, int(np.prod(shape))).reshape(shape)
    return pt.slopes(w, lo, hi), pt.keep_mask(w, p), pt.drop_scale32(p)


def nan(device, *shape):
    return torch.full(shape, float("nan"), device=device)


def offset_view(t):
    """A contiguous view of ``t``'s values at a storage offset of one float (16-byte alignment broken, in bounds)."""
    flat = torch.cat([t.new_zeros(1), t.reshape(-1)])
    u = flat[1:].view(t.shape)
    assert u.data_ptr() % 16 == 4 and u.is_contiguous()
    return u


def leaf(t, dt):
    """A fresh differentiable copy of ``t`` in ``dt`` (never ``t`` itself: ``t.to(t.dtype)`` is ``t``)."""
    return t.detach().clone().to(dt).requires_grad_(True)


def npf(t):
    return t.detach().cpu().numpy()


def no_nan(*ts):
    for t in ts:
        assert t is None or not torch.isnan(t).any(), "an output element was not written"


def assert_mask_exact(out_drop, out, keep, scale32, what):
    """The dropped twin is ``fl(out * fl(1 / (1 - p)))`` where the twin's mask keeps, 0 where it drops: one IEEE multiply, exact."""
    od, o = npf(out_drop), npf(out)
    want = o * np.where(keep, scale32, np.float32(0.0)).astype(np.float32)
    assert want.dtype == np.float32
    assert np.all(od[~keep] == 0), f"{what}: a dropped element is not 0"
    assert np.all((od != 0)[keep & (o != 0)]), f"{what}: a kept element is 0"
    assert np.array_equal(od, want), f"{what}: out_drop is not out * scale on the twin's mask"


def assert_elementwise(got, ref64, what, tol=ELEMENT_TOL, abs_tol=0.0):
    g, r = npf(got).astype(np.float64), np.asarray(ref64, dtype=np.float64)
    assert g.shape == r.shape and not np.isnan(g).any(), what
    assert np.all(g[r == 0] == 0), f"{what}: not exactly 0 where the reference is"
    err = np.abs(g - r)
    bound = tol * np.abs(r) + abs_tol
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off, worst {float((err / np.maximum(bound, 1e-300)).max()):.2f} x the bound"
    nz = r != 0
    return float((err[nz] / np.abs(r[nz])).max() / tol) if nz.any() and abs_tol == 0 else 0.0


def assert_side(out, pre64, tol, what):
    """``out > 0`` agrees with the fp64 pre-activation wherever that is further than ``tol`` from 0."""
    pos, pre = npf(out) > 0, np.asarray(pre64)
    far = np.abs(pre) > tol
    assert np.array_equal(pos[far], (pre > 0)[far]), f"{what}: the side of zero differs outside the tolerance band"
    return pos


def same_sign_cotangents(g, shape, device):
    """Two cotangents, multiples of 1/8 with exact zeros, that share their sign element by element: the backward's
    ``fma(d_out_drop, scale, d_out)`` then never cancels, which a bound relative to the result presumes."""
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    a = torch.randint(0, 17, shape, generator=g).float() / 8 * sign
    b = torch.randint(0, 17, shape, generator=g).float() / 8 * sign
    return a.to(device), b.to(device)


# ---------------------------------------------------------------------------------------------
# (a) glam_bias_res_act_rng_fwd / _bwd: out = act(y + bias + identity), out_drop = Dropout(p)(out)
# ---------------------------------------------------------------------------------------------
LEAKY = 0.01
# what the forward adds to a bit-exact twin for CELU: expf is within 2 ulp of a value in (0, 1] (ulp <= 2^-24 below 1), the subtraction
# of 1 rounds once more — 4 * 2^-23 absolute is room for both
CELU_ABS = 4 * EPS32


def _elementwise_inputs(N, C, has_bias, has_id, seed):
    """Multiples of 1/8; a quarter of the pre-activations exactly 0 (-0.0 without bias / identity), as in test_bias_res_act."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-16, 17, (N, C), generator=g).float() / 8
    bias = torch.randint(-8, 9, (C,), generator=g).float() / 8
    ident = torch.randint(-8, 9, (N, C), generator=g).float() / 8
    zero = torch.rand(N, C, generator=g) < 0.25
    other = (bias if has_bias else 0) + (ident if has_id else 0)
    y = torch.where(zero, -other if (has_bias or has_id) else torch.full_like(y, -0.0), y)
    return g, y, (bias if has_bias else None), (ident if has_id else None), zero


def _act_twin32(v, act, slope32):
    """The forward in np.float32, operation for operation (CELU: fp64, compared with CELU_ABS)."""
    if act == 4:
        return np.where(v > 0, v, v * slope32)
    if act == 1:
        return np.maximum(v, np.float32(0))
    if act == 2:
        return np.where(v > 0, v, v * np.float32(LEAKY))
    if act == 3:
        return np.where(v > 0, v.astype(np.float64), np.expm1(v.astype(np.float64)))
    return v


def _act_derivative64(out, act, slope32):
    """d act / d pre from the OUTPUT, as the backward takes it; at pre-activation 0 the negative side's (torch's convention)."""
    o = out.astype(np.float64)
    neg = {0: np.ones_like(o), 1: np.zeros_like(o), 2: np.full_like(o, np.float64(np.float32(LEAKY))), 3: o + 1.0,
           4: slope32.astype(np.float64)}[act]
    return np.where(o > 0, 1.0, neg)


def run_elementwise(device, N, C, act, p, has_bias, has_id, stream, cot="both", fwd_view=None, bwd_view=None, null_out=False, k=0,
                    state=None):
    """One forward + one backward of the block tail at the C ABI against the twin.  ``fwd_view`` / ``bwd_view`` name the operand handed
    over as a view at a storage offset of one float (that launch then takes the scalar path whatever C is)."""
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream
    what = f"bias_res_act N={N} C={C} act={act} p={p} bias={has_bias} id={has_id} cot={cot} fwd_view={fwd_view} bwd_view={bwd_view}"
    g, y, bias, ident, zero = _elementwise_inputs(N, C, has_bias, has_id, N * 131 + C + act)
    dev = lambda t: None if t is None else t.to(device)
    view = lambda name, t, which: offset_view(t) if (t is not None and which == name) else t
    yd, bd, idd = view("y", dev(y), fwd_view), view("bias", dev(bias), fwd_view), view("identity", dev(ident), fwd_view)
    out = None if null_out else view("out", nan(device, N, C), fwd_view)
    out_drop = view("out_drop", nan(device, N, C), fwd_view)
    st, eff = new_state(stream, device) if state is None else state
    rc = lib.glam_bias_res_act_rng_fwd(P(yd), P(bd), P(idd), N, C, act, LEAKY, LO, HI, p, P(st), P(eff), P(out), P(out_drop), S())
    assert rc == 0, lib.glam_last_error()
    if state is None:
        check_state(st, eff, stream, k, what)
    no_nan(out, out_drop)
    slope32, keep, scale32 = noise(stream, k, (N, C), p)
    # forward: (y + bias) + identity, then ONE multiply — every step a single IEEE operation (the library is built without contraction)
    v = npf(y)
    if has_bias:
        v = v + npf(bias)
    if has_id:
        v = v + npf(ident)
    assert v.dtype == np.float32
    twin = _act_twin32(v, act, slope32)
    if null_out:
        o_dev = torch.from_numpy(v).to(device)                       # a pure Dropout: what is dropped is the input itself
    else:
        o_dev = out
        o = npf(out)
        if act == 3:
            assert np.array_equal(o[v >= 0], twin[v >= 0].astype(np.float32)) and np.abs(o - twin).max() <= CELU_ABS, f"{what}: out"
        elif act == 4:
            assert np.array_equal(o.view(np.uint32), twin.astype(np.float32).view(np.uint32)), f"{what}: out is not the twin's, bit for bit"
        else:
            assert np.array_equal(o, twin), f"{what}: out"
        assert np.array_equal(o > 0, v > 0), f"{what}: out > 0 must say which side of zero the pre-activation is on"
        assert (npf(zero) & (o == 0)).sum() == npf(zero).sum()
    # out_drop: the mask exactly, the kept values against fp64
    assert_mask_exact(out_drop, o_dev, keep, scale32, what)
    pre64 = v.astype(np.float64)
    out64 = {0: pre64, 1: np.maximum(pre64, 0), 2: np.where(pre64 > 0, pre64, pre64 * np.float64(np.float32(LEAKY))),
             3: np.where(pre64 > 0, pre64, np.expm1(pre64)), 4: pt.rrelu(pre64, pre64, slope32)}[act]
    ratio_f = assert_elementwise(out_drop, pt.dropout(out64, keep, p), what + " out_drop",
                                 abs_tol=CELU_ABS * float(scale32) * (1 + ELEMENT_TOL) if act == 3 else 0.0)
    # backward on the recorded eff
    d_out, d_drop = same_sign_cotangents(g, (N, C), device)
    go = view("d_out", d_out, bwd_view) if cot in ("both", "out") else None
    gd = view("d_out_drop", d_drop, bwd_view) if cot in ("both", "drop") else None
    d_y = view("d_y", nan(device, N, C), bwd_view)
    o_in = None if null_out else view("out", o_dev, bwd_view)
    rc = lib.glam_bias_res_act_rng_bwd(P(o_in), P(go), P(gd), N, C, act, LEAKY, LO, HI, p, P(eff), P(d_y), S())
    assert rc == 0, lib.glam_last_error()
    g64 = (npf(d_out).astype(np.float64) if go is not None else 0.0) + \
        (pt.dropout(npf(d_drop), keep, p) if gd is not None else 0.0)
    deriv = np.ones((N, C)) if null_out else _act_derivative64(npf(o_dev), act, slope32)
    ratio_b = assert_elementwise(d_y, g64 * deriv, what + " d_y")
    return max(ratio_f, ratio_b)


def _report(what, ratio):
    if os.environ.get("GLAM_PARITY_REPORT"):
        print(f"[noise] {what}: worst element at {ratio:.2f} of its bound", flush=True)


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("has_bias,has_id", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("N,C", [(50, 60), (50, 15), (1, 4)])
def test_elementwise_paths_and_addends(device, N, C, has_bias, has_id, stream):
    """The float4 path (C % 4 == 0), the scalar path (C = 15) and the smallest launch (one quad), with and without each addend."""
    _report(f"(a) {N}x{C}", run_elementwise(device, N, C, 4, 0.2, has_bias, has_id, stream))


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("cot", ["out", "drop", "both"])
@pytest.mark.parametrize("act,p", [(4, 0.0), (4, 0.2), (4, 0.5), (0, 0.2), (1, 0.2), (2, 0.2), (3, 0.2)])
@pytest.mark.parametrize("C", [60, 15])
def test_elementwise_activations_and_cotangent_routes(device, C, act, p, cot, stream):
    """RReLU with p in {0, 0.2, 0.5}, Dropout(0.2) behind none / ReLU / LeakyReLU / CELU; the backward given d_out only, d_out_drop
    only, and both."""
    _report(f"(a) act {act} p {p}", run_elementwise(device, 50, C, act, p, True, True, stream, cot=cot))


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("operand", ["y", "identity", "out", "out_drop"])
def test_elementwise_forced_scalar(device, operand, stream):
    """C = 60 with one operand at a storage offset of one float: vector width, scalar path — the same words per element."""
    _report(f"(a) view {operand}", run_elementwise(device, 7, 60, 4, 0.2, True, True, stream, fwd_view=operand))


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("operand", ["d_out", "d_out_drop", "d_y", "out"])
def test_elementwise_vector_forward_scalar_backward(device, operand, stream):
    """Forward on aligned tensors (the float4 path), backward given one misaligned operand (the scalar path): it must regenerate the very
    words the vector path drew."""
    _report(f"(a) mixed {operand}", run_elementwise(device, 50, 60, 4, 0.2, True, True, stream, bwd_view=operand))


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("N,C,p", [(32800, 64, 0.5), (35000, 15, 0.0)])
def test_elementwise_second_trip(device, N, C, p, stream):
    """More work than 2048 blocks x 256 threads take in one sweep (524 800 quads on the vector path, 525 000 elements on the scalar
    path): the grid-stride loop runs twice and the elements of the second trip draw the words of THEIR index.  p = 0.5 and p = 0 are
    multiples of 2^-16, and among this many words some have a low half exactly AT the threshold (asserted): such an element is kept
    (``>=``), so p = 0 keeps everything."""
    assert (N * C // 4 if C % 4 == 0 else N * C) > 2048 * 256
    w = pt.words(stream[0], stream[1], N * C)
    assert ((w & np.uint32(0xFFFF)) == np.uint32(int(p * 65536))).any(), "no element at the threshold: the case cannot tell >= from >"
    _report(f"(a) second trip {N}x{C}", run_elementwise(device, N, C, 4, p, True, False, stream))


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("C,p", [(60, 0.2), (15, 0.5)])
def test_elementwise_pure_dropout(device, C, p, stream):
    """``out = NULL`` with act none: a pure Dropout of the input, forward and backward."""
    _report("(a) pure dropout", run_elementwise(device, 50, C, 0, p, False, False, stream, null_out=True, cot="drop"))


# ---------------------------------------------------------------------------------------------
# (b) glam_gru_tail_rng_fwd / _bwd: torch's GRU gate equations, the skip connection, RReLU, the dropped twin
# ---------------------------------------------------------------------------------------------
def gru_gates(gi, gh, h, C):
    """torch.nn.GRU's gate equations (r, z, n, h') on the two pre-activation matrices."""
    r = torch.sigmoid(gi[:, :C] + gh[:, :C])
    z = torch.sigmoid(gi[:, C:2 * C] + gh[:, C:2 * C])
    n = torch.tanh(gi[:, 2 * C:] + r * gh[:, 2 * C:])
    return r, z, n, (1 - z) * n + z * h


def tail_twin(y, side, slope32, keep, p, dt):
    """``out, out_drop`` of RReLU + Dropout under known noise, differentiable, in ``dt``."""
    sl = torch.from_numpy(slope32).to(dt)
    out = torch.where(side, y, y * sl)
    if dt == F32:
        drop = out * torch.from_numpy(np.where(keep, pt.drop_scale32(p), np.float32(0)).astype(np.float32))
    else:
        drop = out * torch.from_numpy(keep.astype(np.float64)) / (1.0 - float(np.float32(p)))
    return out, drop


def assert_out_exact(out, h_new, identity, slope32, what):
    """Given the device's own h' the tail is one add and one multiply: ``out`` is determined bit for bit, slopes included."""
    y = npf(h_new) + npf(identity) if identity is not None else npf(h_new)
    want = np.where(y > 0, y, y * slope32)
    assert np.array_equal(npf(out).view(np.uint32), want.astype(np.float32).view(np.uint32)), f"{what}: out is not RReLU(h' + identity) on the twin's slopes"


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("ident,hstate", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("N,C", [(333, 60), (17, 24), (17, 15), (0, 60)])
def test_gru_tail(device, N, C, ident, hstate, p, stream):
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream
    what = f"gru_tail N={N} C={C} id={ident} hstate={hstate} p={p}"
    g = torch.Generator().manual_seed(N + C)
    r = lambda *s: torch.randn(*s, generator=g)
    gi, gh, h, idn = r(N, 3 * C), r(N, 3 * C), r(N, C), (r(N, C) if ident else None)
    d_out, d_drop, d_hs = r(N, C), r(N, C), (r(N, C) if hstate else None)
    gi_d, gh_d, h_d, id_d, go_d, gd_d, gs_d = (None if t is None else t.to(device) for t in (gi, gh, h, idn, d_out, d_drop, d_hs))
    st, eff = new_state(stream, device)
    hn, out, drop = nan(device, N, C), nan(device, N, C), nan(device, N, C)
    rc = lib.glam_gru_tail_rng_fwd(P(gi_d), P(gh_d), P(h_d), P(id_d), N, C, 4, 0.0, LO, HI, p, P(st), P(eff), P(hn), P(out), P(drop), S())
    assert rc == 0, lib.glam_last_error()
    if N == 0:
        assert [v & M64 for v in st.cpu().tolist()[:2]] == list(stream) and eff.tolist() == [-1, -1]      # nothing launched, nothing drawn
        return
    check_state(st, eff, stream, 0, what)
    no_nan(hn, out, drop)
    slope32, keep, scale32 = noise(stream, 0, (N, C), p)
    assert_mask_exact(drop, out, keep, scale32, what)
    assert_out_exact(out, hn, idn, slope32, what)
    side = (out > 0).cpu()

    def run(dt):
        leaves = [leaf(t, dt) for t in (gi, gh, h)] + ([leaf(idn, dt)] if ident else [])
        _, _, _, h_new = gru_gates(leaves[0], leaves[1], leaves[2], C)
        y = h_new + leaves[3] if ident else h_new
        o, od = tail_twin(y, side, slope32, keep, p, dt)
        loss = (o * d_out.to(dt)).sum() + (od * d_drop.to(dt)).sum() + ((h_new * d_hs.to(dt)).sum() if hstate else 0)
        return (h_new.detach(), y.detach(), o.detach(), od.detach()), torch.autograd.grad(loss, leaves)

    (hn32, y32, o32, od32), g32 = run(F32)
    (hn64, y64, o64, od64), g64 = run(F64)
    _, b = assert_fp32_parity(hn, hn64, hn32, what + " h_new")
    assert_side(out, y64.numpy(), b + EPS32 * float(y64.abs().max()), what)
    assert_fp32_parity(out, o64, o32, what + " out")
    assert_fp32_parity(drop, od64, od32, what + " out_drop")
    dgi, dgh, dh, did = nan(device, N, 3 * C), nan(device, N, 3 * C), nan(device, N, C), (nan(device, N, C) if ident else None)
    rc = lib.glam_gru_tail_rng_bwd(P(gi_d), P(gh_d), P(h_d), P(out), P(go_d), P(gd_d), P(gs_d), N, C, 4, 0.0, LO, HI, p,
                                   P(eff), P(dgi), P(dgh), P(dh), P(did), S())
    assert rc == 0, lib.glam_last_error()
    no_nan(dgi, dgh, dh, did)
    for name, got, r64, r32 in zip(("d_gi", "d_gh", "d_h", "d_identity"), (dgi, dgh, dh, did), g64, g32):
        assert_fp32_parity(got, r64, r32, f"{what} {name}")


# ---------------------------------------------------------------------------------------------
# (d) glam_ts_gemm_rrelu, glam_ts_gemm_act_node: the embedding product with RReLU, the dropped twin and the node product in its epilogue
# ---------------------------------------------------------------------------------------------
def node_matrices(wn, att, C, H, dt):
    """``[W_node | Wa]`` of a TripletMessage (src_1gp/layer.py:37): Wa's columns h and 4 + h are W_node's head h times the attention's
    first and last third."""
    wn, att = wn.to(dt), att.to(dt)
    wa = torch.zeros(C, 8, dtype=dt)
    for hh in range(H):
        wa[:, hh] = wn[:, hh * C:(hh + 1) * C] @ att[0, hh, :C]
        wa[:, 4 + hh] = wn[:, hh * C:(hh + 1) * C] @ att[0, hh, 2 * C:]
    return wn, wa


def stage_node(lib, device, g, C, H):
    P, S = _lib.ptr, _lib.stream
    r = lambda *s: torch.randn(*s, generator=g)
    HC = H * C
    wn, we, att, wsc, bias = r(C, HC) * 0.2, r(4, HC) * 0.2, r(1, H, 3 * C) * 0.2, r(HC, C) * 0.2, r(C)
    staged = torch.empty(lib.glam_triplet_staged_floats(H, C, 4), device=device)
    d = [t.to(device) for t in (wn, we, att, wsc, bias)]
    assert lib.glam_triplet_stage_params(*[P(t) for t in d], C, H, 4, C, 4, P(staged), S()) == 0, lib.glam_last_error()
    at = lib.glam_triplet_staged_node_fragments(H, C, 4)
    assert 0 <= at < staged.numel(), "no node-product fragments for this shape"
    return wn, att, staged[at:]


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("node", [False, True], ids=["rrelu", "act_node"])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("N,K,M,H", [(17, 32, 64, 2), (1, 16, 28, 3), (1000, 16, 60, 3), (2050, 16, 60, 3)])
def test_embedding_epilogues(device, N, K, M, H, p, node, stream):
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream
    if not _lib.route_enabled("x3"):      # (no k_tall_x3, no such epilogue: the two-launch form is what runs)
        assert lib.glam_ts_gemm_rrelu_supported(K, M) == 0
        return
    what = f"ts_gemm_{'act_node' if node else 'rrelu'} N={N} K={K} M={M} p={p}"
    g = torch.Generator().manual_seed(N + K + M)
    r = lambda *s: torch.randn(*s, generator=g)
    x, w, b = r(N, K), r(M, K) * 0.5, r(M)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    img = torch.empty(lib.glam_ts_gemm_image_bytes(K, M) // 4, device=device)
    assert lib.glam_ts_gemm_make_image(P(wd), K, 1, K, M, P(img), S()) == 0
    st, eff = new_state(stream, device)
    out, drop = nan(device, N, M), (nan(device, N, M) if p > 0 else None)
    if node:
        HC = H * M
        wn, att, nfrag = stage_node(lib, device, g, M, H)
        xw, a_ij = nan(device, N, HC), nan(device, N, 8)
        rc = lib.glam_ts_gemm_act_node(P(xd), K, K, P(img), P(bd), M, N, 4, LO, HI, p, P(st), P(eff), P(out), P(drop), P(nfrag), HC, P(xw), P(a_ij), S())
    else:
        rc = lib.glam_ts_gemm_rrelu(P(xd), K, K, P(img), P(bd), M, N, LO, HI, p, P(st), P(eff), P(out), P(drop), S())
    assert rc == 0, lib.glam_last_error()
    check_state(st, eff, stream, 0, what)
    no_nan(out, drop)
    slope32, keep, scale32 = noise(stream, 0, (N, M), p)
    if p > 0:
        assert_mask_exact(drop, out, keep, scale32, what)
    side = (out > 0).cpu()
    d_out, d_drop = same_sign_cotangents(g, (N, M), device)

    def run(dt):
        pre = x.to(dt) @ w.to(dt).t() + b.to(dt)
        o, od = tail_twin(pre, side, slope32, keep, p, dt)
        res = [pre, o, od]
        if node:
            wn_, wa_ = node_matrices(wn, att, M, H, dt)
            rows = od if p > 0 else o
            res += [rows @ wn_, rows @ wa_]
        return res

    r32, r64 = run(F32), run(F64)
    _, bound = assert_fp32_parity(out, r64[1], r32[1], what + " out")
    assert_side(out, r64[0].numpy(), bound, what)
    if p > 0:
        assert_fp32_parity(drop, r64[2], r32[2], what + " out_drop")
    if node:
        no_nan(xw, a_ij)
        assert_fp32_parity(xw, r64[3], r32[3], what + " xw")
        assert_fp32_parity(a_ij, r64[4], r32[4], what + " a_ij")
    # the backward of the epilogue is glam_bias_res_act_rng_bwd on the recorded eff: the fp64 derivative under the twin's noise
    d_pre = nan(device, N, M)
    rc = lib.glam_bias_res_act_rng_bwd(P(out), P(d_out), P(d_drop) if p > 0 else None, N, M, 4, 0.0, LO, HI, p, P(eff), P(d_pre), S())
    assert rc == 0, lib.glam_last_error()
    g64 = npf(d_out).astype(np.float64) + (pt.dropout(npf(d_drop), keep, p) if p > 0 else 0.0)
    _report(what, assert_elementwise(d_pre, g64 * _act_derivative64(npf(out), 4, slope32), what + " d_pre"))


# ---------------------------------------------------------------------------------------------
# (e) glam_linear_narrow_act_fwd / _bwd: y = Linear(Dropout(p)(RReLU(x))), noise on the flat index n K + k
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("N,K,M", [(17, 64, 1), (333, 128, 2), (1, 64, 16), (2050, 256, 12)])
def test_head(device, N, K, M, p, stream):
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream
    what = f"linear_narrow_act N={N} K={K} M={M} p={p}"
    g = torch.Generator().manual_seed(N + K + M)
    r = lambda *s: torch.randn(*s, generator=g)
    x, w, b, dy = r(N, K), r(M, K) * 0.1, r(M), r(N, M)
    xd, wd, bd, dyd = (t.to(device) for t in (x, w, b, dy))
    st, eff = new_state(stream, device)
    y = nan(device, N, M)
    rc = lib.glam_linear_narrow_act_fwd(P(xd), P(wd), P(bd), N, K, M, LO, HI, p, P(st), P(eff), P(y), S())
    assert rc == 0, lib.glam_last_error()
    check_state(st, eff, stream, 0, what)
    ws = torch.empty(lib.glam_linear_narrow_bwd_workspace_bytes(K, M), dtype=torch.uint8, device=device)
    dx, dw, db = nan(device, N, K), nan(device, M, K), nan(device, M)
    rc = lib.glam_linear_narrow_act_bwd(P(xd), P(wd), P(dyd), N, K, M, LO, HI, p, P(eff), P(dx), P(dw), P(db), P(ws), ws.numel(), S())
    assert rc == 0, lib.glam_last_error()
    no_nan(y, dx, dw, db)
    slope32, keep, _ = noise(stream, 0, (N, K), p)
    side = x > 0                        # the pre-activation is the INPUT here: its side of zero is exact

    def run(dt):
        leaves = [leaf(t, dt) for t in (x, w, b)]
        _, ad = tail_twin(leaves[0], side, slope32, keep, p, dt)
        yy = ad @ leaves[1].t() + leaves[2]
        return yy.detach(), torch.autograd.grad((yy * dy.to(dt)).sum(), leaves)

    (y32, g32), (y64, g64) = run(F32), run(F64)
    assert_fp32_parity(y, y64, y32, what + " y")
    for name, got, r64, r32 in zip(("dx", "dW", "db"), (dx, dw, db), g64, g32):
        assert_fp32_parity(got, r64, r32, f"{what} {name}")
    # dx is 0 exactly where the mask drops (no element of the row's gradient leaks through a dropped input)
    assert np.all(npf(dx)[~keep] == 0), f"{what}: dx behind a dropped element"


# ---------------------------------------------------------------------------------------------
# (f) glam_graph_norm_drop_fwd / _bwd: PairNorm / the graph LayerNorm statistics + the Dropout behind them
# ---------------------------------------------------------------------------------------------
NORM_SIZES = [1, 2, 31, 63, 0]          # 1-row, 2-row, one register pass less one, the largest graph the wave form is chosen for, empty


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("want_y,want_gy,want_add", [(True, True, True), (False, False, False), (True, False, True), (False, True, False)])
@pytest.mark.parametrize("setting", [("pair", 1.0, 1e-5), ("layer", 1.0, 1e-5)], ids=GC.setting_id)
@pytest.mark.parametrize("D", [24, 64])
def test_graph_norm_dropout(device, D, setting, want_y, want_gy, want_add, stream):
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream
    kind, scale, eps = setting
    mode, p, sizes = GC.MODE[kind], 0.2, NORM_SIZES
    what = f"graph_norm_drop D={D} {kind} y={want_y} gy={want_gy} addend={want_add}"
    batch, B = GC.batch_of(sizes), len(sizes)
    N = batch.numel()
    assert lib.glam_graph_norm_drop_supported(N, B, D) == 1 and lib.glam_graph_norm_drop_supported(64 * B, B, D) == 0
    g = torch.Generator().manual_seed(D + mode)
    sd = torch.exp(torch.empty(B, 1).uniform_(-2.3, 2.3, generator=g))
    x = (torch.randn(N, D, generator=g) + torch.empty(B, D).uniform_(-3.0, 3.0, generator=g)[batch]) * sd[batch]
    gy_drop, gy, add = (torch.randn(N, D, generator=g) for _ in range(3))
    sp = ops.SegmentPtr(batch.to(device), B)
    xd = x.to(device)
    st, eff = new_state(stream, device)
    y, yd = (nan(device, N, D) if want_y else None), nan(device, N, D)
    rc = lib.glam_graph_norm_drop_fwd(P(xd), P(sp.ptr), N, B, D, mode, scale, eps, p, P(st), P(eff), P(y), P(yd), S())
    assert rc == 0, lib.glam_last_error()
    check_state(st, eff, stream, 0, what)
    no_nan(y, yd)
    _, keep, scale32 = noise(stream, 0, (N, D), p)
    if want_y:
        assert_mask_exact(yd, y, keep, scale32, what)
    else:
        assert np.all(npf(yd)[~keep] == 0), f"{what}: a dropped element is not 0"
    m64 = torch.from_numpy(keep.astype(np.float64)) / (1.0 - float(np.float32(p)))
    cot = gy_drop.double() * m64 + (gy.double() if want_gy else 0)
    ref = {dt: GC.run_oracle(setting, sizes, x, cot, dt) for dt in (F64, F32)}
    if want_y:
        assert_fp32_parity(y, ref[F64][0], ref[F32][0], what + " y")
    assert_fp32_parity(yd, ref[F64][0] * m64, ref[F32][0] * m64.float(), what + " y_drop")
    one = torch.tensor(sizes)[batch] == 1
    if mode == 0:
        assert (yd.cpu()[one] == 0).all()                                   # a 1-row PairNorm graph: x - mean = 0
    else:
        assert np.all((npf(yd) != 0) == keep), f"{what}: the zeros of y_drop are not the twin's mask"
    dx = nan(device, N, D)
    gy_d, gyd_d, add_d = (gy.to(device) if want_gy else None), gy_drop.to(device), (add.to(device) if want_add else None)
    rc = lib.glam_graph_norm_drop_bwd(P(xd), P(gy_d), P(gyd_d), P(sp.ptr), N, B, D, mode, scale, eps, p, P(eff), P(add_d), P(dx), S())
    assert rc == 0, lib.glam_last_error()
    no_nan(dx)
    extra = add if want_add else torch.zeros_like(add)
    assert_fp32_parity(dx, ref[F64][1] + extra.double(), ref[F32][1] + extra, what + " dx")
    GC.assert_per_graph_parity(dx.cpu(), ref[F64][1] + extra.double(), ref[F32][1] + extra, sizes, what + " dx per graph")


# ---------------------------------------------------------------------------------------------
# (g) one launch sequence on one state, no host synchronisation in between
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
def test_one_launch_sequence(device, stream):
    """Eight RNG launches of six kinds back to back on one state, read back only after the last: launch k must have drawn, for EVERY
    element, the words of offset + k — the first fills the 2048-block grid cap twice over, the second is a single block.  This is what
    catches blocks of one launch reading different stream positions (rng.h: the agent-scope loads of the pair).  Run once."""
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream
    g = torch.Generator().manual_seed(8)
    r = lambda *s: torch.randn(*s, generator=g).to(device)
    st, _ = new_state(stream, device)
    effs = [torch.full((2,), -1, dtype=torch.int64, device=device) for _ in range(8)]
    p = 0.2
    # inputs and outputs of all eight, made before the first launch
    y0, o0, d0 = r(32800, 64), nan(device, 32800, 64), nan(device, 32800, 64)                       # 0: tail, 2048 blocks, two trips
    y1, o1, d1 = r(1, 4), nan(device, 1, 4), nan(device, 1, 4)                                      # 1: tail, one block
    gi, gh, h2, id2 = r(17, 72), r(17, 72), r(17, 24), r(17, 24)                                    # 2: GRU tail
    hn2, o2, d2 = nan(device, 17, 24), nan(device, 17, 24), nan(device, 17, 24)
    x3, w3, b3, y3 = r(333, 128), r(2, 128) * 0.1, r(2), nan(device, 333, 2)                        # 3: the head
    sizes = NORM_SIZES                                                                              # 4: PairNorm + Dropout
    batch = GC.batch_of(sizes)
    sp = ops.SegmentPtr(batch.to(device), len(sizes))
    x4, y4, yd4 = r(batch.numel(), 24), nan(device, batch.numel(), 24), nan(device, batch.numel(), 24)
    x5, d5 = r(50, 15), nan(device, 50, 15)                                                         # 5: a pure Dropout, scalar path
    x6, w6, b6, o6, d6 = r(1000, 16), r(60, 16) * 0.5, r(60), nan(device, 1000, 60), nan(device, 1000, 60)     # 6: embedding epilogue
    y6 = r(1000, 60)                                                  # (without k_tall_x3: one more tail launch in its place)
    x3_route = _lib.route_enabled("x3")
    if x3_route:
        img = torch.empty(lib.glam_ts_gemm_image_bytes(16, 60) // 4, device=device)
        assert lib.glam_ts_gemm_make_image(P(w6), 16, 1, 16, 60, P(img), S()) == 0
    y7, o7, d7 = r(35000, 15), nan(device, 35000, 15), nan(device, 35000, 15)                       # 7: tail, scalar path, two trips
    rcs = [
        lib.glam_bias_res_act_rng_fwd(P(y0), None, None, 32800, 64, 4, 0.0, LO, HI, p, P(st), P(effs[0]), P(o0), P(d0), S()),
        lib.glam_bias_res_act_rng_fwd(P(y1), None, None, 1, 4, 4, 0.0, LO, HI, p, P(st), P(effs[1]), P(o1), P(d1), S()),
        lib.glam_gru_tail_rng_fwd(P(gi), P(gh), P(h2), P(id2), 17, 24, 4, 0.0, LO, HI, p, P(st), P(effs[2]), P(hn2), P(o2), P(d2), S()),
        lib.glam_linear_narrow_act_fwd(P(x3), P(w3), P(b3), 333, 128, 2, LO, HI, p, P(st), P(effs[3]), P(y3), S()),
        lib.glam_graph_norm_drop_fwd(P(x4), P(sp.ptr), batch.numel(), len(sizes), 24, 0, 1.0, 1e-5, p, P(st), P(effs[4]), P(y4), P(yd4), S()),
        lib.glam_bias_res_act_rng_fwd(P(x5), None, None, 50, 15, 0, 0.0, LO, HI, p, P(st), P(effs[5]), None, P(d5), S()),
        (lib.glam_ts_gemm_rrelu(P(x6), 16, 16, P(img), P(b6), 60, 1000, LO, HI, p, P(st), P(effs[6]), P(o6), P(d6), S()) if x3_route else
         lib.glam_bias_res_act_rng_fwd(P(y6), None, None, 1000, 60, 4, 0.0, LO, HI, p, P(st), P(effs[6]), P(o6), P(d6), S())),
        lib.glam_bias_res_act_rng_fwd(P(y7), None, None, 35000, 15, 4, 0.0, LO, HI, p, P(st), P(effs[7]), P(o7), P(d7), S()),
    ]
    assert rcs == [0] * 8, (rcs, lib.glam_last_error())
    # ---- the one read-back ----
    seed, off = stream
    for k, e in enumerate(effs):
        assert [v & M64 for v in e.cpu().tolist()] == [seed, off + k], f"launch {k} recorded {e.tolist()}"
    check_state(st, effs[7], stream, 7, "after the sequence")

    def tail_exact(k, y, o, d, act=4):
        no_nan(o, d)
        sl, keep, sc = noise(stream, k, tuple(y.shape), p)
        want = _act_twin32(npf(y), act, sl).astype(np.float32)
        if o is not None:
            assert np.array_equal(npf(o).view(np.uint32), want.view(np.uint32)), f"launch {k}: slopes of another stream position"
        assert_mask_exact(d, torch.from_numpy(want), keep, sc, f"launch {k}")

    tail_exact(0, y0, o0, d0)
    tail_exact(1, y1, o1, d1)
    sl, keep, sc = noise(stream, 2, (17, 24), p)
    no_nan(hn2, o2, d2)
    assert_out_exact(o2, hn2, id2, sl, "launch 2")
    assert_mask_exact(d2, o2, keep, sc, "launch 2")
    sl, keep, _ = noise(stream, 3, (333, 128), p)
    head = lambda dt: tail_twin(x3.cpu().to(dt), x3.cpu() > 0, sl, keep, p, dt)[1] @ w3.cpu().to(dt).t() + b3.cpu().to(dt)
    assert_fp32_parity(y3, head(F64), head(F32), "launch 3 y")
    _, keep, sc = noise(stream, 4, tuple(x4.shape), p)
    no_nan(y4, yd4)
    assert_mask_exact(yd4, y4, keep, sc, "launch 4")
    tail_exact(5, x5, None, d5, act=0)
    sl, keep, sc = noise(stream, 6, (1000, 60), p)
    no_nan(o6, d6)
    assert_mask_exact(d6, o6, keep, sc, "launch 6")
    if not x3_route:
        tail_exact(6, y6, o6, d6)
    else:
        side = (o6 > 0).cpu()
        emb = lambda dt: tail_twin(x6.cpu().to(dt) @ w6.cpu().to(dt).t() + b6.cpu().to(dt), side, sl, keep, p, dt)[0]
        assert_fp32_parity(o6, emb(F64), emb(F32), "launch 6 out")
    tail_exact(7, y7, o7, d7)


# ---------------------------------------------------------------------------------------------
# (c) the GRU step with its products: glam_gru_fused_rng_fwd, glam_gru_ws_rng_fwd(_xc / _pre / _pre_node), glam_gru_bwd_ws_rng(_pre)
# ---------------------------------------------------------------------------------------------
# form -> (forward entry point, CELU on x, x_celu kept, kept-gates form, merge_identity, separate identity, p, d_hstate)
GRU_FORMS = {
    "fused":     dict(celu=True, keep_xc=False, gates=False, merge=False, ident=True, p=0.2, hstate=True),
    "ws":        dict(celu=False, keep_xc=False, gates=False, merge=False, ident=False, p=0.0, hstate=False),
    "xc":        dict(celu=True, keep_xc=True, gates=False, merge=True, ident=False, p=0.2, hstate=True),
    "pre":       dict(celu=True, keep_xc=False, gates=False, merge=False, ident=True, p=0.2, hstate=True),
    "pre_gates": dict(celu=True, keep_xc=True, gates=True, merge=True, ident=False, p=0.2, hstate=True),
    "pre_node":  dict(celu=False, keep_xc=False, gates=True, merge=False, ident=True, p=0.2, hstate=False),
}
NODE_HEADS = {64: 2, 24: 3, 48: 3, 60: 3}


@pytest.mark.parametrize("stream", STREAMS, ids=STREAM_IDS)
@pytest.mark.parametrize("form", list(GRU_FORMS))
@pytest.mark.parametrize("N,C", [(1, 64), (17, 24), (1000, 48), (2050, 60)])
def test_gru_step(device, N, C, form, stream):
    """``x~ = celu?(x)``, both gate products, torch.nn.GRU's gate equations, the skip connection, RReLU and the dropped twin in one
    launch, in every form: the fp32 fused launch; the warp-specialised launch on the plain images (with and without ``x_celu``), on the
    pre-split image, with the kept gates ``[r | z | n | gh_n]`` instead of both pre-activation matrices, and with the node product of the
    next application.  The backward in one launch (``glam_gru_bwd_ws_rng`` on the transposed images, ``_rng_pre`` on the pre-split one;
    two-matrix and kept-gates form; ``merge_identity`` 0 and 1; CELU differentiated from x and from the kept celu(x)); the fused
    forward's backward is ``glam_gru_tail_rng_bwd`` on its gi / gh."""
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream
    cfg = GRU_FORMS[form]
    celu, gates, merge, p = cfg["celu"], cfg["gates"], cfg["merge"], cfg["p"]
    what = f"gru_step[{form}] N={N} C={C}"
    assert lib.glam_gru_ws_supported(C) == 1
    M = 3 * C
    g = torch.Generator().manual_seed(N + C + len(form))
    r = lambda *s: torch.randn(*s, generator=g)
    x, h, w_ih, w_hh, b_ih, b_hh = r(N, C), r(N, C), r(M, C) * 0.3, r(M, C) * 0.3, r(M), r(M)
    idn = r(N, C) if cfg["ident"] else None
    d_out, d_drop, d_hs = r(N, C), (r(N, C) if p > 0 else None), (r(N, C) if cfg["hstate"] else None)
    xd, hd, wid, whd, bid, bhd, idd, god, gdd, gsd = (None if t is None else t.to(device) for t in (x, h, w_ih, w_hh, b_ih, b_hh, idn, d_out, d_drop, d_hs))
    id_in = hd if merge else idd                          # merge_identity: the skip connection and the GRU state are ONE tensor
    st, eff = new_state(stream, device)
    gi = nan(device, N, 4 * C if gates else M)
    gh = None if gates else nan(device, N, M)
    hn, out, drop = nan(device, N, C), nan(device, N, C), (nan(device, N, C) if p > 0 else None)
    xc = nan(device, N, C) if cfg["keep_xc"] else None
    head = (P(xd), P(hd), P(id_in))
    mid = (P(bid), P(bhd), N, C, int(celu), 4, 0.0, LO, HI, p, P(st), P(eff), P(gi), P(gh), P(hn), P(out), P(drop))
    node = None
    if form == "fused":
        imgs = torch.empty(2, lib.glam_gru_fused_image_bytes() // 4, device=device)
        assert lib.glam_gru_fused_make_images(P(wid), P(whd), C, P(imgs[0]), P(imgs[1]), S()) == 0
        rc = lib.glam_gru_fused_rng_fwd(*head, P(imgs[0]), P(imgs[1]), *mid, S())
    elif form in ("ws", "xc"):
        ia, ib = (torch.empty(lib.glam_ts_gemm_image_bytes(C, M) // 4, device=device) for _ in range(2))
        ta, tb = (torch.empty(lib.glam_ts_gemm_image_bytes(M, C) // 4, device=device) for _ in range(2))
        for w, i, t in ((wid, ia, ta), (whd, ib, tb)):
            assert lib.glam_ts_gemm_make_image(P(w), C, 1, C, M, P(i), S()) == 0
            assert lib.glam_ts_gemm_make_image(P(w), C, 0, M, C, P(t), S()) == 0
        if form == "ws":
            rc = lib.glam_gru_ws_rng_fwd(*head, P(ia), P(ib), *mid, S())
        else:
            rc = lib.glam_gru_ws_rng_fwd_xc(*head, P(ia), P(ib), *mid, P(xc), S())
    else:
        pre = torch.empty(2, lib.glam_gru_ws_pre_bytes(), dtype=torch.uint8, device=device)
        assert lib.glam_gru_ws_make_pre(P(wid), P(whd), C, P(pre[0]), P(pre[1]), S()) == 0
        if form == "pre_node":
            H = NODE_HEADS[C]
            wn, att, nfrag = stage_node(lib, device, g, C, H)
            xw, a_ij = nan(device, N, H * C), nan(device, N, 8)
            node = (wn, att, H, xw, a_ij)
            rc = lib.glam_gru_ws_rng_fwd_pre_node(*head, P(pre[0]), *mid, P(xc), P(nfrag), H * C, P(xw), P(a_ij), S())
        else:
            rc = lib.glam_gru_ws_rng_fwd_pre(*head, P(pre[0]), *mid, P(xc), S())
    assert rc == 0, lib.glam_last_error()
    check_state(st, eff, stream, 0, what)
    no_nan(gi, gh, hn, out, drop, xc)
    slope32, keep, scale32 = noise(stream, 0, (N, C), p)
    if p > 0:
        assert_mask_exact(drop, out, keep, scale32, what)
    assert_out_exact(out, hn, h if merge else idn, slope32, what)
    side = (out > 0).cpu()

    def run(dt):
        L = {k: leaf(t, dt) for k, t in dict(x=x, h=h).items()}
        if idn is not None:
            L["id"] = leaf(idn, dt)
        xt = torch.nn.functional.celu(L["x"]) if celu else L["x"]
        a = xt @ w_ih.to(dt).t() + b_ih.to(dt)
        b = L["h"] @ w_hh.to(dt).t() + b_hh.to(dt)
        a.retain_grad(), b.retain_grad()
        rr, zz, nn_, h_new = gru_gates(a, b, L["h"], C)
        skip = L["h"] if merge else L.get("id")
        y = h_new + skip if skip is not None else h_new
        o, od = tail_twin(y, side, slope32, keep, p, dt)
        loss = (o * d_out.to(dt)).sum() + ((od * d_drop.to(dt)).sum() if p > 0 else 0) + ((h_new * d_hs.to(dt)).sum() if d_hs is not None else 0)
        loss.backward()
        fw = dict(gi=a, gh=b, r=rr, z=zz, n=nn_, h_new=h_new, y=y, out=o, drop=od, xc=xt)
        if node is not None:
            wn_, wa_ = node_matrices(node[0], node[1], C, node[2], dt)
            fw["xw"], fw["a_ij"] = od @ wn_, od @ wa_
        fw = {k: v.detach() for k, v in fw.items()}
        bw = dict(d_x=L["x"].grad, d_h=L["h"].grad, d_id=L["id"].grad if "id" in L else None, d_gi=a.grad, d_gh=b.grad)
        return fw, bw

    (f32, b32), (f64, b64) = run(F32), run(F64)
    par = lambda got, key, r64=f64, r32=f32: assert_fp32_parity(got, r64[key], r32[key], f"{what} {key}")
    _, bound = par(hn, "h_new")
    assert_side(out, f64["y"].numpy(), bound + EPS32 * float(f64["y"].abs().max()), what)
    par(out, "out")
    if p > 0:
        par(drop, "drop")
    if xc is not None:
        par(xc, "xc")
    if gates:
        for j, key in enumerate(("r", "z", "n")):
            par(gi[:, j * C:(j + 1) * C], key)
        assert_fp32_parity(gi[:, M:], f64["gh"][:, 2 * C:], f32["gh"][:, 2 * C:], f"{what} gh_n")
    else:
        par(gi, "gi")
        par(gh, "gh")
    if node is not None:
        no_nan(node[3], node[4])
        par(node[3], "xw")
        par(node[4], "a_ij")
    # ---- backward ----
    did = nan(device, N, C) if (cfg["ident"]) else None
    bpar = lambda got, key: assert_fp32_parity(got, b64[key], b32[key], f"{what} {key}")
    if form == "fused":
        dgi, dgh, dh = nan(device, N, M), nan(device, N, M), nan(device, N, C)
        rc = lib.glam_gru_tail_rng_bwd(P(gi), P(gh), P(hd), P(out), P(god), P(gdd), P(gsd), N, C, 4, 0.0, LO, HI, p, P(eff), P(dgi), P(dgh), P(dh),
                                       P(did), S())
        assert rc == 0, lib.glam_last_error()
        no_nan(dgi, dgh, dh, did)
        bpar(dgi, "d_gi"), bpar(dgh, "d_gh"), bpar(did, "d_id")
        return
    dgi = nan(device, N, 4 * C if gates else M)
    dgh = None if gates else nan(device, N, M)
    dx, dh = nan(device, N, C), nan(device, N, C)
    xin, flag = (xc, 2) if xc is not None else (xd, 1 if celu else 0)
    lead = (P(gi), P(gh), P(hd), P(out), P(god), P(gdd), P(gsd), P(xin))
    tail = (N, C, flag, 4, 0.0, LO, HI, p, P(eff), int(merge), P(dgi), P(dgh), P(did), P(dx), P(dh), S())
    if form in ("ws", "xc"):
        rc = lib.glam_gru_bwd_ws_rng(*lead, P(ta), P(tb), *tail)
    else:
        rc = lib.glam_gru_bwd_ws_rng_pre(*lead, P(pre[1]), *tail)
    assert rc == 0, lib.glam_last_error()
    no_nan(dgi, dgh, dx, dh, did)
    bpar(dx, "d_x"), bpar(dh, "d_h")
    if did is not None:
        bpar(did, "d_id")
    if gates:      # D = [d_pr | d_pz | d_pn | d_pn r]: d_gi = D[:, :3C], d_gh = [D[:, :2C] | D[:, 3C:]]
        bpar(dgi[:, :M], "d_gi")
        bpar(torch.cat([dgi[:, :2 * C], dgi[:, M:]], 1), "d_gh")
    else:
        bpar(dgi, "d_gi"), bpar(dgh, "d_gh")


# ---------------------------------------------------------------------------------------------
# (h) through the Python surface: ops.manual_seed, the offset read from ops.rng_state before every call
# ---------------------------------------------------------------------------------------------
SURFACE_SEEDS = [1234, 0x1E3779B9F4A7C159]          # (ops.manual_seed keeps 63 bits)


def _offset(device):
    return int(ops.rng_state(device)[1].item())


@pytest.mark.parametrize("seed", SURFACE_SEEDS, ids=STREAM_IDS)
def test_python_surface_ops(device, seed):
    """``ops.rrelu`` (with its dropped twin), ``ops.dropout``, ``ops.linear_rrelu`` and ``ops.rrelu_dropout_linear_narrow`` after
    ``ops.manual_seed``: each advances the stream by exactly one, and outputs and gradients under random cotangents equal the fp64
    reference under the twin's noise at the offset read before the call."""
    p = 0.2
    g = torch.Generator().manual_seed(31)
    r = lambda *s: torch.randn(*s, generator=g)
    ops.manual_seed(seed, device)
    assert _offset(device) == 0 and int(ops.rng_state(device)[0].item()) == seed

    def case(what, leaves, dev_fn, twin_fn, noise_shape):
        """``dev_fn(*device leaves) -> [outputs]``; ``twin_fn(slopes, keep, dt, *cpu leaves) -> [outputs]``."""
        o0 = _offset(device)
        dl = [t.to(device).requires_grad_(True) for t in leaves]
        with ops.weight_scope():
            outs = dev_fn(*dl)
            assert _offset(device) == o0 + 1, f"{what}: the stream advanced by {_offset(device) - o0}"
            cots = [r(*o.shape) for o in outs]
            grads = torch.autograd.grad(sum((o * c.to(device)).sum() for o, c in zip(outs, cots)), dl)
        sl, keep, _ = noise((seed, o0), 0, noise_shape, p)

        def run(dt):
            ll = [leaf(t, dt) for t in leaves]
            oo = twin_fn(sl, keep, dt, *ll)
            gg = torch.autograd.grad(sum((o * c.to(dt)).sum() for o, c in zip(oo, cots)), ll)
            return torch.cat([o.detach() for o in oo], 1), list(gg)
        assert_twin_parity(run, torch.cat(list(outs), 1), list(grads), what)

    x = r(50, 60)

    def dev_rrelu(xd):
        out = ops.rrelu(xd, drop_p=p)
        twin = ops.take_dropped(out, p)
        assert twin is not None
        return [out, twin]
    case("ops.rrelu", [x], dev_rrelu, lambda sl, keep, dt, xl: list(tail_twin(xl, x > 0, sl, keep, p, dt)), (50, 60))
    one = np.ones((50, 60), dtype=np.float32)
    case("ops.dropout", [x], lambda xd: [ops.dropout(xd, p)], lambda sl, keep, dt, xl: [tail_twin(xl, x > 0, one, keep, p, dt)[1]], (50, 60))

    xe, we, be = r(1000, 16), r(60, 16) * 0.5, r(60)
    side = {}

    def dev_linear_rrelu(xd, wd, bd):
        y = ops.linear_rrelu(xd, wd, bd, LO, HI, drop_p=p)
        assert y is not None
        twin = ops.take_dropped(y, p)
        side["emb"] = (y > 0).cpu()
        return [y, twin]
    if _lib.route_enabled("x3"):
        case("ops.linear_rrelu", [xe, we, be], dev_linear_rrelu,
             lambda sl, keep, dt, xl, wl, bl: list(tail_twin(xl @ wl.t() + bl, side["emb"], sl, keep, p, dt)), (1000, 60))
    else:
        assert ops.linear_rrelu(xe.to(device), we.to(device), be.to(device), LO, HI, drop_p=p) is None

    xh, wh, bh = r(333, 128), r(2, 128) * 0.1, r(2)

    def dev_head(xd, wd, bd):
        y = ops.rrelu_dropout_linear_narrow(xd, wd, bd, LO, HI, p)
        assert y is not None
        return [y]
    case("ops.rrelu_dropout_linear_narrow", [xh, wh, bh], dev_head,
         lambda sl, keep, dt, xl, wl, bl: [tail_twin(xl, xh > 0, sl, keep, p, dt)[1] @ wl.t() + bl], (333, 128))


@pytest.mark.parametrize("seed", SURFACE_SEEDS, ids=STREAM_IDS)
def test_python_surface_message_block(device, seed):
    """One training-mode MessageBlock (src_1gp/layer.py:240-266; RReLU, Dropout(0.2), TripletMessage, GRU, skip connection) applied twice
    with shared weights (model.py:53-54) on the output of an RReLU that wrote its dropped twin, as the model's input embedding does: the
    two applications are exactly two RNG launches (each tail draws its slopes AND the next application's Dropout mask).  Reference:
    ``oracle.triplet_message`` + ``oracle.gru_step`` in fp64 / fp32 under the twin's noise at ``offset`` and ``offset + 1``; outputs, the
    gradient of the input and of every parameter under random cotangents."""
    p = 0.2
    b = synth_batch(24, seed=5)
    torch.manual_seed(3)
    blk = layer.MessageBlock(60, 60, 4, norm="_None", dropout="Dropout(0.2)", conv="_TripletMessage", act="RReLU", res=True).to(device).train()
    assert float(np.float32(blk.act.lower)) == float(np.float32(LO)) and float(np.float32(blk.act.upper)) == float(np.float32(HI))
    names = [n for n, _ in blk.named_parameters()]
    N = b.x.size(0)
    g = torch.Generator().manual_seed(N)
    pre = torch.randn(N, 60, generator=g)
    c1, c2, c3 = (torch.randn(N, 60, generator=g) for _ in range(3))
    bd = synth_batch(24, seed=5).to(device)
    ops.manual_seed(seed, device)
    pre_d = pre.to(device).requires_grad_(True)
    with ops.weight_scope():
        o_in = _offset(device)
        x0 = ops.rrelu(pre_d, drop_p=p)
        o = _offset(device)
        assert o == o_in + 1
        y1, h1 = blk(x0, bd.edge_index, bd.edge_attr, h=None, batch=bd.batch)
        y2, h2 = blk(y1, bd.edge_index, bd.edge_attr, h=h1, batch=bd.batch)
        assert _offset(device) == o + 2, f"two applications made {_offset(device) - o} RNG launches"
        loss = (y1 * c1.to(device)).sum() + (y2 * c2.to(device)).sum() + (h2.squeeze(0) * c3.to(device)).sum()
        grads = torch.autograd.grad(loss, [pre_d] + list(blk.parameters()))
    no_nan(y1, y2, h2)
    nz = [noise((seed, o_in + k), 0, (N, 60), p) for k in range(3)]
    sides = [pre > 0, (y1 > 0).cpu(), (y2 > 0).cpu()]
    prm = {n: q.detach().cpu() for n, q in blk.named_parameters()}
    ei = b.edge_index
    stash = {}

    def run(dt):
        q = {n: leaf(t, dt) for n, t in prm.items()}
        pl = leaf(pre, dt)
        ea = b.edge_attr.to(dt)

        def app(x_drop, identity, hh, k):
            c = O.triplet_message(x_drop, ei, ea, q["conv.conv.weight_node"], q["conv.conv.weight_edge"], q["conv.conv.weight_triplet_att"],
                                  q["conv.conv.weight_scale"], q["conv.conv.bias"])
            hn = O.gru_step(torch.nn.functional.celu(c), hh, q["gru.weight_ih_l0"], q["gru.weight_hh_l0"], q["gru.bias_ih_l0"], q["gru.bias_hh_l0"])
            y = hn + identity
            stash[(dt, k)] = y.detach()
            out, drop = tail_twin(y, sides[k], nz[k][0], nz[k][1], p, dt)
            return out, drop, hn
        x0_, d0_ = tail_twin(pl, sides[0], nz[0][0], nz[0][1], p, dt)
        o1, d1, hn1 = app(d0_, x0_, x0_, 1)
        o2, _, hn2 = app(d1, o1, hn1, 2)
        ls = (o1 * c1.to(dt)).sum() + (o2 * c2.to(dt)).sum() + (hn2 * c3.to(dt)).sum()
        gg = torch.autograd.grad(ls, [pl] + [q[n] for n in names])
        return torch.cat([o1, o2, hn2], 1).detach(), list(gg)

    assert_twin_parity(run, torch.cat([y1, y2, h2.squeeze(0)], 1), list(grads), "MessageBlock x 2 (train)", names=["x"] + names)
    for k, y in ((1, y1), (2, y2)):
        y64 = stash[(F64, k)]
        assert_side(y, y64.numpy(), 1e-5 * max(1.0, float(y64.abs().max())), f"application {k}")
