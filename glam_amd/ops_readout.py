"""Readouts, segment reductions, graph norms, block tails and per-pair fusion pools (src_1gp/layer.py:161-220, 270-283;
src_1gp/model.py:41).

Part of ``glam_amd.ops`` (every public name here is re-exported there: ``from glam_amd import ops; ops.pool5(...)``).  Knobs, the weight
scope, the padded-column bookkeeping and the index staging live in ``glam_amd/ops.py`` and are read through ``_o`` at call time."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from . import ops as _o
from ._lib import GlamHipError, f32c, ptr, require_device, stream

# --------------------------------------------------------------------------------------
# readouts
# --------------------------------------------------------------------------------------
class _Pool5(torch.autograd.Function):
    """``x`` holds ``D`` channels in rows of ``x.size(1) >= D`` floats (zero padding behind them: the padded flow of odd widths)."""

    @staticmethod
    def forward(ctx, x, sp, k, D):
        require_device(x)
        x = f32c(x, "x")
        N, ld = x.shape
        if N != sp.N:
            raise GlamHipError(f"pool: x has {N} rows but batch has {sp.N}")
        out = torch.empty(sp.B, (2 + k) * D, dtype=torch.float32, device=x.device)
        topk = torch.empty(sp.B, k, dtype=torch.int32, device=x.device)
        _lib.api().glam_pool5_padded_fwd(ptr(x), ptr(sp.ptr), N, sp.B, ld, D, k, ptr(out), ptr(topk), stream())
        ctx.save_for_backward(topk)
        ctx.sp, ctx.dims = sp, (N, ld, D, k)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        (topk,) = ctx.saved_tensors
        N, ld, D, k = ctx.dims
        sp = ctx.sp
        d_out = f32c(d_out, "d_out")
        d_x = torch.empty(N, ld, dtype=torch.float32, device=d_out.device)
        _lib.api().glam_pool5_padded_bwd(ptr(d_out), ptr(sp.ptr), ptr(topk), N, sp.B, ld, D, k, ptr(d_x), stream())
        return d_x, None, None, None


def pool5(x, sp, k=3):
    """mean || add || sort-pool(k) readout, ``[B, (2+k)*D]``."""
    base = _o.padded_base(x) if x.dim() == 2 else None
    if base is not None and base.size(1) <= 128 and base.size(1) - x.size(1) < 4:
        return _Pool5.apply(base, sp, k, x.size(1))      # odd widths: straight from the zero-padded rows, no compaction copy
    return _Pool5.apply(x, sp, k, x.size(1))


_MODES = {"sum": 0, "add": 0, "mean": 1, "max": 2}


class _SegmentPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sp, mode):
        require_device(x)
        x = f32c(x, "x")
        N, D = x.shape
        if N != sp.N:
            raise GlamHipError(f"pool: x has {N} rows but batch has {sp.N}")
        out = torch.empty(sp.B, D, dtype=torch.float32, device=x.device)
        argmax = torch.empty(sp.B, D, dtype=torch.int32, device=x.device) if mode == 2 else None
        _lib.api().glam_segment_pool_fwd(ptr(x), ptr(sp.ptr), N, sp.B, D, mode, ptr(out), ptr(argmax), stream())
        ctx.sp, ctx.dims, ctx.argmax = sp, (N, D, mode), argmax
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        N, D, mode = ctx.dims
        sp = ctx.sp
        d_out = f32c(d_out, "d_out")
        d_x = torch.empty(N, D, dtype=torch.float32, device=d_out.device)
        _lib.api().glam_segment_pool_bwd(ptr(d_out), ptr(sp.ptr), ptr(ctx.argmax), N, sp.B, D, mode, ptr(d_x), stream())
        return d_x, None, None


def segment_pool(x, sp, reduce="sum"):
    """``scatter(x, batch, dim=0, reduce)`` over the sorted ``batch`` behind ``sp``."""
    squeeze = x.dim() == 1
    out = _SegmentPool.apply(x.unsqueeze(-1) if squeeze else x, sp, _MODES[reduce])
    return out.squeeze(-1) if squeeze else out


class _SegmentAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, v, sp):
        require_device(gate, v)
        gate, v = f32c(gate.reshape(-1), "gate"), f32c(v, "v")
        N, D = v.shape
        if gate.numel() != N or N != sp.N:
            raise GlamHipError("segment_attention: gate / v / batch disagree on the node count")
        out = torch.empty(sp.B, D, dtype=torch.float32, device=v.device)
        stats = torch.empty(sp.B, 2, dtype=torch.float32, device=v.device)
        _lib.api().glam_segment_attn_fwd(ptr(gate), ptr(v), ptr(sp.ptr), N, sp.B, D, ptr(out), ptr(stats), stream())
        ctx.save_for_backward(gate, v, out, stats)
        ctx.sp = sp
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        gate, v, out, stats = ctx.saved_tensors
        sp = ctx.sp
        N, D = v.shape
        d_out = f32c(d_out, "d_out")
        d_gate, d_v = torch.empty_like(gate), torch.empty_like(v)
        _lib.api().glam_segment_attn_bwd(ptr(gate), ptr(v), ptr(out), ptr(stats), ptr(d_out), ptr(sp.ptr), N,
                                         sp.B, D, ptr(d_gate), ptr(d_v), stream())
        return d_gate, d_v, None


class _BiasResAct(torch.autograd.Function):
    """``act(y + bias + identity)``: the tail of a MessageBlock whose conv has no GRU (GCN / GAT), one launch per direction.
    ``rng = (rr_lower, rr_upper, drop_p)``: training-mode RReLU (``act == 4``) and / or a second output ``Dropout(drop_p)(out)``
    from the device-side Philox stream; ``want_out=False`` with ``act == 0`` is a plain Dropout.  Returns ``(out, out_drop)``."""

    @staticmethod
    def forward(ctx, y, bias, identity, act, slope, rng=None, want_out=True):
        ctx.set_materialize_grads(False)
        require_device(y, bias, identity)
        y = f32c(y, "y")
        bias = None if bias is None else f32c(bias, "bias")
        identity = None if identity is None else f32c(identity, "identity")
        N, C = y.shape
        out = torch.empty_like(y) if want_out else None
        out_drop, eff = None, None
        if rng is None:
            if act == _o.ACT_CODES["rrelu"] or not want_out:
                raise GlamHipError("bias_res_act: 'rrelu' / dropout-only need rng=(lower, upper, drop_p)")
            _lib.api().glam_bias_res_act_fwd(ptr(y), ptr(bias), ptr(identity), N, C, act, float(slope), ptr(out), stream())
        else:
            lo, hi, p = (float(v) for v in rng)
            eff = torch.empty(2, dtype=torch.int64, device=y.device)
            out_drop = torch.empty_like(y) if p > 0 else None
            _lib.api().glam_bias_res_act_rng_fwd(ptr(y), ptr(bias), ptr(identity), N, C, act, float(slope), lo, hi, p,
                                                 ptr(_o.rng_state(y.device)), ptr(eff), ptr(out), ptr(out_drop), stream())
        ctx.save_for_backward(*([out] if out is not None else []))
        ctx.eff = eff
        ctx.shape = (N, C)
        ctx.cfg = (act, float(slope), bias is not None, identity is not None, None if rng is None else tuple(float(v) for v in rng))
        return out, out_drop

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_out_drop=None):
        out = ctx.saved_tensors[0] if ctx.saved_tensors else None
        act, slope, has_bias, has_id, rng = ctx.cfg
        N, C = ctx.shape
        d_out = None if d_out is None else f32c(d_out, "d_out")
        d_out_drop = None if d_out_drop is None else f32c(d_out_drop, "d_out_drop")
        ref = d_out if d_out is not None else d_out_drop
        d_y = torch.empty_like(ref)
        if rng is None:
            _lib.api().glam_bias_res_act_bwd(ptr(out), ptr(d_out), N, C, act, slope, ptr(d_y), stream())
        else:
            _lib.api().glam_bias_res_act_rng_bwd(ptr(out), ptr(d_out), ptr(d_out_drop), N, C, act, slope, rng[0], rng[1], rng[2],
                                                 ptr(ctx.eff), ptr(d_y), stream())
        return d_y, (d_y.sum(0) if has_bias else None), (d_y if has_id else None), None, None, None, None


def bias_res_act(y, bias, identity, act="none", slope=0.0, rng=None):
    out, out_drop = _BiasResAct.apply(y, bias, identity, _o.ACT_CODES[act], slope, rng, True)
    if out_drop is not None:
        _o.register_dropped(out, out_drop, rng[2])
    return out


def rrelu(x, lower=1.0 / 8, upper=1.0 / 3, drop_p=0.0):
    """Training-mode ``torch.nn.RReLU(lower, upper)`` on the device-side Philox stream (one launch per direction, slopes
    regenerated in the backward); ``drop_p > 0`` also writes the dropped twin for a ``Dropout(drop_p)`` that follows."""
    shape = x.shape
    out, out_drop = _BiasResAct.apply(x.reshape(-1, shape[-1]), None, None, _o.ACT_CODES["rrelu"], 0.0, (lower, upper, drop_p), True)
    out = out.view(shape)
    if out_drop is not None:
        _o.register_dropped(out, out_drop.view(shape), drop_p)
    return out


def dropout(x, p):
    """Training-mode ``torch.nn.Dropout(p)``: ``x * mask / (1 - p)``; the mask is regenerated in the backward (no mask tensor)."""
    shape = x.shape
    _, out_drop = _BiasResAct.apply(x.reshape(-1, shape[-1]), None, None, _o.ACT_CODES["none"], 0.0, (1.0, 1.0, float(p)), False)
    return out_drop.view(shape)


class _LstmCell(torch.autograd.Function):
    """Gate math of one ``torch.nn.LSTM`` cell step (Set2Set): ``(gates[B,4C], c[B,C]) -> (h', c')``, one launch each way."""

    @staticmethod
    def forward(ctx, gates, c_prev):
        require_device(gates, c_prev)
        gates, c_prev = f32c(gates, "gates"), f32c(c_prev, "c")
        B, C = c_prev.shape
        h_new, c_new = torch.empty_like(c_prev), torch.empty_like(c_prev)
        _lib.api().glam_lstm_cell_fwd(ptr(gates), ptr(c_prev), B, C, ptr(h_new), ptr(c_new), stream())
        ctx.save_for_backward(gates, c_prev)
        return h_new, c_new

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_h, d_c):
        gates, c_prev = ctx.saved_tensors
        B, C = c_prev.shape
        d_h = None if d_h is None else f32c(d_h, "d_h")
        d_c = None if d_c is None else f32c(d_c, "d_c")
        d_gates, d_cp = torch.empty_like(gates), torch.empty_like(c_prev)
        _lib.api().glam_lstm_cell_bwd(ptr(gates), ptr(c_prev), ptr(d_h), ptr(d_c), B, C, ptr(d_gates), ptr(d_cp), stream())
        return d_gates, d_cp


def lstm_cell(gates, c_prev):
    return _LstmCell.apply(gates, c_prev)


class _QueryAttention(torch.autograd.Function):
    """Set2Set's attention read ``r_g = sum_n softmax_n(<x_n, q_g>) x_n`` with the logits formed inside the kernel."""

    @staticmethod
    def forward(ctx, x, q, sp):
        require_device(x, q)
        x, q = f32c(x, "x"), f32c(q, "q")
        N, D = x.shape
        if N != sp.N or q.shape != (sp.B, D):
            raise GlamHipError("query_attention: x / q disagree with the batch vector")
        r = torch.empty(sp.B, D, dtype=torch.float32, device=x.device)
        stats = torch.empty(sp.B, 2, dtype=torch.float32, device=x.device)
        _lib.api().glam_s2s_attn_fwd(ptr(x), ptr(q), ptr(sp.ptr), N, sp.B, D, ptr(r), ptr(stats), stream())
        ctx.save_for_backward(x, q, r, stats)
        ctx.sp = sp
        return r

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_r):
        x, q, r, stats = ctx.saved_tensors
        sp = ctx.sp
        d_r = f32c(d_r, "d_r")
        d_x, d_q = torch.empty_like(x), torch.empty_like(q)
        _lib.api().glam_s2s_attn_bwd(ptr(x), ptr(q), ptr(r), ptr(stats), ptr(d_r), ptr(sp.ptr), x.size(0), sp.B, x.size(1),
                                     ptr(d_x), ptr(d_q), stream())
        return d_x, d_q, None


def query_attention_supported(D):
    return D % 4 == 0 and D <= 128


def query_attention(x, q, sp):
    return _QueryAttention.apply(x, q, sp)


def segment_attention(gate, v, sp):
    """``scatter_add(softmax(gate, batch) * v, batch)`` -> ``[B, D]`` (GlobalAttention / Set2Set)."""
    return _SegmentAttn.apply(gate, v, sp)


class _EdgeReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, gi, mode):
        require_device(msg)
        msg = f32c(msg, "msg")
        E, D = msg.shape
        if E != gi.E:
            raise GlamHipError(f"edge_reduce: {E} messages for {gi.E} edges")
        out = torch.empty(gi.N, D, dtype=torch.float32, device=msg.device)
        argmax = torch.empty(gi.N, D, dtype=torch.int32, device=msg.device) if mode == 2 else None
        _lib.api().glam_edge_reduce_fwd(ptr(msg), ptr(gi.rowptr), ptr(gi.eid), gi.N, E, D, mode, ptr(out), ptr(argmax), stream())
        ctx.gi, ctx.dims, ctx.argmax = gi, (E, D, mode), argmax
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        E, D, mode = ctx.dims
        gi = ctx.gi
        d_out = f32c(d_out, "d_out")
        d_msg = torch.empty(E, D, dtype=torch.float32, device=d_out.device)
        _lib.api().glam_edge_reduce_bwd(ptr(d_out), ptr(gi.rowptr), ptr(gi.eid), ptr(ctx.argmax), gi.N, E, D, mode, ptr(d_msg), stream())
        return d_msg, None, None


def edge_reduce(msg, gi, reduce="sum"):
    """``scatter(msg, edge_index[1], dim=0, dim_size=N, reduce)`` over the CSR-by-target in ``gi``."""
    squeeze = msg.dim() == 1
    out = _EdgeReduce.apply(msg.unsqueeze(-1) if squeeze else msg, gi, _MODES[reduce])
    return out.squeeze(-1) if squeeze else out


class _GraphNorm(torch.autograd.Function):
    """``with_identity``: the op also returns ``x`` itself as a second output — the skip connection of a MessageBlock
    (src_1gp/layer.py:253-265: ``x`` feeds the norm AND ``x + identity``).  Both gradient paths then arrive at THIS node and the
    backward kernel sums them in its store (glam_graph_norm_bwd_add) instead of autograd launching an add."""

    @staticmethod
    def forward(ctx, x, sp, mode, scale, eps, with_identity=False, drop_p=0.0):
        require_device(x)
        x = f32c(x, "x")
        N, D = x.shape
        if N != sp.N:
            raise GlamHipError(f"graph_norm: x has {N} rows but batch has {sp.N}")
        ctx.drop_p, ctx.eff = float(drop_p), None
        if drop_p > 0:
            # the training-mode Dropout(drop_p) behind the norm from the same launch: the output IS the dropped tensor (graph_norm_drop_supported)
            y = torch.empty_like(x)
            ctx.eff = torch.empty(2, dtype=torch.int64, device=x.device)
            _lib.api().glam_graph_norm_drop_fwd(ptr(x), ptr(sp.ptr), N, sp.B, D, mode, float(scale), float(eps), float(drop_p),
                                                ptr(_o.rng_state(x.device)), ptr(ctx.eff), None, ptr(y), stream())
        else:
            y = torch.zeros_like(x) if sp.B == 0 else torch.empty_like(x)
            _lib.api().glam_graph_norm_fwd(ptr(x), ptr(sp.ptr), N, sp.B, D, mode, float(scale), float(eps), ptr(y), stream())
        ctx.save_for_backward(x)
        ctx.sp, ctx.cfg = sp, (mode, float(scale), float(eps))
        if with_identity:
            ctx.set_materialize_grads(False)
            return y, x.view_as(x)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, d_id=None):
        (x,) = ctx.saved_tensors
        mode, scale, eps = ctx.cfg
        sp = ctx.sp
        N, D = x.shape
        if gy is None:                  # only the identity output was used
            return d_id, None, None, None, None, None, None
        gy = f32c(gy, "gy")
        dx = torch.empty_like(x)
        lib = _lib.api()
        if ctx.drop_p > 0:              # gy is the gradient of the DROPPED output: the mask is regenerated inside the launch
            lib.glam_graph_norm_drop_bwd(ptr(x), None, ptr(gy), ptr(sp.ptr), N, sp.B, D, mode, scale, eps, ctx.drop_p, ptr(ctx.eff),
                                         ptr(None if d_id is None else f32c(d_id, "d_identity")), ptr(dx), stream())
            return dx, None, None, None, None, None, None
        if d_id is not None and N > 0 and sp.B > 0:
            lib.glam_graph_norm_bwd_add(ptr(x), ptr(gy), ptr(sp.ptr), N, sp.B, D, mode, scale, eps, ptr(f32c(d_id, "d_identity")), ptr(dx), stream())
            return dx, None, None, None, None, None, None
        lib.glam_graph_norm_bwd(ptr(x), ptr(gy), ptr(sp.ptr), N, sp.B, D, mode, scale, eps, ptr(dx), stream())
        if d_id is not None:
            dx = d_id if (N == 0 or sp.B == 0) else dx + d_id
        return dx, None, None, None, None, None, None


def graph_norm_drop_supported(x, sp):
    """The norm + Dropout launch pair exists for this shape (molecule-sized graphs, a multiple of 4 channels <= 64)."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and sp.B > 0
            and _lib.api().glam_graph_norm_drop_supported(x.size(0), sp.B, x.size(1)) == 1)


def pair_norm(x, sp, scale=1.0, eps=1e-5, with_identity=False, drop_p=0.0):
    """PyG ``PairNorm(scale, eps=1e-5)(x, batch)`` (one kernel per direction); ``with_identity``: ``(y, x)`` — see _GraphNorm;
    ``drop_p > 0`` (``graph_norm_drop_supported``): the result is ``Dropout(drop_p)(PairNorm(x))`` in training mode, from the one launch."""
    return _GraphNorm.apply(x, sp, 0, scale, eps, with_identity, drop_p)


def graph_standardize(x, sp, eps=1e-5, with_identity=False):
    """Statistics part of PyG's graph ``LayerNorm(x, batch)``: zero mean / unit variance per graph."""
    return _GraphNorm.apply(x, sp, 1, 1.0, eps, with_identity, 0.0)


class _EdgeWeightedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, gi, mean, self_slot, with_identity=False):
        require_device(x, w)
        x_in = x
        x, w = f32c(x, "x"), f32c(w, "w")
        N, D = x.shape
        E, K = w.shape
        if N != gi.N or E != gi.E:
            raise GlamHipError("edge_weighted_sum: x / w disagree with the edge list")
        out = torch.empty(N, K + int(self_slot), D, dtype=torch.float32, device=x.device)
        _lib.api().glam_edge_wsum_fwd(ptr(x), ptr(w), ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid), N, E, D, K, int(mean),
                                      int(self_slot), ptr(out), stream())
        ctx.save_for_backward(w)
        ctx.gi, ctx.cfg = gi, (N, E, D, K, int(mean), int(self_slot))
        ctx.aliased = bool(with_identity)
        if ctx.aliased:
            ctx.set_materialize_grads(False)
            return out, x_in.view_as(x_in)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_alias=None):
        (w,) = ctx.saved_tensors
        gi = ctx.gi
        N, E, D, K, mean, self_slot = ctx.cfg
        if d_out is None:                    # (only with the alias: the sums themselves were not used)
            return d_alias, None, None, None, None, None
        d_out = f32c(d_out, "d_out")
        colptr, dst, eid_t = gi.transpose()
        dx = torch.empty(N, D, dtype=torch.float32, device=d_out.device)
        lib = _lib.api()
        d_alias = None if d_alias is None else f32c(d_alias, "d_identity")
        if d_alias is not None and K in (4, 8) and D % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (d_out, w, d_alias)):
            # the skip connection's gradient joins the sums in this launch (no add launch of the autograd engine); the launch
            # exists for 16-byte aligned operands only (glam_edge_wsum_bwd_add refuses the rest)
            lib.glam_edge_wsum_bwd_add(ptr(d_out), ptr(w), ptr(colptr), ptr(dst), ptr(eid_t), ptr(gi.rowptr), N, E, D, K, mean, self_slot,
                                       ptr(d_alias), ptr(dx), stream())
            return dx, None, None, None, None, None
        lib.glam_edge_wsum_bwd(ptr(d_out), ptr(w), ptr(colptr), ptr(dst), ptr(eid_t), ptr(gi.rowptr), N, E, D, K, mean, self_slot, ptr(dx), stream())
        return (dx if d_alias is None else dx + d_alias), None, None, None, None, None


def edge_weighted_sum(x, w, gi, mean=False, self_slot=False, with_identity=False):
    """``S[n,k,:] = (1/deg_n) sum_{e->n} w[e,k] * x[src_e,:]`` -> ``[N, K, D]`` (no gradient w.r.t. ``w``: edge data);
    ``self_slot``: ``[N, K+1, D]`` with ``S[n,K,:] = x[n,:]`` (K in {4, 8}, D % 4 == 0).  ``with_identity``: returns ``(S, identity)`` with
    ``identity`` = ``x`` handed back through this node (a skip connection around the caller then sends its gradient here: it is added
    inside the backward launch)."""
    if with_identity:
        if torch.is_grad_enabled() and x.requires_grad:
            return _EdgeWeightedSum.apply(x, w, gi, mean, self_slot, True)
        return _EdgeWeightedSum.apply(x, w, gi, mean, self_slot), x
    return _EdgeWeightedSum.apply(x, w, gi, mean, self_slot)


def self_slot_supported(K, D):
    return K in (4, 8) and D % 4 == 0


# --------------------------------------------------------------------------------------
# NNConv over continuous edge features (csrc/nnconv_ec.hip): no per-edge weight tensor
# --------------------------------------------------------------------------------------
class _NNConvECStack(torch.autograd.Function):
    """``Wstack`` f32[34 Cin, Cout] = [A_0; ...; A_31; b1; root] from ``nn.2.weight``, ``nn.2.bias`` and ``root`` (one launch each way)."""

    @staticmethod
    def forward(ctx, w1, b1, root):
        require_device(w1, b1, root)
        w1, b1, root = f32c(w1, "nn.2.weight"), f32c(b1, "nn.2.bias"), f32c(root, "root")
        Cin, Cout = root.shape
        out = torch.empty(34 * Cin, Cout, dtype=torch.float32, device=w1.device)
        _lib.api().glam_nnconv_ec_stack(ptr(w1), ptr(b1), ptr(root), Cin, Cout, ptr(out), stream())
        ctx.dims = (Cin, Cout)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_ws):
        Cin, Cout = ctx.dims
        d_ws = f32c(d_ws, "d_wstack")
        dw1 = torch.empty(Cin * Cout, 32, dtype=torch.float32, device=d_ws.device)
        db1 = torch.empty(Cin * Cout, dtype=torch.float32, device=d_ws.device)
        droot = torch.empty(Cin, Cout, dtype=torch.float32, device=d_ws.device)
        _lib.api().glam_nnconv_ec_unstack(ptr(d_ws), Cin, Cout, ptr(dw1), ptr(db1), ptr(droot), stream())
        return dw1, db1, droot


def nnconv_ec_stack(w1, b1, root):
    """The stacked weight of ``nnconv_edge_conditioned`` (build it once per model forward: ``ops.scoped_weights``)."""
    return _NNConvECStack.apply(w1, b1, root)


class _NNConvEC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, edge_attr, gi, w0, b0, wstack, bias, mean, with_identity=False):
        require_device(x, edge_attr, w0, b0, wstack)
        x_in = x
        x, ea = f32c(x, "x"), f32c(edge_attr, "edge_attr")
        w0, b0, wstack = f32c(w0, "nn.0.weight"), f32c(b0, "nn.0.bias"), f32c(wstack, "wstack")
        bias = None if bias is None else f32c(bias, "bias")
        N, Cin = x.shape
        E, De = ea.shape
        Cout = wstack.size(1)
        if N != gi.N or E != gi.E or wstack.size(0) != 34 * Cin or tuple(w0.shape) != (32, De):
            raise GlamHipError("nnconv_edge_conditioned: x / edge_attr / weights disagree with the edge list")
        lib = _lib.api()
        h = torch.empty(E, 32, dtype=torch.float32, device=x.device)
        out = torch.empty(N, Cout, dtype=torch.float32, device=x.device)
        nws = lib.glam_nnconv_ec_workspace_bytes(N, E, De, Cin, Cout, 0)
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
        lib.glam_nnconv_ec_fwd(ptr(x), ptr(ea), ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid), N, E, De, Cin, Cout, ptr(w0), ptr(b0),
                               ptr(wstack), ptr(bias), int(mean), ptr(h), ptr(ws), ws.numel(), ptr(out), stream())
        del ws
        ctx.save_for_backward(x, ea, wstack, h)
        ctx.gi, ctx.dims, ctx.has_bias = gi, (N, E, De, Cin, Cout, int(mean)), bias is not None
        ctx.aliased = bool(with_identity)
        if ctx.aliased:
            ctx.set_materialize_grads(False)
            return out, x_in.view_as(x_in)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_alias=None):
        x, ea, wstack, h = ctx.saved_tensors
        gi = ctx.gi
        N, E, De, Cin, Cout, mean = ctx.dims
        if d_out is None:                    # (only with the alias: the layer's output itself was not used)
            return d_alias, None, None, None, None, None, None, None, None
        d_out = f32c(d_out, "d_out")
        d_alias = None if d_alias is None else f32c(d_alias, "d_identity")
        colptr, dst, eid_t = gi.transpose()
        dev = d_out.device
        f32 = dict(dtype=torch.float32, device=dev)
        dx, dw0, db0 = torch.empty(N, Cin, **f32), torch.empty(32, De, **f32), torch.empty(32, **f32)
        dws, dbias = torch.empty(34 * Cin, Cout, **f32), torch.empty(Cout, **f32)
        lib = _lib.api()
        ws = torch.empty(max(lib.glam_nnconv_ec_workspace_bytes(N, E, De, Cin, Cout, 1), 16), dtype=torch.uint8, device=dev)
        lib.glam_nnconv_ec_bwd(ptr(d_out), ptr(x), ptr(ea), ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid), ptr(colptr), ptr(dst), ptr(eid_t),
                               N, E, De, Cin, Cout, ptr(wstack), ptr(h), mean, ptr(d_alias), ptr(dx), ptr(dw0), ptr(db0), ptr(dws),
                               ptr(dbias), ptr(ws), ws.numel(), stream())
        return dx, None, None, dw0, db0, dws, (dbias if ctx.has_bias else None), None, None


def nnconv_ec_supported(De, hidden, Cin, Cout):
    return _lib.api().glam_nnconv_ec_supported(De, hidden, Cin, Cout) == 1


def nnconv_edge_conditioned(x, edge_attr, gi, w0, b0, w1, b1, root, bias, mean=True, with_identity=False, wstack=None):
    """PyG ``NNConv(Cin, Cout, Linear(De, 32) -> ReLU -> Linear(32, Cin*Cout), aggr='mean' | 'add')`` on continuous edge features
    without the per-edge weight tensor: ``out = [S | x] @ Wstack + bias`` (csrc/nnconv_ec.hip; the algebra is in its header).
    ``w0, b0, w1, b1``: ``nn.0.weight``, ``nn.0.bias``, ``nn.2.weight``, ``nn.2.bias``; ``bias`` may be None; ``wstack``: a prebuilt
    ``nnconv_ec_stack(w1, b1, root)`` (shared by the applications of one forward), else built here.  No gradient w.r.t.
    ``edge_attr`` (edge data).  ``with_identity``: returns ``(out, identity)`` as ``edge_weighted_sum`` does."""
    if wstack is None:
        wstack = nnconv_ec_stack(w1, b1, root)
    if with_identity:
        if torch.is_grad_enabled() and x.requires_grad:
            return _NNConvEC.apply(x, edge_attr, gi, w0, b0, wstack, bias, mean, True)
        return _NNConvEC.apply(x, edge_attr, gi, w0, b0, wstack, bias, mean), x
    return _NNConvEC.apply(x, edge_attr, gi, w0, b0, wstack, bias, mean)


class _PairPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mol, pro, msp, psp, with_identity=False):
        require_device(mol, pro)
        mol_in, pro_in = mol, pro
        mol, pro = f32c(mol, "mol_out"), f32c(pro, "pro_out")
        if msp.B != psp.B or mol.size(1) != pro.size(1) or mol.size(0) != msp.N or pro.size(0) != psp.N:
            raise GlamHipError("pair_pool: the two batches disagree (pair count / width / node count)")
        P, D = msp.B, mol.size(1)
        out = torch.empty(P, 2, dtype=torch.float32, device=mol.device)
        arg = torch.empty(P, 2, dtype=torch.int32, device=mol.device)
        sums = torch.empty(P, 2, D, dtype=torch.float32, device=mol.device)
        lib = _lib.api()
        ws = torch.empty(max(lib.glam_pair_pool_workspace_bytes(P, D), 16), dtype=torch.uint8, device=mol.device)
        lib.glam_pair_pool_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), P, D, ptr(out), ptr(arg), ptr(sums), ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(mol, pro, arg, sums)
        ctx.sps = (msp, psp)
        ctx.aliased = bool(with_identity)
        if ctx.aliased:      # the two inputs come back as outputs: what the caller does with them next sends its gradient HERE
            ctx.set_materialize_grads(False)
            return out, mol_in.view_as(mol_in), pro_in.view_as(pro_in)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_ma=None, d_pa=None):
        mol, pro, arg, sums = ctx.saved_tensors
        msp, psp = ctx.sps
        if d_out is None:                    # (only with the aliases: the fusion values themselves were not used)
            return d_ma, d_pa, None, None, None
        d_out = f32c(d_out, "d_out")
        d_mol, d_pro = torch.empty_like(mol), torch.empty_like(pro)
        lib = _lib.api()
        if d_ma is not None or d_pa is not None:
            d_ma = None if d_ma is None else f32c(d_ma, "d_mol (next use)")
            d_pa = None if d_pa is None else f32c(d_pa, "d_pro (next use)")
            lib.glam_pair_pool_bwd_add(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(arg), ptr(sums), ptr(d_out), msp.B, mol.size(1),
                                       ptr(d_ma), ptr(d_pa), ptr(d_mol), ptr(d_pro), stream())
        else:
            lib.glam_pair_pool_bwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(arg), ptr(sums), ptr(d_out), msp.B,
                                   mol.size(1), ptr(d_mol), ptr(d_pro), stream())
        return d_mol, d_pro, None, None, None


def pair_pool(mol_out, pro_out, msp, psp, with_identity=False):
    """``[max, mean]`` of ``mol[seg_i] @ pro[seg_i].T`` per pair -> ``[P, 2]`` (dot_and_global_pool2).  ``with_identity``: returns
    ``(out, mol_out, pro_out)`` with the two matrices handed back through this node where that saves the add launches of their second
    use (the next message step): its gradient is then added inside this node's backward launch."""
    if with_identity:
        D = mol_out.size(1)
        if (torch.is_grad_enabled() and mol_out.requires_grad and pro_out.requires_grad and mol_out.is_cuda
                and mol_out.dtype == torch.float32 and pro_out.dtype == torch.float32 and mol_out.size(1) == pro_out.size(1)
                and _lib.api().glam_pair_pool_add_supported(D) == 1):
            return _PairPool.apply(mol_out, pro_out, msp, psp, True)
        return _PairPool.apply(mol_out, pro_out, msp, psp), mol_out, pro_out
    return _PairPool.apply(mol_out, pro_out, msp, psp)


class _PairPool5(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mol, pro, msp, psp):
        require_device(mol, pro)
        mol, pro = f32c(mol, "mol_out"), f32c(pro, "pro_out")
        if msp.B != psp.B or mol.size(1) != pro.size(1) or mol.size(0) != msp.N or pro.size(0) != psp.N:
            raise GlamHipError("pair_pool5: the two batches disagree (pair count / width / node count)")
        P, D = msp.B, mol.size(1)
        out = torch.empty(P, 5, dtype=torch.float32, device=mol.device)
        arg = torch.empty(P, 6, dtype=torch.int32, device=mol.device)
        _lib.api().glam_pair_pool5_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), P, D, ptr(out), ptr(arg), stream())
        ctx.save_for_backward(mol, pro, out, arg)
        ctx.sps = (msp, psp)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        mol, pro, out, arg = ctx.saved_tensors
        msp, psp = ctx.sps
        d_out = f32c(d_out, "d_out")
        d_mol, d_pro = torch.empty_like(mol), torch.empty_like(pro)
        _lib.api().glam_pair_pool5_bwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(out), ptr(arg), ptr(d_out), msp.B,
                                       mol.size(1), ptr(d_mol), ptr(d_pro), stream())
        return d_mol, d_pro, None, None


def pair_pool5(mol_out, pro_out, msp, psp):
    """``[max, mean, median, min, std]`` of ``mol[seg_i] @ pro[seg_i].T`` per pair -> ``[P, 5]`` (dot_and_global_pool5);
    widths that are multiples of 4 up to 128 (``pad_cols`` the operands first: zero columns do not change a score)."""
    return _PairPool5.apply(mol_out, pro_out, msp, psp)


# --------------------------------------------------------------------------------------
# screening: the fusion against proteins that are held once (csrc/pairpool.hip, glam_pair_pool_indexed_fwd)
# --------------------------------------------------------------------------------------
class PairIndex:
    """A validated pair -> protein index: ``host`` int32 ``[P]`` (numpy) with every entry in ``[0, Q)``.  ``on(device)`` is its device
    copy, made once per device (out of pinned memory, only enqueued) and shared by every launch that reads it."""

    def __init__(self, host, Q):
        self.host, self.P, self.Q = host, int(host.shape[0]), int(Q)
        self._dev = {}
        self._by_protein = None

    def on(self, device):
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = _stage_int32(self.host, device, "the pair -> protein index")
        return t

    def by_protein(self):
        """The pairs grouped by protein, for the sums of the training call (``ops.pair_pool_shared`` / ``ops.pair_rows``): ``order`` int32
        ``[P]`` — the stable argsort of the index (the pairs of a protein keep their batch order) — and ``ptr`` int32 ``[Q + 1]``, the
        offsets of the proteins' runs in it.  Built once, on the host; ``.on(device)`` -> their device copies, made once per device."""
        if self._by_protein is None:
            self._by_protein = PairsByProtein(self.host, self.Q)
        return self._by_protein


def _stage_int32(host, device, what):
    """Device copy of a host int32 vector out of pinned memory (only enqueued).  Not inside a hipGraph capture: the copy would be baked
    into the graph and the pinned buffer allocated under it — the eager first visit of a batch makes the copies a capture then finds."""
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise GlamHipError(f"{what} has no copy on {device} yet and a hipGraph capture cannot make one: keep ONE PairIndex across the "
                           "steps (ops.pair_index) and run the first step on it eagerly, as GraphedTrainStep does")
    n = int(host.shape[0])
    staged = torch.empty(max(n, 1), dtype=torch.int32, pin_memory=True)
    staged.numpy()[:n] = host
    return staged.to(device, non_blocking=True)[:n]


class PairsByProtein:
    """``order`` / ``ptr`` of ``PairIndex.by_protein`` (host, int32 numpy) and their device copies."""

    def __init__(self, host, Q):
        P, Q = int(host.shape[0]), int(Q)
        if P and (int(host.min()) < 0 or int(host.max()) >= Q):
            raise IndexError(f"the pair -> protein index must lie in [0, {Q})")
        self.order = np.argsort(host, kind="stable").astype(np.int32)
        self.ptr = np.zeros(Q + 1, dtype=np.int32)
        np.cumsum(np.bincount(host, minlength=Q)[:Q], out=self.ptr[1:])
        if int(self.ptr[-1]) != P:
            raise IndexError("the pair -> protein index does not sort into its proteins' runs")
        self.P, self.Q = P, Q
        self._dev = {}

    def on(self, device):
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            both = _stage_int32(np.concatenate([self.order, self.ptr]), device, "the pair list by protein")      # (one copy)
            t = self._dev[device] = (both[:self.P], both[self.P:])
        return t


def pair_index(pro_of_pair, P, Q, default="identity", name="pro_of_pair", over="proteins"):
    """``PairIndex`` of ``pro_of_pair`` for ``P`` pairs over ``Q`` proteins — host only, before anything is launched (the kernel trusts
    the index; the policy of ``data.resident_table``).  A host sequence, numpy array or CPU tensor of integers of length ``P``;
    ``IndexError`` for a wrong length or an entry outside ``[0, Q)``; a device tensor is refused (validating it would be a hidden
    read-back).  ``None``: ``default="identity"`` pairs ligand i with protein i (needs ``Q == P``), ``default="single"`` pairs every
    ligand with the one protein (needs ``Q == 1``).  ``name`` / ``over``: what the messages call the index and the things it points
    into (``ops.pair_pool_gather`` validates ``idx1`` / ``idx2`` over drugs with the same rules)."""
    P, Q = int(P), int(Q)
    if isinstance(pro_of_pair, PairIndex):
        if pro_of_pair.P != P or pro_of_pair.Q != Q:
            raise IndexError(f"{name} was validated for {pro_of_pair.P} pairs over {pro_of_pair.Q} {over}, not {P} over {Q}")
        return pro_of_pair
    if pro_of_pair is None:
        if default == "identity":
            if Q != P:
                if name != "pro_of_pair":
                    raise IndexError(f"{name}=None takes segment i for pair i: {P} pairs but {Q} {over}")
                raise IndexError(f"pro_of_pair=None pairs ligand i with protein i: {P} ligands but {Q} proteins")
            return PairIndex(np.arange(P, dtype=np.int32), Q)
        if Q != 1:
            raise IndexError(f"pro_of_pair=None screens against the one encoded protein, but the encoding holds {Q}: pass the index")
        return PairIndex(np.zeros(P, dtype=np.int32), Q)
    if torch.is_tensor(pro_of_pair):
        if pro_of_pair.device.type != "cpu":
            raise GlamHipError(f"{name} lives on a device: it is validated on the host before the launch, which would be a hidden "
                               "read-back — pass the host sequence / numpy array / CPU tensor it was made from")
        pro_of_pair = pro_of_pair.detach().numpy()
    idx = np.asarray(pro_of_pair)
    if idx.size == 0:
        idx = np.zeros(0, dtype=np.int64)
    if idx.dtype.kind not in "iu":
        raise IndexError(f"{name} must hold integers, got {idx.dtype}")
    if idx.ndim != 1 or idx.shape[0] != P:
        raise IndexError(f"{name} must have one entry per pair: shape {tuple(idx.shape)} for {P} pairs")
    if P and (int(idx.min()) < 0 or int(idx.max()) >= Q):
        raise IndexError(f"{name} must lie in [0, {Q}): got {int(idx.min())} .. {int(idx.max())}")
    return PairIndex(idx.astype(np.int32), Q)


def pair_pool_indexed(mol_out, pro_out, msp, psp, pro_of_pair=None, return_argmax=False):
    """``[max, mean]`` of ``mol[seg_i] @ pro[seg_q].T`` with ``q = pro_of_pair[i]`` -> ``[P, 2]``: ``pair_pool`` against proteins that are
    held once (``psp.B`` segments) instead of once per pair.  The max column — and with ``return_argmax`` the ``[P, 2]`` int32 rows of
    the maximum in ``mol_out`` / ``pro_out`` (-1 for an empty pair) — is bit for bit that of ``pair_pool`` on replicated residue rows.
    ``pro_of_pair``: see ``pair_index`` (``None`` = identity).  Inference only: there is no backward (training is ``ops.pair_pool``)."""
    P, Q = msp.B, psp.B
    index = pair_index(pro_of_pair, P, Q)
    if torch.is_grad_enabled() and (mol_out.requires_grad or pro_out.requires_grad):
        raise GlamHipError("pair_pool_indexed is inference only (no backward): call it under torch.no_grad(); the training route is "
                           "ops.pair_pool on one protein graph per pair")
    require_device(mol_out, pro_out)
    mol, pro = f32c(mol_out, "mol_out"), f32c(pro_out, "pro_out")
    if mol.size(1) != pro.size(1) or mol.size(0) != msp.N or pro.size(0) != psp.N:
        raise GlamHipError("pair_pool_indexed: the two batches disagree (width / node count)")
    D = mol.size(1)
    out = torch.empty(P, 2, dtype=torch.float32, device=mol.device)
    arg = torch.empty(P, 2, dtype=torch.int32, device=mol.device) if return_argmax else None
    lib = _lib.api()
    ws = torch.empty(max(lib.glam_pair_pool_workspace_bytes(P, D), 16), dtype=torch.uint8, device=mol.device)
    lib.glam_pair_pool_indexed_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(index.on(mol.device)), P, Q, D, ptr(out), ptr(arg),
                                   ptr(ws), ws.numel(), stream())
    return (out, arg) if return_argmax else out


# --------------------------------------------------------------------------------------
# panel screening: every ligand against every selected protein, protein-stationary (csrc/pairpanel.hip, glam_pair_pool_panel_fwd)
# --------------------------------------------------------------------------------------
PANEL_CHUNK = 64      # residue rows per chunk (one per lane of the wave that holds them) = kPanelChunk of csrc/pairpanel.hip


class PanelPlan:
    """The work of one panel call over a validated selection: ``sel`` int32 ``[Qs]`` (every entry in ``[0, Q)``) and ``work`` int32
    ``[4 * total_chunks + Qs + 1]`` — per chunk of 64 residue rows, in selection order, ``(j, first row of the chunk in the encoding,
    rows in the chunk, index of its partials in the workspace)``, then ``chunk_ptr[Qs + 1]``, the offsets of the selections' chunk
    runs (``chunks`` / ``chunk_ptr`` are views of it).  Host numpy; ``on(device)`` -> ``(sel, work)`` on the device, made once per
    device (one copy out of pinned memory, only enqueued) and shared by every launch that reads them."""

    def __init__(self, sel, sizes):
        self.sel, self.Qs, self.Q = sel, int(sel.shape[0]), int(sizes.shape[0])
        first = np.zeros(self.Q + 1, dtype=np.int64)
        np.cumsum(sizes, out=first[1:])
        if int(first[-1]) >= 2 ** 31 - 1:
            raise IndexError("panel_plan: the proteins hold 2^31 residue rows or more")
        self.N = int(first[-1])
        n_chunks = (sizes[sel] + PANEL_CHUNK - 1) // PANEL_CHUNK                     # per selection
        chunk_ptr = np.zeros(self.Qs + 1, dtype=np.int64)
        np.cumsum(n_chunks, out=chunk_ptr[1:])
        self.total_chunks = T = int(chunk_ptr[-1])
        if T >= 2 ** 31 - 1:
            raise IndexError("panel_plan: the selection has 2^31 chunks or more")
        j = np.repeat(np.arange(self.Qs, dtype=np.int64), n_chunks)
        c = np.arange(T, dtype=np.int64) - chunk_ptr[j]                              # chunk inside its protein
        table = np.empty((T, 4), dtype=np.int32)
        table[:, 0] = j
        table[:, 1] = first[sel[j]] + PANEL_CHUNK * c
        table[:, 2] = np.minimum(sizes[sel[j]] - PANEL_CHUNK * c, PANEL_CHUNK)
        table[:, 3] = np.arange(T)
        self.work = np.concatenate([table.reshape(-1), chunk_ptr.astype(np.int32)])
        self.chunks, self.chunk_ptr = self.work[:4 * T].reshape(T, 4), self.work[4 * T:]
        self._dev = {}

    def on(self, device):
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            both = _stage_int32(np.concatenate([self.sel, self.work]), device, "the panel's selection and work table")      # (one copy)
            t = self._dev[device] = (both[:self.Qs], both[self.Qs:])
        return t


def panel_plan(sizes_host, proteins=None):
    """``PanelPlan`` of the selection ``proteins`` over ``Q = len(sizes_host)`` proteins of ``sizes_host[q]`` residue rows — host only
    (numpy), before anything is launched (the kernel trusts the table; the policy of ``pair_index``).  ``proteins``: ``None`` = all
    ``Q`` in order, or a host sequence / numpy array / CPU tensor of integers in ``[0, Q)``, in any order, duplicates allowed;
    ``IndexError`` for a wrong dtype or an entry outside ``[0, Q)``; a device tensor is refused (validating it would be a hidden
    read-back)."""
    if torch.is_tensor(sizes_host):
        if sizes_host.device.type != "cpu":
            raise GlamHipError("panel_plan: the proteins' sizes live on a device: the plan is built on the host — pass their host copy")
        sizes_host = sizes_host.detach().numpy()
    sizes = np.asarray(sizes_host)
    if sizes.size == 0:
        sizes = np.zeros(0, dtype=np.int64)
    if sizes.dtype.kind not in "iu" or sizes.ndim != 1 or (sizes.size and int(sizes.min()) < 0):
        raise IndexError("panel_plan: the proteins' sizes must be a vector of non-negative integers")
    sizes = sizes.astype(np.int64)
    Q = int(sizes.shape[0])
    if proteins is None:
        return PanelPlan(np.arange(Q, dtype=np.int32), sizes)
    if torch.is_tensor(proteins):
        if proteins.device.type != "cpu":
            raise GlamHipError("proteins lives on a device: it is validated on the host before the launch, which would be a hidden "
                               "read-back — pass the host sequence / numpy array / CPU tensor it was made from")
        proteins = proteins.detach().numpy()
    sel = np.asarray(proteins)
    if sel.size == 0:
        sel = np.zeros(0, dtype=np.int64)
    if sel.dtype.kind not in "iu":
        raise IndexError(f"proteins must hold integers, got {sel.dtype}")
    if sel.ndim != 1:
        raise IndexError(f"proteins must be a vector of protein numbers: shape {tuple(sel.shape)}")
    if sel.size and (int(sel.min()) < 0 or int(sel.max()) >= Q):
        raise IndexError(f"proteins must lie in [0, {Q}): got {int(sel.min())} .. {int(sel.max())}")
    return PanelPlan(sel.astype(np.int32), sizes)


def pair_pool_panel(mol_out, pro_out, msp, psp, plan, molsum=None, prosum=None, return_argmax=False, slab=0):
    """``[max, mean]`` of ``mol[seg_l] @ pro[seg_q].T`` for EVERY ligand ``l`` and every selected protein ``q = plan.sel[j]`` ->
    ``[L, Qs, 2]``: the panel of ``Qs`` calls of ``pair_pool_indexed`` with ``pro_of_pair = [sel[j]] * L`` from one protein-stationary
    launch (+ a finish launch).  The max column — and with ``return_argmax`` the ``[L, Qs, 2]`` int32 rows of the maximum in ``mol_out``
    / ``pro_out`` (-1 for an empty ligand or protein) — is bit for bit that of those calls; the mean is ``<molsum[l], prosum[q]> /
    (n_l n_q)`` and within the fp64-twin bound.  ``plan``: ``panel_plan`` over the sizes of ``psp``'s segments.  ``molsum`` ``[L, D]``
    / ``prosum`` ``[Q, D]``: the segments' column sums (``segment_pool(x, sp, "sum")``), computed here when missing — a caller that
    keeps the proteins keeps ``prosum`` too.  ``slab``: ligands per wave, 0 = the library chooses.  Widths 1..128.  Inference only:
    there is no backward (training is ``ops.pair_pool`` / ``ops.pair_pool_shared``)."""
    if not isinstance(plan, PanelPlan):
        raise GlamHipError("pair_pool_panel: plan must come from ops.panel_plan (the kernel trusts its table)")
    L, Q, Qs = msp.B, psp.B, plan.Qs
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (mol_out, pro_out, molsum, prosum)):
        raise GlamHipError("pair_pool_panel is inference only (no backward): call it under torch.no_grad(); the training routes are "
                           "ops.pair_pool on one protein graph per pair and ops.pair_pool_shared on proteins held once")
    if plan.Q != Q or plan.N != psp.N:
        raise GlamHipError(f"pair_pool_panel: the plan was made for {plan.Q} proteins of {plan.N} residue rows, the encoding holds {Q} of {psp.N}")
    require_device(mol_out, pro_out)
    if (mol_out.dim() != 2 or pro_out.dim() != 2 or mol_out.size(1) != pro_out.size(1) or mol_out.size(0) != msp.N
            or pro_out.size(0) != psp.N):
        raise GlamHipError(f"pair_pool_panel: the two sides disagree (width / node count): mol {tuple(mol_out.shape)} for {msp.N} rows, "
                           f"pro {tuple(pro_out.shape)} for {psp.N} rows")
    D = mol_out.size(1)
    for name, t, rows in (("molsum", molsum, L), ("prosum", prosum, Q)):
        if t is not None and (t.dim() != 2 or tuple(t.shape) != (rows, D) or t.device != mol_out.device):
            raise GlamHipError(f"pair_pool_panel: {name} must be the [{rows}, {D}] column sums on {mol_out.device}, got {tuple(t.shape)} on {t.device}")
    if int(slab) < 0:
        raise GlamHipError(f"pair_pool_panel: slab must be 0 (choose) or the ligands per wave, got {slab}")
    lib = _lib.api()
    if _lib.load().glam_pair_pool_panel_supported(D) != 0:          # (a status: the raw binding hands it back)
        raise GlamHipError(f"pair_pool_panel: width {D} is outside the kernel table (1..128)")
    mol, pro = f32c(mol_out, "mol_out"), f32c(pro_out, "pro_out")
    dev = mol.device
    out = torch.empty(L, Qs, 2, dtype=torch.float32, device=dev)
    arg = torch.empty(L, Qs, 2, dtype=torch.int32, device=dev) if return_argmax else None
    if L == 0 or Qs == 0:
        return (out, arg) if return_argmax else out
    if msp.N == 0 or psp.N == 0:          # no row on one side: every pair is empty (and the empty matrix has no address to pass)
        out.zero_()
        if return_argmax:
            arg.fill_(-1)
        return (out, arg) if return_argmax else out
    molsum =f32c(molsum, "molsum") if molsum is not None else segment_pool(mol, msp, "sum")
    prosum = f32c(prosum, "prosum") if prosum is not None else segment_pool(pro, psp, "sum")
    sel, work = plan.on(dev)
    ws = torch.empty(max(lib.glam_pair_pool_panel_workspace_bytes(plan.total_chunks, L), 16), dtype=torch.uint8, device=dev)
    lib.glam_pair_pool_panel_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(work), plan.total_chunks, ptr(sel), Qs, L, Q, D,
                                 ptr(molsum), ptr(prosum), int(slab), ptr(out), ptr(arg), ptr(ws), ws.numel(), stream())
    return (out, arg) if return_argmax else out


# --------------------------------------------------------------------------------------
# training against proteins held once: the indexed fusion with a backward (csrc/pairshared.hip)
# --------------------------------------------------------------------------------------
class _PairPoolShared(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mol, pro, msp, psp, index, with_identity=False):
        mol_in, pro_in = mol, pro
        mol, pro = f32c(mol, "mol_out"), f32c(pro, "pro_out")
        P, Q, D, dev = msp.B, psp.B, mol.size(1), mol.device
        pidx = index.on(dev)
        order, qptr = index.by_protein().on(dev)
        out = torch.empty(P, 2, dtype=torch.float32, device=dev)
        arg = torch.empty(P, 2, dtype=torch.int32, device=dev)
        sums = torch.empty(P, 2, D, dtype=torch.float32, device=dev)
        lib = _lib.api()
        ws = torch.empty(max(lib.glam_pair_pool_workspace_bytes(P, D), 16), dtype=torch.uint8, device=dev)
        lib.glam_pair_pool_shared_fwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(pidx), P, Q, D, ptr(out), ptr(arg), ptr(sums),
                                      ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(mol, pro, arg, sums, pidx, order, qptr)
        ctx.sps = (msp, psp)
        ctx.aliased = bool(with_identity)
        if ctx.aliased:      # (as _PairPool: what the caller does with the two matrices next sends its gradient HERE)
            ctx.set_materialize_grads(False)
            return out, mol_in.view_as(mol_in), pro_in.view_as(pro_in)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_ma=None, d_pa=None):
        mol, pro, arg, sums, pidx, order, qptr = ctx.saved_tensors
        msp, psp = ctx.sps
        if d_out is None:
            return d_ma, d_pa, None, None, None, None
        d_out = f32c(d_out, "d_out")
        d_ma = None if d_ma is None else f32c(d_ma, "d_mol (next use)")
        d_pa = None if d_pa is None else f32c(d_pa, "d_pro (next use)")
        if msp.B == 0:       # no pair: the entry point writes nothing
            d_mol = torch.zeros_like(mol) if d_ma is None else d_ma
            d_pro = torch.zeros_like(pro) if d_pa is None else d_pa
            return d_mol, d_pro, None, None, None, None
        d_mol, d_pro = torch.empty_like(mol), torch.empty_like(pro)
        _lib.api().glam_pair_pool_shared_bwd(ptr(mol), ptr(pro), ptr(msp.ptr), ptr(psp.ptr), ptr(pidx), ptr(order), ptr(qptr), ptr(arg),
                                             ptr(sums), ptr(d_out), msp.B, psp.B, mol.size(1), ptr(d_ma), ptr(d_pa), ptr(d_mol),
                                             ptr(d_pro), stream())
        return d_mol, d_pro, None, None, None, None


def pair_pool_shared(mol_out, pro_out, msp, psp, pro_of_pair=None, with_identity=False):
    """``pair_pool_indexed`` WITH a backward: ``[max, mean]`` of ``mol[seg_i] @ pro[seg_q].T`` with ``q = pro_of_pair[i]`` -> ``[P, 2]``
    against proteins held once (``psp.B`` segments), for training.  The forward is bit for bit ``pair_pool_indexed``; the gradient of a
    protein's residue rows is the sum over every pair that points at it, taken in batch order without atomics (two runs are
    bit-equal); a protein no pair references gets zeros.  ``pro_of_pair``: see ``pair_index`` (``None`` = identity; every ligand against
    the one protein when ``psp.B == 1``).  ``with_identity``:
    as ``pair_pool`` — ``(out, mol_out, pro_out)`` with the two matrices handed back through the node where its backward launch can
    add their later gradients itself (``glam_pair_pool_add_supported``), the plain triple otherwise."""
    P, Q = msp.B, psp.B
    index = pair_index(pro_of_pair, P, Q, default="single" if Q == 1 and P != 1 else "identity")
    require_device(mol_out, pro_out)
    if (mol_out.dim() != 2 or pro_out.dim() != 2 or mol_out.size(1) != pro_out.size(1) or mol_out.size(0) != msp.N
            or pro_out.size(0) != psp.N):
        raise GlamHipError("pair_pool_shared: the two batches disagree (width / node count)")
    if with_identity:
        D = mol_out.size(1)
        if (torch.is_grad_enabled() and mol_out.requires_grad and pro_out.requires_grad and mol_out.dtype == torch.float32
                and pro_out.dtype == torch.float32 and _lib.api().glam_pair_pool_add_supported(D) == 1):
            return _PairPoolShared.apply(mol_out, pro_out, msp, psp, index, True)
        return _PairPoolShared.apply(mol_out, pro_out, msp, psp, index), mol_out, pro_out
    return _PairPoolShared.apply(mol_out, pro_out, msp, psp, index)


class _PairRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, index):
        pidx = index.on(flat.device)
        order, qptr = index.by_protein().on(flat.device)
        ctx.save_for_backward(order, qptr)
        ctx.dims = (index.P, index.Q, tuple(flat.shape[1:]))
        return flat.index_select(0, pidx)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_rows):
        order, qptr = ctx.saved_tensors
        P, Q, tail = ctx.dims
        d_rows = f32c(d_rows, "d_rows")
        W = int(np.prod(tail, dtype=np.int64))
        if P == 0 or W == 0:
            return torch.zeros((Q,) + tail, dtype=torch.float32, device=d_rows.device), None
        d_flat = torch.empty((Q,) + tail, dtype=torch.float32, device=d_rows.device)
        _lib.api().glam_pair_rows_bwd(ptr(d_rows), ptr(order), ptr(qptr), P, Q, W, ptr(d_flat), stream())
        return d_flat, None


def pair_rows(flat, index):
    """``flat[index]`` -> ``[P, ...]``: the rows of a matrix that holds every protein once, one per pair (``index``: a ``PairIndex`` or
    what ``pair_index`` accepts, over ``flat.size(0)`` rows).  Its backward sums the pairs' rows per protein in batch order
    (``glam_pair_rows_bwd``): ``index_select``'s own backward is an atomic ``index_add``, whose bits change from run to run."""
    if not isinstance(index, PairIndex):
        index = pair_index(index, len(index), flat.size(0))
    elif index.Q != flat.size(0):
        raise IndexError(f"pair_rows: the index was validated over {index.Q} rows, the matrix has {flat.size(0)}")
    require_device(flat)
    if flat.dtype != torch.float32:
        raise GlamHipError(f"pair_rows: expected float32, got {flat.dtype}")
    return _PairRows.apply(flat, index)


# --------------------------------------------------------------------------------------
# drug x drug: the fusion with BOTH sides held once and both indexed (csrc/pairgather.hip, glam_pair_pool_gather_fwd)
# --------------------------------------------------------------------------------------
def pair_pool_gather(x1, x2, sp1, sp2, idx1=None, idx2=None, return_argmax=False):
    """``[max, mean]`` of ``x1[seg_a] @ x2[seg_b].T`` with ``a = idx1[i]``, ``b = idx2[i]`` -> ``[P, 2]``: ``pair_pool`` on two sets of
    small segments that are each held once (``sp1.B`` / ``sp2.B`` of them) — one wave per pair, one launch.  The max column — and with
    ``return_argmax`` the ``[P, 2]`` int32 rows of the maximum in ``x1`` / ``x2`` (-1 for an empty pair) — is bit for bit that of
    ``pair_pool`` on physically gathered rows; the mean is the same bits on every run and within the fp64-twin bound.
    ``idx1`` / ``idx2``: see ``pair_index``; ``None`` = identity on that side (needs ``sp.B == P``); ``P`` is the length of whichever is
    given.  Widths 1..128.  Inference only: there is no backward (training is ``ops.pair_pool`` on one graph per pair and side)."""
    Q1, Q2 = sp1.B, sp2.B
    given = idx1 if idx1 is not None else idx2
    P = Q1 if given is None else given.P if isinstance(given, PairIndex) else len(given)
    i1 = None if idx1 is None and Q1 == P else pair_index(idx1, P, Q1, name="idx1", over="segments of x1")
    i2 = None if idx2 is None and Q2 == P else pair_index(idx2, P, Q2, name="idx2", over="segments of x2")
    if torch.is_grad_enabled() and (x1.requires_grad or x2.requires_grad):
        raise GlamHipError("pair_pool_gather is inference only (no backward): call it under torch.no_grad(); the training route is "
                           "ops.pair_pool on one graph per pair and side")
    require_device(x1, x2)
    if x1.dim() != 2 or x2.dim() != 2 or x1.size(1) != x2.size(1) or x1.size(0) != sp1.N or x2.size(0) != sp2.N:
        raise GlamHipError(f"pair_pool_gather: the two sides disagree (width / node count): x1 {tuple(x1.shape)} for {sp1.N} rows, "
                           f"x2 {tuple(x2.shape)} for {sp2.N} rows")
    x1, x2 = f32c(x1, "x1"), f32c(x2, "x2")
    D = x1.size(1)
    lib = _lib.api()
    if lib.glam_pair_pool_gather_load_bytes(ptr(x1), ptr(x2), D) == 0:
        raise GlamHipError(f"pair_pool_gather: width {D} is outside the kernel table (1..128)")
    out = torch.empty(P, 2, dtype=torch.float32, device=x1.device)
    arg = torch.empty(P, 2, dtype=torch.int32, device=x1.device) if return_argmax else None
    lib.glam_pair_pool_gather_fwd(ptr(x1), ptr(x2), ptr(sp1.ptr), ptr(sp2.ptr), ptr(None if i1 is None else i1.on(x1.device)),
                                  ptr(None if i2 is None else i2.on(x1.device)), P, Q1, Q2, D, ptr(out), ptr(arg), stream())
    return (out, arg) if return_argmax else out


# --------------------------------------------------------------------------------------
# training on drugs held once: the gathered fusion with a backward (csrc/pairgather.hip train_fwd, csrc/pairgather_bwd.hip)
# --------------------------------------------------------------------------------------
class _PairPoolGatherShared(torch.autograd.Function):
    """``i1`` / ``i2``: the validated ``PairIndex`` of each side (an identity side too: its by-drug lists are read by the backward);
    ``null1`` / ``null2``: hand the kernels a NULL index on that side (identity)."""

    @staticmethod
    def forward(ctx, x1, x2, sp1, sp2, i1, i2, null1, null2, with_identity=False):
        x1_in, x2_in = x1, x2
        x1, x2 = f32c(x1, "x1"), f32c(x2, "x2")
        P, Q1, Q2, D, dev = i1.P, sp1.B, sp2.B, x1.size(1), x1.device
        d1, d2 = i1.on(dev), i2.on(dev)
        order1, lptr1 = i1.by_protein().on(dev)
        order2, lptr2 = i2.by_protein().on(dev)
        out = torch.empty(P, 2, dtype=torch.float32, device=dev)
        arg = torch.empty(P, 2, dtype=torch.int32, device=dev)
        sums = torch.empty(P, 2, D, dtype=torch.float32, device=dev)
        ctx.rows = x1.size(0) > 0 and x2.size(0) > 0
        if ctx.rows:
            _lib.api().glam_pair_pool_gather_train_fwd(ptr(x1), ptr(x2), ptr(sp1.ptr), ptr(sp2.ptr), ptr(None if null1 else d1),
                                                       ptr(None if null2 else d2), P, Q1, Q2, D, ptr(out), ptr(arg), ptr(sums), stream())
        else:                # no row on one side: every pair is empty (and the empty matrix has no address to pass)
            out.zero_()
            arg.fill_(-1)
        ctx.save_for_backward(x1, x2, arg, sums, d1, d2, order1, lptr1, order2, lptr2)
        ctx.sps, ctx.null, ctx.P = (sp1, sp2), (bool(null1), bool(null2)), P
        ctx.aliased = bool(with_identity)
        if ctx.aliased:      # (as _PairPool: what the caller does with the two matrices next sends its gradient HERE)
            ctx.set_materialize_grads(False)
            return out, x1_in.view_as(x1_in), x2_in.view_as(x2_in)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_a1=None, d_a2=None):
        x1, x2, arg, sums, d1, d2, order1, lptr1, order2, lptr2 = ctx.saved_tensors
        sp1, sp2 = ctx.sps
        none = (None,) * 7
        if d_out is None:
            return (d_a1, d_a2) + none
        d_out = f32c(d_out, "d_out")
        d_a1 = None if d_a1 is None else f32c(d_a1, "d_x1 (next use)")
        d_a2 = None if d_a2 is None else f32c(d_a2, "d_x2 (next use)")
        if ctx.P == 0 or not ctx.rows:       # no pair, or only empty ones: the entry point writes nothing
            return (torch.zeros_like(x1) if d_a1 is None else d_a1, torch.zeros_like(x2) if d_a2 is None else d_a2) + none
        d_x1, d_x2 = torch.empty_like(x1), torch.empty_like(x2)
        _lib.api().glam_pair_pool_gather_bwd(ptr(x1), ptr(x2), ptr(sp1.ptr), ptr(sp2.ptr), ptr(None if ctx.null[0] else d1),
                                             ptr(None if ctx.null[1] else d2), ptr(order1), ptr(lptr1), ptr(order2), ptr(lptr2), ptr(arg),
                                             ptr(sums), ptr(d_out), ctx.P, sp1.B, sp2.B, x1.size(1), ptr(d_a1), ptr(d_a2), ptr(d_x1),
                                             ptr(d_x2), stream())
        return (d_x1, d_x2) + none


def pair_pool_gather_shared(x1, x2, sp1, sp2, idx1=None, idx2=None, with_identity=False):
    """``pair_pool_gather`` WITH a backward: ``[max, mean]`` of ``x1[seg_a] @ x2[seg_b].T`` with ``a = idx1[i]``, ``b = idx2[i]`` ->
    ``[P, 2]`` on two sets of small segments that are each held once, for training.  The forward is bit for bit ``pair_pool_gather``; the
    gradient of a segment's rows — on EITHER side — is the sum over every pair that points at it, taken in batch order without atomics
    (two runs are bit-equal, one launch for both sides); a segment no pair references gets zeros.  ``idx1`` / ``idx2``: as
    ``pair_pool_gather`` (``pair_index``; ``None`` = identity on that side, needs ``sp.B == P``); keep ONE ``PairIndex`` per side across
    the steps that use it — its device copies are made on the first, eager, visit and a hipGraph capture needs them to exist.  Widths
    1..128.  ``with_identity``: as ``pair_pool`` — ``(out, x1, x2)`` with the two matrices handed back through the node (both require
    grad, fp32): its backward launch then adds their later gradients itself; the plain triple otherwise."""
    Q1, Q2 = sp1.B, sp2.B
    given = idx1 if idx1 is not None else idx2
    P = Q1 if given is None else given.P if isinstance(given, PairIndex) else len(given)
    i1 = pair_index(idx1, P, Q1, name="idx1", over="segments of x1")
    i2 = pair_index(idx2, P, Q2, name="idx2", over="segments of x2")
    require_device(x1, x2)
    if x1.dim() != 2 or x2.dim() != 2 or x1.size(1) != x2.size(1) or x1.size(0) != sp1.N or x2.size(0) != sp2.N:
        raise GlamHipError(f"pair_pool_gather_shared: the two sides disagree (width / node count): x1 {tuple(x1.shape)} for {sp1.N} rows, "
                           f"x2 {tuple(x2.shape)} for {sp2.N} rows")
    D = x1.size(1)
    if not 1 <= D <= 128:
        raise GlamHipError(f"pair_pool_gather_shared: width {D} is outside the kernel table (1..128)")
    args = (x1, x2, sp1, sp2, i1, i2, idx1 is None, idx2 is None)
    if with_identity:
        # (the add runs inside the backward launch for every width of the table: 1 <= D <= 128, checked above)
        if (torch.is_grad_enabled() and x1.requires_grad and x2.requires_grad and x1.dtype == torch.float32 and x2.dtype == torch.float32):
            return _PairPoolGatherShared.apply(*args, True)
        return _PairPoolGatherShared.apply(*args), x1, x2
    return _PairPoolGatherShared.apply(*args)
