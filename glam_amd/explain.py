"""What a trained model attends to: the explanation pass behind the reference's ``src_1gp/visualize_gp.py``.

The fused kernels never write an attention weight (the training forward keeps the segment max and exp-sum, the inference forward
nothing).  The functions here compute them from the INPUTS of a conv / readout with three small inference-only kernels
(``csrc/attn_export.hip``): per-edge, per-head attention of a message step, per-atom "attention sent", and the readout's per-node
weights.  ``explain(model, batch)`` runs one eager eval forward of an ``Architecture``, captures those inputs with forward
pre-hooks and returns everything ``visualize_gp.py`` paints from.  No autograd, no CPU path: CPU tensors raise ``GlamHipError``.

The two-tower models have ``explain_pair``: the scoring call (``screen`` / ``score_pairs``) plus, per message step, the maps of its
fusion — per atom the best partner row and the mean over the partner's rows, and the same per residue / per atom of the other drug
(``ops.pair_map``, ``csrc/pairmap.hip``: one launch for both sides, the score matrix never stored).
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional

import torch
import torch.nn.functional as F

from . import _lib, layer, ops
from ._lib import GlamHipError, f32c, ptr, require_device, stream
from .layer import _ceil4, _pad_de


# --------------------------------------------------------------------------------------
# the three launches
# --------------------------------------------------------------------------------------
def edge_attention(a_ij, edge_attr, M, gi, heads, slope=0.2):
    """``alpha[E, heads]`` (a view of ``[E, 4]`` storage, caller's edge order) of the separable logits
    ``leaky(a_ij[dst, h] + <edge_attr[e], M[:, h]> + a_ij[src, 4 + h])`` soft-maxed over the incoming edges of every target:
    ``a_ij[N, 8]``, ``edge_attr[E, De]`` with ``De`` in {4, 8}, ``M[De, 4]``, ``gi`` the ``GraphIndex``, ``1 <= heads <= 4``."""
    require_device(a_ij, edge_attr, M)
    a_ij, edge_attr, M = f32c(a_ij, "a_ij"), f32c(edge_attr, "edge_attr"), f32c(M, "M")
    N, E = gi.N, gi.E
    De = edge_attr.size(1) if edge_attr.dim() == 2 else -1
    if a_ij.shape != (N, 8) or edge_attr.shape != (E, De) or M.shape != (De, 4):
        raise GlamHipError(f"edge_attention: shape mismatch a_ij={tuple(a_ij.shape)} edge_attr={tuple(edge_attr.shape)} M={tuple(M.shape)} "
                           f"for N={N} E={E}")
    alpha4 = torch.zeros(E, 4, dtype=torch.float32, device=a_ij.device)
    _lib.api().glam_edge_attention(ptr(a_ij), ptr(edge_attr), ptr(M), ptr(gi.rowptr), ptr(gi.src), ptr(gi.eid), N, E, int(heads), De,
                                   float(slope), ptr(alpha4), stream())
    return alpha4[:, :heads]


def _alpha4(alpha):
    """The ``[E, 4]`` storage behind ``alpha[E, H]`` when it is the view ``edge_attention`` returned, else a zero-padded copy."""
    base = alpha._base
    if (base is not None and base.shape == (alpha.size(0), 4) and base.is_contiguous() and base.dtype == torch.float32
            and alpha.stride() == (4, 1) and alpha.storage_offset() == base.storage_offset()):
        return base
    return F.pad(alpha, (0, 4 - alpha.size(1))).contiguous() if alpha.size(1) != 4 else f32c(alpha, "alpha")


def attention_sent(alpha, gi):
    """``sent[N, heads]``: ``sent[n, h]`` = sum of ``alpha[e, h]`` over the edges that leave ``n`` — how much its neighbours listen to
    atom ``n``.  Summed in the order of the CSR by source, so bit-reproducible."""
    require_device(alpha)
    if alpha.dim() != 2 or alpha.size(0) != gi.E or alpha.dtype != torch.float32:
        raise GlamHipError(f"attention_sent: alpha must be float32 [E={gi.E}, heads], got {alpha.dtype} {tuple(alpha.shape)}")
    H = alpha.size(1)
    if H > 4:
        return torch.cat([attention_sent(alpha[:, h0:h0 + 4], gi) for h0 in range(0, H, 4)], dim=1)
    sent = torch.zeros(gi.N, 4, dtype=torch.float32, device=alpha.device)
    if H == 0:
        return sent[:, :0]
    colptr, _, eid_t = gi.transpose()
    _lib.api().glam_edge_attention_sent(ptr(_alpha4(alpha)), ptr(colptr), ptr(eid_t), gi.N, gi.E, H, ptr(sent), stream())
    return sent[:, :H]


def segment_softmax(gate, sp):
    """``w[N]``: the softmax of ``gate[N]`` over the nodes of every graph of ``sp`` (a ``SegmentPtr``)."""
    require_device(gate)
    gate = f32c(gate.reshape(-1), "gate")
    if gate.numel() != sp.N:
        raise GlamHipError("segment_softmax: gate and the batch vector disagree on the node count")
    w = torch.zeros(sp.N, dtype=torch.float32, device=gate.device)
    _lib.api().glam_segment_softmax(ptr(gate), None, None, ptr(sp.ptr), sp.N, sp.B, 1, 1, ptr(w), stream())
    return w


def query_softmax(x, q, sp):
    """``w[N]``: the softmax over every graph's nodes of ``<x_n, q_g>`` (Set2Set's read), the logits formed in the kernel from
    ``x[N, D]`` and ``q[B, D]``.  Odd widths run on rows zero-padded to a multiple of four; more than 128 channels raise."""
    require_device(x, q)
    if x.dim() != 2 or q.dim() != 2 or x.size(0) != sp.N or q.shape != (sp.B, x.size(1)):
        raise GlamHipError("query_softmax: x / q disagree with the batch vector")
    D = x.size(1)
    ld = _ceil4(D)
    if ld != D:
        x, q = ops.pad_cols(x, ld), F.pad(q, (0, ld - D))
    x, q = f32c(x, "x"), f32c(q, "q")
    w = torch.zeros(sp.N, dtype=torch.float32, device=x.device)
    _lib.api().glam_segment_softmax(None, ptr(x), ptr(q), ptr(sp.ptr), sp.N, sp.B, D, ld, ptr(w), stream())
    return w


# --------------------------------------------------------------------------------------
# modules
# --------------------------------------------------------------------------------------
_ATTENTION_CONVS = (layer.TripletMessage, layer.TripletMessageLight, layer.GATConv)
_WRAPPERS = (layer._TripletMessage, layer._TripletMessageLight, layer._GATConv, layer._NNConv, layer._GCNConv)


def _row_padded(Wa, M, C):
    """``Wa`` with its input rows zero-padded to the padded width the rows flow at."""
    return F.pad(Wa, (0, 0, 0, _ceil4(C) - C)).contiguous(), M.contiguous()


def conv_attention(conv, x, edge_index, edge_attr=None):
    """``(edge_index_used, alpha[E', H])`` of one application of ``conv`` to ``x``: a ``TripletMessage``, ``TripletMessageLight`` or
    ``GATConv`` (or its ``_...`` wrapper).  For GATConv this is PyG's ``return_attention_weights=True`` pair: the edge list WITH the
    self loops its forward adds.  ``NNConv`` / ``GCNConv`` have no attention and raise."""
    return _conv_attention(conv, x, edge_index, edge_attr)[:2]


@torch.no_grad()
def _conv_attention(conv, x, edge_index, edge_attr):
    """``conv_attention`` + the ``GraphIndex`` of the edge list it returns."""
    if isinstance(conv, _WRAPPERS):
        conv = conv.conv
    if not isinstance(conv, _ATTENTION_CONVS):
        raise GlamHipError(f"conv_attention: {type(conv).__name__} has no attention weights (TripletMessage, TripletMessageLight, GATConv do)")
    require_device(x, edge_index, edge_attr)
    N = x.size(0)
    if isinstance(conv, layer.GATConv):
        C = conv.out_channels
        gi0 = ops.graph_index(edge_index, N)
        ei, gi, _ = layer._with_self_loops(gi0, edge_index, N, False)
        xl = ops.linear(x, conv.lin_l.weight, conv.lin_l.bias)
        a_r = (xl * conv.att_r.view(1, C)).sum(-1, keepdim=True)                       # target side, as GATConv.forward
        a_l = (xl * conv.att_l.view(1, C)).sum(-1, keepdim=True)
        a_ij = torch.cat([F.pad(a_r, (0, 3)), F.pad(a_l, (0, 3))], dim=1)
        return ei, edge_attention(a_ij, x.new_zeros(ei.size(1), 4), x.new_zeros(4, 4), gi, 1, conv.negative_slope), gi
    if edge_attr is None:
        raise GlamHipError(f"conv_attention: {type(conv).__name__} needs edge_attr")
    C, De = conv.node_channels, conv.edge_channels
    edge_attr = edge_attr.unsqueeze(-1) if edge_attr.dim() == 1 else edge_attr
    if x.dim() != 2 or x.size(1) != C or edge_attr.size(1) != De:
        raise GlamHipError(f"conv_attention: x has {x.size(1)} and edge_attr {edge_attr.size(1)} columns; expected ({C}, {De})")
    Cp, Dp = _ceil4(C), _pad_de(De)
    gi = ops.graph_index(edge_index, N)
    ea = F.pad(edge_attr, (0, Dp - De)) if Dp != De else edge_attr
    x_p = ops.pad_cols(x, Cp)
    if isinstance(conv, layer.TripletMessageLight):
        Wa, M = ops.scoped_weights(("light-attention", id(conv.weight_node)), conv.weight_node, lambda: _row_padded(*conv._attention_weights(), C))
        return edge_index, edge_attention(ops.matmul_tall(x_p, Wa), ea, M, gi, 1, conv.negative_slope), gi
    if conv.heads <= 4:
        _, Wa, _, M, _, _, _ = ops.scoped_weights(("triplet-derived", id(conv.weight_node)), conv.weight_node, conv._staged_wide)
        return edge_index, edge_attention(ops.matmul_tall(x_p, Wa), ea, M, gi, conv.heads, conv.negative_slope), gi
    parts = []                 # heads > 4: groups of at most four, as the layer itself runs them (TripletMessage._head_groups)
    for h0 in range(0, conv.heads, 4):
        h1 = min(h0 + 4, conv.heads)
        Wa, M = ops.scoped_weights(("triplet-attention", id(conv.weight_node), h0), conv.weight_node, lambda: _row_padded(*conv._attention_weights(h0, h1), C))
        parts.append(edge_attention(ops.matmul_tall(x_p, Wa), ea, M, gi, h1 - h0, conv.negative_slope))
    return edge_index, torch.cat(parts, dim=1), gi


@torch.no_grad()
def readout_attention(readout, x, batch, num_graphs=None):
    """The per-node weights of ``readout`` on ``x``: ``[N]`` for ``GlobalLAPool`` / ``GlobalAttention``; ``[processing_steps, N]`` for
    ``Set2Set``, one row per step of the same LSTM recurrence as its forward.  ``GlobalPool5`` has none and raises."""
    if isinstance(readout, layer.GlobalLAPool):
        readout = readout.pool
    if not isinstance(readout, (layer.GlobalAttention, layer.Set2Set)):
        raise GlamHipError(f"readout_attention: {type(readout).__name__} has no attention weights (GlobalLAPool, GlobalAttention, Set2Set do)")
    require_device(x, batch)
    sp = ops.segment_ptr(batch, num_graphs)
    if isinstance(readout, layer.GlobalAttention):
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        g = readout.gate_nn
        gate = ops.linear(x, g.weight, g.bias) if type(g) is torch.nn.Linear else g(x)
        return segment_softmax(gate.view(-1), sp)
    B, C, L = sp.B, readout.in_channels, readout.lstm
    Cp = _ceil4(C)
    fused = ops.query_attention_supported(Cp)
    h, c, q_star = x.new_zeros(B, C), x.new_zeros(B, C), x.new_zeros(B, 2 * C)
    x_p = ops.pad_cols(x, Cp) if fused else x
    bias = L.bias_ih_l0 + L.bias_hh_l0
    steps = []
    for _ in range(readout.processing_steps):                  # Set2Set.forward, with the weights kept
        if fused:
            gates = torch.addmm(torch.addmm(bias, q_star, L.weight_ih_l0.t()), h, L.weight_hh_l0.t())
            h, c = ops.lstm_cell(gates, c)
            h_p = h if Cp == C else F.pad(h, (0, Cp - C))
            steps.append(query_softmax(x_p, h_p, sp))
            r = ops.query_attention(x_p, h_p, sp)
            q_star = torch.cat([h, r if Cp == C else r[:, :C]], dim=-1)
            continue
        gates = F.linear(q_star, L.weight_ih_l0, L.bias_ih_l0) + F.linear(h, L.weight_hh_l0, L.bias_hh_l0)
        i, f, g, o = gates.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        e = (x * h.index_select(0, batch)).sum(dim=-1)
        steps.append(segment_softmax(e, sp))
        q_star = torch.cat([h, ops.segment_attention(e, x, sp)], dim=-1)
    return torch.stack(steps) if steps else x.new_zeros(0, sp.N)


# --------------------------------------------------------------------------------------
# the whole model
# --------------------------------------------------------------------------------------
@dataclasses.dataclass
class Explanation:
    """What ``explain`` returns.  ``out[B, out_dim]`` the prediction; ``hidden[N, C]`` the final node rows (the ``xm`` the reference's
    visualizer model returns beside ``out``); ``edge_index[2, E']`` the edges ``edge_attention`` speaks about (GATConv: with its self
    loops); ``edge_attention`` / ``atom_sent``: per message step ``[E', H]`` / ``[N, H]``, ``None`` for a conv without attention;
    ``readout_attention``: ``[N]``, ``[steps, N]`` (Set2Set) or ``None``; ``ptr[B + 1]`` the node range of every molecule."""
    out: torch.Tensor
    hidden: torch.Tensor
    edge_index: torch.Tensor
    edge_attention: List[Optional[torch.Tensor]]
    atom_sent: List[Optional[torch.Tensor]]
    readout_attention: Optional[torch.Tensor]
    ptr: torch.Tensor

    CONTENTS = ("hidden_node", "lapool_attention", "set2set_attention", "edge_attention")

    def weights(self, content="hidden_node"):
        """The per-atom ``[N]`` vector the visualizer paints: ``'hidden_node'`` = ``hidden.mean(-1)`` (visualize_gp.py:109),
        ``'lapool_attention'`` the readout's weights, ``'set2set_attention'`` those of the last processing step, ``'edge_attention'`` the
        last message step's attention sent, averaged over heads."""
        if content == "hidden_node":
            return self.hidden.mean(dim=-1)
        if content in ("lapool_attention", "set2set_attention"):
            w = self.readout_attention
            if w is None or w.dim() != (1 if content == "lapool_attention" else 2):
                raise ValueError(f"{content!r}: the model's readout gave no such weights")
            return w if w.dim() == 1 else w[-1]
        if content == "edge_attention":
            if not self.atom_sent or self.atom_sent[-1] is None:
                raise ValueError("'edge_attention': the model's conv has no attention weights")
            return self.atom_sent[-1].mean(dim=-1)
        raise ValueError(f"Unknown content to visualize: {content!r} (one of {self.CONTENTS})")

    def per_molecule(self, t, per=None):
        """``t`` split by molecule into a list of ``B`` tensors: along its first dimension, which runs over nodes (``per='node'``) or over
        the edges of ``edge_index`` (``per='edge'``, an edge belongs to its target's molecule; the edges of a molecule keep their order).
        ``per=None`` takes whichever of the two counts matches, nodes first."""
        N, E = self.hidden.size(0), self.edge_index.size(1)
        if per is None:
            per = "node" if t.size(0) == N else "edge"
        if per not in ("node", "edge") or t.size(0) != (N if per == "node" else E):
            raise ValueError(f"per_molecule: the first dimension ({t.size(0)}) is neither the node count {N} nor the edge count {E}")
        bounds = self.ptr.to(device=t.device, dtype=torch.int64)
        if per == "node":
            return list(t.split((bounds[1:] - bounds[:-1]).tolist()))
        gid = torch.bucketize(self.edge_index[1].to(t.device), bounds[1:], right=True)
        order = torch.argsort(gid, stable=True)
        counts = torch.bincount(gid, minlength=bounds.numel() - 1)
        return list(t.index_select(0, order).split(counts.tolist()))


def explain(model, batch):
    """One eager eval forward of ``model`` (an ``Architecture``) on ``batch`` plus a handful of small launches -> ``Explanation``.
    The model must be in eval mode: training-mode RReLU and Dropout would make the explanation random."""
    from .model import Architecture
    if not isinstance(model, Architecture):
        raise GlamHipError(f"explain: expected an Architecture, got {type(model).__name__} (the two-tower models have explain_pair: the "
                           "per-atom and per-residue maps of their fusion; conv_attention / readout_attention work on their blocks)")
    if model.training:
        raise GlamHipError("explain: the model is in training mode (RReLU slopes and Dropout masks are random there): call model.eval() first")
    require_device(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
    conv = model.mol_conv.conv.conv
    conv_in, readout_in = [], []
    hooks = [conv.register_forward_pre_hook(lambda m, args: conv_in.append(args)),
             model.mol_readout.register_forward_pre_hook(lambda m, args: readout_in.append(args))]
    try:
        with torch.no_grad():
            out = model._eager_forward(batch)          # the eager route: a hipGraph replay runs no hooks
    finally:
        for h in hooks:
            h.remove()
    if len(conv_in) != model.message_steps or len(readout_in) != 1:
        raise GlamHipError(f"explain: captured {len(conv_in)} conv and {len(readout_in)} readout applications, expected "
                           f"{model.message_steps} and 1")
    hidden, node_batch = readout_in[0][0], readout_in[0][1]
    num_graphs = readout_in[0][2] if len(readout_in[0]) > 2 else None
    sp = ops.segment_ptr(node_batch, num_graphs)
    has_attention = isinstance(conv, _ATTENTION_CONVS)
    edge_index, alphas, sents = batch.edge_index, [], []
    with ops.weight_scope():                           # (the attention weights are derived once for the message_steps applications)
        for args in conv_in:
            if not has_attention:
                alphas.append(None)
                sents.append(None)
                continue
            edge_index, alpha, gi = _conv_attention(conv, args[0], args[1], args[2] if len(args) > 2 else None)
            alphas.append(alpha)
            sents.append(attention_sent(alpha, gi))
    ro = model.mol_readout
    w = readout_attention(ro, hidden, node_batch, num_graphs) if isinstance(ro, (layer.GlobalLAPool, layer.GlobalAttention, layer.Set2Set)) else None
    return Explanation(out=out, hidden=hidden, edge_index=edge_index, edge_attention=alphas, atom_sent=sents, readout_attention=w, ptr=sp.ptr)


# --------------------------------------------------------------------------------------
# the pair models: what the fusion pools from
# --------------------------------------------------------------------------------------
@dataclasses.dataclass
class PairExplanation:
    """What ``explain_pair`` returns.  ``out[P, out_dim]`` the prediction, bit for bit ``screen`` / ``score_pairs``; ``fusion[P, 2 *
    message_steps]`` the ``[max, mean]`` columns the head saw, step by step; ``contacts``: per step the ``[P, 2]`` int32 rows of the maximum
    (``return_argmax`` of those calls); ``maps``: per step an ``ops.PairMap`` — side 1 the ligand's atoms (DTI) / the first drug's (DDI),
    side 2 the residues / the second drug's atoms, ragged and pair-major; ``ptr1`` / ``ptr2`` int32 ``[P + 1]``: the rows of pair ``i`` in
    the side's vectors."""
    out: torch.Tensor
    fusion: torch.Tensor
    contacts: List[torch.Tensor]
    maps: list
    ptr1: torch.Tensor
    ptr2: torch.Tensor

    CONTENTS = ("max", "mean")

    def per_pair(self, t, side):
        """``t``, whose first dimension runs over the rows of ``side`` (1 or 2), split into a list of ``P`` tensors."""
        if side not in (1, 2):
            raise ValueError(f"per_pair: side must be 1 or 2, got {side!r}")
        bounds = (self.ptr1 if side == 1 else self.ptr2).to(dtype=torch.int64)
        sizes = (bounds[1:] - bounds[:-1]).tolist()
        if t.size(0) != sum(sizes):
            raise ValueError(f"per_pair: the first dimension ({t.size(0)}) is not the row count of side {side} ({sum(sizes)})")
        return list(t.split(sizes))

    def weights(self, side, content="max", step=-1):
        """The per-row ``[R]`` vector a painter would use for ``side`` (1 or 2): ``'max'`` = the row's best score against the partner,
        ``'mean'`` its mean score, of message step ``step`` (the last by default)."""
        if side not in (1, 2):
            raise ValueError(f"weights: side must be 1 or 2, got {side!r}")
        if content not in self.CONTENTS:
            raise ValueError(f"Unknown content to visualize: {content!r} (one of {self.CONTENTS})")
        if not self.maps:
            raise ValueError("weights: the model has no message step, so no fusion and no map")
        return getattr(self.maps[step], f"{content}{side}")


def explain_pair(model, *args, **kwargs):
    """Why a pair scored as it did: the scoring call of a two-tower model plus one ``ops.pair_map`` launch per message step ->
    ``PairExplanation``.  ``eval()`` mode under ``torch.no_grad()``; every refusal of ``screen`` / ``score_pairs`` applies.

    ``ArchitectureDTI``: ``explain_pair(model, data_mol, enc, pro_of_pair=None)`` — ``screen`` on a ``ProteinEncoding`` — or
    ``explain_pair(model, data_mol, data_pro)`` with one protein graph per ligand (encoded here, then the same path).
    ``ArchitectureDDI``: ``explain_pair(model, enc, first, second)`` — ``score_pairs`` on a ``DrugEncoding``."""
    from .model import ArchitectureDDI, ArchitectureDTI
    if isinstance(model, ArchitectureDTI):
        return _explain_dti(model, *args, **kwargs)
    if isinstance(model, ArchitectureDDI):
        return _explain_ddi(model, *args, **kwargs)
    raise GlamHipError(f"explain_pair: expected an ArchitectureDTI or ArchitectureDDI, got {type(model).__name__} (explain() takes an Architecture)")


def _pair_explanation(out, fusion, contacts, maps, plan):
    _, ptr1, ptr2 = plan.on(out.device)
    fusion = torch.cat(fusion, dim=1) if fusion else out.new_zeros(plan.P, 0)
    return PairExplanation(out=out, fusion=fusion, contacts=contacts, maps=maps, ptr1=ptr1, ptr2=ptr2)


def _explain_dti(model, data_mol, enc, pro_of_pair=None):
    from .model import ProteinEncoding, _host_sizes
    model._screen_guard("explain_pair")          # (before the batch form's encode_proteins, which would name itself in the refusal)
    if not isinstance(enc, ProteinEncoding):
        if not all(hasattr(enc, k) for k in ("x", "edge_index", "edge_attr", "batch")):
            raise GlamHipError("explain_pair: for an ArchitectureDTI the call is explain_pair(model, data_mol, enc, pro_of_pair=None) on a "
                               "ProteinEncoding (model.encode_proteins) or explain_pair(model, data_mol, data_pro) on a batch of one protein "
                               f"graph per ligand, got {type(enc).__name__}")
        enc = model.encode_proteins(enc)                # one protein graph per ligand: encoded once, then the identity index
        if pro_of_pair is None:
            pro_of_pair = range(enc.num_graphs)
    out, contacts, fusion, rows, msp, index = model._screen("explain_pair", data_mol, enc, pro_of_pair, True)
    bounds = msp.ptr.cpu().numpy().astype("int64")      # (the ligands' sizes: one read-back, after the pass is enqueued)
    plan = ops.map_plan(bounds[1:] - bounds[:-1], _host_sizes(enc), None, index)
    maps = [layer.dot_and_global_pool2_map(x, r, msp, enc.sp, plan) for x, r in zip(rows, enc.rows)]
    return _pair_explanation(out, fusion, contacts, maps, plan)


def _explain_ddi(model, enc, first=None, second=None):
    from .model import DrugEncoding, _host_sizes
    model._pairs_guard("explain_pair")
    if not isinstance(enc, DrugEncoding) or first is None or second is None:
        raise GlamHipError("explain_pair: for an ArchitectureDDI the call is explain_pair(model, enc, first, second) on a DrugEncoding; two "
                           "collated batches are not taken — enc = model.encode_drugs(batch) first, then the pairs as two index vectors")
    out, contacts, fusion, i1, i2 = model._score_pairs("explain_pair", enc, first, second, True)
    sizes = _host_sizes(enc)
    plan = ops.map_plan(sizes, sizes, i1, i2)
    maps = [layer.dot_and_global_pool2_map(r1, r2, enc.sp, enc.sp, plan) for r1, r2 in zip(enc.rows1, enc.rows2)]
    return _pair_explanation(out, fusion, contacts, maps, plan)
