"""MI355X drop-in for the reference's model assembly (``src_1gp/model.py``).

``Architecture`` / ``Model`` keep the reference constructor keywords (``model.py:24-33``), the
sub-module names (checkpoint keys ``mol_lin0.*``, ``mol_conv.*``, ``mol_readout.*``, ``mol_flat.*``,
``lin_out1.*``) and the call ``model(batch) -> [B, out_dim]`` used by the reference trainers
(``trainer.py:295``).  ``ArchitectureDDI`` mirrors the two-drug variant (``src_2gi_ddi/model.py:9-62``), ``ArchitectureDTI`` the two-tower variant
(``src_2gi_dti_scr/model.py:14-68``).
"""
from __future__ import annotations

import weakref

import torch

from . import graphs, hits, ops
from ._lib import GlamHipError

from .layer import _None  # noqa: F401
from .layer import GlobalPool5, GlobalLAPool, Set2Set  # noqa: F401  (resolved from config strings)
from .layer import LinearBlock, MessageBlock, dot_and_global_pool2, first_node_spec, flat_then_head, following_dropout, prestage_pass
from .layer import _BatchNorm, _LayerNorm, _PairNorm, dot_and_global_pool2_gather, dot_and_global_pool2_indexed, dot_and_global_pool2_shared
from .layer import dot_and_global_pool2_gather_shared, dot_and_global_pool2_grid, dot_and_global_pool2_panel
from .layer import dot_and_global_pool2_panel_shared


def model_args(args):
    """Filter a run.py-style ``Namespace`` down to constructor keywords (model.py:7-15)."""
    other = ["dataset_root", "dataset", "split", "seed", "gpu", "note", "batch_size", "epochs", "loss", "optim", "k",
             "lr", "lr_reduce_rate", "lr_reduce_patience", "early_stop_patience", "verbose_patience", "split_seed",
             "test"]
    return {k: v for k, v in args.__dict__.items() if k not in other}


def _readout(name, hid_dim):
    return eval("{}(in_channels=hid_dim, processing_steps=3)".format(name), globals(), {"hid_dim": hid_dim})  # noqa: S307


class Architecture(torch.nn.Module):
    def __init__(self, mol_in_dim=15, mol_edge_in_dim=4, hid_dim_alpha=4, e_dim=1024, out_dim=1,
                 mol_block="_NNConv", message_steps=3, mol_readout="GlobalPool5",
                 pre_norm="_None", graph_norm="_None", flat_norm="_None", end_norm="_None",
                 pre_do="_None()", graph_do="Dropout(0.2)", flat_do="_None()", end_do="Dropout(0.2)",
                 pre_act="RReLU", graph_act="RReLU", flat_act="RReLU", graph_res=True):
        super().__init__()
        hid_dim = mol_in_dim * hid_dim_alpha
        self.mol_lin0 = LinearBlock(mol_in_dim, hid_dim, norm=pre_norm, dropout=pre_do, act=pre_act)
        self.mol_conv = MessageBlock(hid_dim, hid_dim, mol_edge_in_dim, norm=graph_norm, dropout=graph_do,
                                     conv=mol_block, act=graph_act, res=graph_res)
        self.message_steps = message_steps
        self.mol_readout = _readout(mol_readout, hid_dim)
        _mol_ro = 5 if mol_readout == "GlobalPool5" else 2
        self.mol_flat = LinearBlock(_mol_ro * hid_dim, e_dim, norm=flat_norm, dropout=flat_do, act=flat_act)
        self.lin_out1 = LinearBlock(e_dim, out_dim, norm=end_norm, dropout=end_do, act="_None")

    def forward(self, data_mol):
        # a batch content seen before is replayed from hipGraphs (glam_amd.graphs.GraphedCallable): the reference's eager training
        # loop (src_1gp/trainer.py:286-304) runs unchanged at graphed speed; ``model.graphed_call = False`` keeps every call eager
        return graphs.graphed_call(self, self._eager_forward, data_mol)

    def _eager_forward(self, data_mol):
        with ops.weight_scope():     # weight re-layouts are shared by the message_steps applications of the block
            out = self._forward(data_mol)
        ops.poll_checks()            # deferred id checks of foreign batches (GLAM_VALIDATE=deferred) whose flag has come back
        return out

    def _forward(self, data_mol):
        m = _Tower(self, "mol", data_mol)
        prestage_pass(m.stage())                                                   # (the pass's weight re-layouts from one launch)
        # (next_dropout: the block behind applies Dropout to this output first — the activation's launch writes the dropped twin)
        # (... and next_node: that block's TripletMessage reads this output — the embedding's launch writes its node product too)
        m.x = self.mol_lin0(data_mol.x, batch=data_mol.batch, next_dropout=following_dropout(self.mol_conv),    # model.py:49
                            next_node=first_node_spec(self.mol_conv, data_mol.x.size(0), data_mol.edge_index, data_mol.edge_attr))
        for i in range(self.message_steps):                                        # model.py:53-54
            with ops.block_feeds_itself(i + 1 < self.message_steps):      # (its output is the same block's next input)
                m.step()
        # model.py:57, 60-61 — in the default configuration in training mode the head applies mol_flat's RReLU and its own Dropout to
        # the elements it reads (layer.flat_then_head)
        return flat_then_head(self.mol_flat, self.lin_out1, m.pooled())


Model = Architecture


class _Tower:
    """One graph tower of one pass — ``model.<name>_lin0 / _conv / _readout / _flat`` over the batch ``data``: ``x`` the rows after the
    last ``step()`` (a fusion that hands them back writes them here), ``n`` the graph count a collated Batch already knows (PyG's pools
    would read it back from ``batch``), else None."""

    def __init__(self, model, name, data):
        self.lin0, self.conv = getattr(model, name + "_lin0"), getattr(model, name + "_conv")
        self.readout, self.flat = getattr(model, name + "_readout"), getattr(model, name + "_flat")
        self.data, self.n, self.x, self.h = data, getattr(data, "num_graphs", None) or None, None, None

    def stage(self):
        return self.lin0, self.conv, self.data.x, self.data.edge_attr

    def step(self):
        """One application of the MessageBlock -> its rows."""
        d = self.data
        self.x, self.h = self.conv(self.x, d.edge_index, d.edge_attr, h=self.h, batch=d.batch)
        return self.x

    def pooled(self):
        return self.readout(self.x, self.data.batch, self.n)

    def flat_out(self):
        return self.flat(self.pooled())


def _embed(*towers):
    """The start of a pass: its weight re-layouts from as few launches as possible (``prestage_pass``, every tower in ONE call), then
    each tower's input LinearBlock, in the order given."""
    prestage_pass(*[t.stage() for t in towers])
    for t in towers:
        t.x = t.lin0(t.data.x, batch=t.data.batch)


def _fused_walk(steps, a, b, b_feeds_itself, fuse):
    """Both towers step by step, and after every step ``fuse(a.x, b.x)`` -> ``(f, a.x, b.x)``, the fusion that hands the rows back (every
    step's outputs feed the fusion AND the next step / the readouts: both gradients then meet inside its backward launch instead of in
    an add launch per tower) -> the steps' ``f``.  ``b_feeds_itself``: ``b``'s block too runs under ``block_feeds_itself``
    (``ArchitectureDDI`` wraps both blocks, ``ArchitectureDTI`` the ligand's alone)."""
    _embed(a, b)
    fusion = []
    for i in range(steps):
        with ops.block_feeds_itself(i + 1 < steps):      # (its output is the same block's next input)
            a.step()
            if b_feeds_itself:
                b.step()
        if not b_feeds_itself:
            b.step()
        f, a.x, b.x = fuse(a.x, b.x)
        fusion.append(f)
    return fusion


def _tower_stamp(modules):
    """Changes whenever a parameter or buffer of ``modules`` is written (version counters; storage addresses for ``.data`` swaps and
    ``.to()``; ``ops.PARAM_EPOCH`` for the optimizers that write through raw pointers)."""
    ts = [t for m in modules for t in list(m.parameters()) + list(m.buffers())]
    return ops.PARAM_EPOCH, sum(t._version for t in ts), tuple(t.data_ptr() for t in ts)


_PER_GRAPH_NORMS = (_None, _BatchNorm, _LayerNorm, _PairNorm)      # slots given ``batch``
_PER_ROW_NORMS = (_None, _BatchNorm)                               # the *_flat slots (no ``batch``)

# What the guards of a model that holds graphs once call its things: ``slots`` (block, admitted norm types) of the towers held once,
# ``thing`` one graph of them, ``call`` the reference call an encoding stands for, ``copy`` / ``fusion`` / ``train`` / ``eager`` the words of the inference
# guard, ``rows`` / ``encode`` / ``written`` those of the encoding check.
def _slots(*towers):
    return tuple((f"{t}_{s}", ok) for t in towers for s, ok in (("lin0", _PER_GRAPH_NORMS), ("conv", _PER_GRAPH_NORMS), ("flat", _PER_ROW_NORMS)))


_DTI_WORDS = dict(slots=_slots("pro"), thing="protein", call="model(data_mol, data_pro)", copy="protein copy", fusion="indexed",
                  train="model(data_mol, data_pro) on one protein graph per pair", eager="a library walk never repeats a batch",
                  rows="residue rows", encode="encode_proteins",
                  written="a protein-side parameter or buffer (pro_lin0 / pro_conv / pro_readout / pro_flat)")
# (forward_panel holds BOTH sides once: every ligand stands for Qs rows of the expanded batch, every protein for L * its entries in sel)
_DTI_PANEL_WORDS = dict(_DTI_WORDS, slots=_slots("mol", "pro"), thing="graph", call="model(M, P) on the expanded batch")
_DDI_WORDS = dict(slots=_slots("mol1", "mol2"), thing="drug", call="model(mol1, mol2)", copy="copy of a drug", fusion="gathered",
                  train="model(mol1, mol2) on one graph per pair and side",
                  eager="its pair index is validated on the host and differs from call to call", rows="rows", encode="encode_drugs",
                  written="a parameter or buffer of a tower (mol1_* / mol2_* lin0, conv, readout, flat)")


def _tower_norms_guard(model, what, w):
    """The norm rules of an encoding that stands for every copy of a graph."""
    for name, ok in w["slots"]:
        norm = getattr(model, name).norm
        if type(norm) not in ok:
            raise GlamHipError(f"{what}: {name}'s norm {type(norm).__name__} is not per graph or per row here — it normalises over "
                               f"the whole batch (rows of every copy of every {w['thing']}), so its result depends on how often each "
                               f"{w['thing']} is repeated and one encoding cannot reproduce {w['call']}")


def _inference_guard(model, what, w):
    """The guard of the calls that make or read an encoding: ``eval()``, no grad, per-graph norms, not under a capture."""
    if model.training:
        raise GlamHipError(f"{what}: the model is in training mode — Dropout / RReLU noise is drawn per {w['copy']} and BatchNorm takes "
                           "statistics over the replicated rows, so one encoding cannot stand for the copies: call model.eval()")
    if torch.is_grad_enabled():
        raise GlamHipError(f"{what} is inference only (the {w['fusion']} fusion has no backward): call it under torch.no_grad(); "
                           f"training runs {w['train']}")
    _tower_norms_guard(model, what, w)
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise GlamHipError(f"{what} runs eagerly ({w['eager']}): not inside a hipGraph capture")


def _shared_guard(model, w, what="forward_shared"):
    """The guard of ``forward_shared`` (and of ``forward_panel``, under its name ``what``): the norms an encoding refuses, and a
    ``_BatchNorm`` in their slots while training."""
    thing, call = w["thing"], w["call"]
    _tower_norms_guard(model, what, w)
    for name, _ in w["slots"] if model.training else ():
        if type(getattr(model, name).norm) is _BatchNorm:
            raise GlamHipError(f"{what}: {name}'s norm _BatchNorm takes its batch statistics over the {thing} rows of the step, "
                               f"and in {call} those weigh each {thing} by how often it is repeated — over {thing}s held once they are "
                               f"other statistics: train with {call}, or call {what} in eval() (running statistics are per row)")


def _check_encoding(model, what, enc, cls, stamp, rows, w):
    """``enc`` is this model's (``cls``) and as fresh as ``stamp``, with one entry of ``rows`` (the attribute) per message step."""
    if not isinstance(enc, cls) or enc.model() is not model:
        raise GlamHipError(f"{what}: the encoding was made by another model (its {w['rows']} are that model's): {w['encode']}() on this one")
    if enc.stamp != stamp or len(getattr(enc, rows)) != model.message_steps:
        raise GlamHipError(f"{what}: the encoding is stale — {w['written']} was written since {w['encode']}(): encode again")


def _head_is_per_row(model):
    """Both norms of the head (``lin_out0`` / ``lin_out1``) are per row in ``eval()``: a pair row's result does not depend on the rows it
    is batched with, so the head may run over the rows of several columns at once (``screen_panel``, ``score_matrix``)."""
    return type(model.lin_out0.norm) in _PER_ROW_NORMS and type(model.lin_out1.norm) in _PER_ROW_NORMS


def _check_head(what, head):
    """The ``head=`` keyword of the table calls: ``"rows"`` (the listed head over pair rows) or ``"factored"`` (``ops.pair_head``)."""
    if head not in ("rows", "factored"):
        raise GlamHipError(f"{what}: head = {head!r} is not \"rows\" (the listed head over the table's pair rows) or \"factored\" "
                           "(ops.pair_head: no [pairs, e_dim] hidden matrix)")
    return head == "factored"


def _head_activation(model, what, route, instead):
    """``(act, slope)`` of the table heads' kernels (``ops.pair_head``, ``ops.pair_head_classes``) for ``model``'s head, or the refusal in
    the words of ``route`` — what the two routes share: both norm slots ``_None``, both dropout slots idle, ``end_act`` elementwise and
    deterministic, ``lin_out1`` ending in its linear layer, the fusion columns within the kernels' registers."""
    from torch.nn import Dropout, LeakyReLU, ReLU, RReLU
    for name in ("lin_out0", "lin_out1"):
        block = getattr(model, name)
        if type(block.norm) is not _None:
            raise GlamHipError(f"{what}: {route} has no norm in the head, {name}'s norm is {type(block.norm).__name__} — its "
                               f"input does not separate into a row part and a column part: {instead}")
        d = block.dropout
        if not (type(d) is _None or (type(d) is Dropout and (not d.training or d.p == 0))):
            raise GlamHipError(f"{what}: {route} needs {name}'s dropout slot idle (_None, or a Dropout in eval()), got "
                               f"{type(d).__name__}: {instead}")
    a = model.lin_out0.act
    if type(a) is _None:
        act = "none", 0.0
    elif type(a) is ReLU:
        act = "relu", 0.0
    elif type(a) is LeakyReLU:
        act = "leaky", float(a.negative_slope)
    elif type(a) is RReLU and not a.training:
        act = "leaky", (float(a.lower) + float(a.upper)) / 2          # eval: the fixed mean slope, as in LinearBlock.forward
    else:
        raise GlamHipError(f"{what}: {route} applies end_act inside its kernel and knows _None, ReLU, LeakyReLU and RReLU (eval), "
                           f"not {type(a).__name__}: {instead}")
    if type(model.lin_out1.act) is not _None:
        raise GlamHipError(f"{what}: {route} ends in lin_out1's linear layer, which here is followed by "
                           f"{type(model.lin_out1.act).__name__}: {instead}")
    if 2 * model.message_steps > ops.HEAD_MAX_F:
        raise GlamHipError(f"{what}: {route} keeps the 2 * message_steps fusion columns of a pair in registers, at most "
                           f"{ops.HEAD_MAX_F}; this model has {2 * model.message_steps}: {instead}")
    return act


def _factored_head(model, what, block_pairs=0):
    """``(act, slope)`` of ``ops.pair_head`` for ``model``'s head (``lin_out0`` / ``lin_out1``), or the refusal of ``head="factored"`` —
    on the host, before the first launch.  The factored head is ``lin_out1.linear(act(lin_out0.linear(.)))``: both norm slots ``_None``,
    both dropout slots idle (``_None``, or a ``Dropout`` in ``eval()``), ``end_act`` elementwise and deterministic, at most 8 task columns,
    and no head blocks (there is no hidden matrix to keep in pieces)."""
    act = _head_activation(model, what, "head=\"factored\"", "use head=\"rows\"")
    out_dim = model.lin_out1.linear.out_features
    if out_dim > ops.HEAD_MAX_OUT:
        raise GlamHipError(f"{what}: head=\"factored\" keeps out_dim accumulators per pair in registers, at most {ops.HEAD_MAX_OUT}; "
                           f"this model has out_dim = {out_dim}: use head=\"rows\"")
    if isinstance(block_pairs, bool) or block_pairs != 0:
        raise GlamHipError(f"{what}: block_pairs = {block_pairs!r} cuts the hidden matrix of head=\"rows\" into blocks; head=\"factored\" has "
                           "no hidden matrix and no blocks: leave block_pairs at 0")
    return act


def _class_head(model, what):
    """``(act, slope)`` of ``ops.pair_head_classes`` for ``model``'s head, or the refusal of the class route (``classify_matrix``,
    ``classify_panel``, ``score="logp"`` of the top calls) — on the host, before the first launch: the checks of ``_factored_head``
    without its limit of 8 task columns, and a head that has classes to choose between."""
    instead = "take the logits from head=\"rows\" and torch.log_softmax / argmax"
    act = _head_activation(model, what, "the class head", instead)
    out_dim = model.lin_out1.linear.out_features
    if not 2 <= out_dim <= ops.HEAD_MAX_CLASSES:
        raise GlamHipError(f"{what}: the class head calls one of 2..{ops.HEAD_MAX_CLASSES} classes; this model has out_dim = {out_dim}"
                           + (" (one column is a score, not a class: score=\"logit\")" if out_dim == 1 else f": {instead}"))
    return act


def _fusion_columns(fusion, R, Cs, like):
    """The steps' ``[R, Cs, 2]`` fusions side by side -> ``[R, Cs, 2 * steps]`` (zeros for an empty table), ``None`` without steps."""
    if not fusion:
        return None
    if R * Cs == 0:
        return like.new_zeros(R, Cs, 2 * len(fusion))
    return ops.cat_cols([t.reshape(R * Cs, 2) for t in fusion]).view(R, Cs, 2 * len(fusion))


def _table_head_factored(model, act, flat_a, flat_b, fusion, R, Cs):
    """``ops.pair_head`` over the table: the two flat matrices as they are, ``f`` = ``_fusion_columns``."""
    return ops.pair_head(flat_a, flat_b, _fusion_columns(fusion, R, Cs, flat_a), model.lin_out0.linear, model.lin_out1.linear, act[0], act[1])


def _table_head_classes(model, act, flat_a, flat_b, fusion, R, Cs, classes, logits):
    """``ops.pair_head_classes`` over the table, on the operands of ``_table_head_factored`` -> ``ops.ClassTable``."""
    return ops.pair_head_classes(flat_a, flat_b, _fusion_columns(fusion, R, Cs, flat_a), model.lin_out0.linear, model.lin_out1.linear,
                                 act[0], act[1], classes, logits)


def _table_rows(a_rows, b_rows, fusion):
    """The head's input over pair rows: ``cat[a_rows, b_rows, fusion_0, ...]``, every step's fusion of those pairs as ``[pairs, 2]``."""
    return ops.cat_cols([a_rows, b_rows] + [f.reshape(a_rows.size(0), 2) for f in fusion])


def _table_head_rows(model, a, b, fusion, R, Cs, per_block):
    """The listed head (``lin_out0`` / ``lin_out1``, inside the caller's weight scope) over the table of ``a`` ``[R, hid]`` against ``b``
    ``[Cs, hid]`` -> ``[R, Cs, out_dim]``.  ``per_block`` > 0 (both head norms per row): over blocks of that many table rows, row
    ``(i - i0) * Cs + j`` of a block = ``cat[a[i], b[j], fusion_0[i, j], ...]``; ONE block that covers the table is returned as the head
    wrote it.  ``per_block`` = 0 (a batch-less norm must see one column ``[R, .]`` at a time): once per column.  Empty: zeros, no head."""
    head = lambda rows: model.lin_out1(model.lin_out0(rows))       # noqa: E731
    if R == 0 or Cs == 0:
        return a.new_zeros(R, Cs, model.lin_out1.linear.out_features)
    if not per_block:
        return torch.stack([head(_table_rows(a, b[j:j + 1].expand(R, -1).contiguous(), [f[:, j].contiguous() for f in fusion]))
                            for j in range(Cs)], 1)
    out = None if per_block >= R else a.new_empty(R, Cs, model.lin_out1.linear.out_features)
    for i0 in range(0, R, per_block):
        n = min(R, i0 + per_block) - i0
        ai, fi = (a, fusion) if n == R else (a[i0:i0 + n], [f[i0:i0 + n] for f in fusion])          # (the whole table: no views)
        block = head(_table_rows(ai.repeat_interleave(Cs, 0), b.repeat(n, 1), fi)).view(n, Cs, -1)
        if out is None:
            return block
        out[i0:i0 + n] = block
    return out


def _table_guard(model, what, enc, head, classes=False, block_pairs=0):
    """What opens a table call, in this order: the inference guard, the encoding, then the head — ``classes``: the class head's checks
    (``_class_head``), else the ``head=`` keyword and with ``"factored"`` its checks -> ``(act, slope)`` of the kernel head, or None."""
    model._encoding_guard(what, enc)
    if classes:
        return _class_head(model, what)
    return _factored_head(model, what, block_pairs) if _check_head(what, head) else None


def _check_score(what, score):
    """The ``score=`` keyword of the top calls: ``"logit"`` (column ``task`` of the head's output) or ``"logp"`` (the log-softmax of class
    ``task``, through the class head); whether it is the latter."""
    if score not in ("logit", "logp"):
        raise GlamHipError(f"{what}: score = {score!r} is not \"logit\" (the raw output column task) or \"logp\" (the log-softmax of class "
                           "task over the model's classes: ops.pair_head_classes)")
    return score == "logp"


def _check_task(what, task, out_dim):
    if isinstance(task, bool) or not isinstance(task, int) or not 0 <= task < out_dim:
        raise GlamHipError(f"{what}: task = {task!r} is not one of the model's {out_dim} task column(s)")


def _top_scores(classify, table, what, args, task, head, logp):
    """``(scores, column)`` of one block of a top call: ``sel[..., 0]`` of the class route under the call's name (the log-softmax of
    class ``task``, merged in place by stride), else column ``task`` of the table call's output."""
    if logp:
        return classify(what, *args, [task], False).sel, 0
    return table(*args, head=head), task


def _shared_index(model, given, P, Q, device, **words):
    """``ops.pair_index`` of ``given``; the default of ``None`` is kept per (P, Q, device): the index a later capture of the same step
    meets already has its device copies.  ``words``: ``pair_index``'s own (``default``, ``name``, ``over``)."""
    if given is not None:
        return ops.pair_index(given, P, Q, **words)
    cache = model.__dict__.setdefault("_shared_defaults", {})
    key = (P, Q, str(device))
    if key not in cache:
        cache[key] = ops.pair_index(None, P, Q, **words)
    return cache[key]


def _host_sizes(enc):
    """``enc.sizes_host``: the row counts of an encoding's segments on the host — ONE read-back of ``sp.ptr`` per encoding, on first use."""
    if enc.sizes_host is None:
        enc.sizes_host = _segment_sizes(enc.sp)
    return enc.sizes_host


def _segment_sizes(sp):
    ptr = sp.ptr.cpu().numpy().astype("int64")          # (the read-back)
    return ptr[1:] - ptr[:-1]


def _cached_plan(plans, make_plan, Q, selection, sizes, bound=None, stale=None):
    """The plan (``make_plan``: ``ops.panel_plan`` / ``ops.grid_plan``) of ``selection`` over ``Q`` segments out of the dict ``plans`` —
    keyed by the validated selection, ``None`` = all in order — or made from ``sizes()`` and kept.  The selection is validated on the
    host first (the sizes play no part in that); ``sizes`` is called after it, only for a plan that is missing or ``stale(plan)``.
    ``bound``: the first-inserted plan leaves when the dict holds that many; ``None`` = unbounded."""
    sel = None if selection is None else make_plan([0] * Q, selection).sel
    key = None if sel is None else tuple(sel.tolist())
    plan = plans.get(key)
    if plan is None or (stale is not None and stale(plan)):
        plan = make_plan(sizes(), sel)
        while bound is not None and key not in plans and len(plans) >= bound:
            plans.pop(next(iter(plans)))
        plans[key] = plan
    return plan


def _step_fusions(steps, return_argmax, fuse):
    """``fuse(step)`` for every step, in order — the step's fusion, or ``(fusion, argmax)`` with ``return_argmax`` -> the two lists."""
    got = [fuse(s) for s in range(steps)]
    return ([f for f, _ in got], [a for _, a in got]) if return_argmax else (got, [])


class ProteinEncoding:
    """What ``ArchitectureDTI.encode_proteins`` keeps of ``Q`` protein graphs for ``screen``: ``rows[s]`` the residue rows after
    message step ``s`` (contiguous, as the fusion reads them), ``sp`` their ``SegmentPtr``, ``flat`` = ``pro_flat(pro_readout(.))``
    ``[Q, hid]``, ``num_graphs`` = Q, and the stamp of the protein-side parameters it was computed from (``model`` is a weak reference).

    What the first ``screen_panel`` call on it adds (``panel()``; ``encode_proteins`` and ``screen`` never touch these): ``sizes_host``, the
    proteins' residue counts on the host — ONE read-back of ``sp.ptr`` per encoding, never per batch; ``prosum[s]`` ``[Q, hid]``, the column
    sums of ``rows[s]`` per protein (the mean column's protein half); ``plans``, a small cache of ``ops.PanelPlan`` keyed by the selection."""

    _MAX_PLANS = 16

    def __init__(self, model, rows, sp, flat, stamp):
        self.model, self.rows, self.sp, self.flat, self.stamp = weakref.ref(model), rows, sp, flat, stamp
        self.num_graphs = sp.B
        self.sizes_host, self.prosum, self.plans = None, None, {}

    def panel(self, proteins=None):
        """``ops.PanelPlan`` of the selection ``proteins`` (``ops.panel_plan``: ``None`` = every protein in order) — from the cache when this
        selection was planned before — after filling ``sizes_host`` (the one read-back) and ``prosum`` (one segment-sum launch per step) if
        this is the encoding's first panel call.  The selection is validated on the host before anything is launched or read back."""
        plan = _cached_plan(self.plans, ops.panel_plan, self.num_graphs, proteins, lambda: _host_sizes(self), self._MAX_PLANS)
        if self.prosum is None:
            self.prosum = [ops.segment_pool(r, self.sp, "sum") for r in self.rows]
        return plan


class ArchitectureDTI(torch.nn.Module):
    """Ligand + protein two-tower model with per-pair fusion (src_2gi_dti_scr/model.py:14-68)."""

    def __init__(self, mol_in_dim=15, pro_in_dim=49, mol_edge_in_dim=4, pro_edge_in_dim=8, hid_dim_alpha=4,
                 e_dim=1024, out_dim=1, mol_block="_NNConv", pro_block="_GCNConv", message_steps=3,
                 mol_readout="GlobalPool5", pro_readout="GlobalPool5",
                 pre_norm="_None", graph_norm="_None", flat_norm="_None", end_norm="_None",
                 pre_do="_None()", graph_do="Dropout(0.2)", flat_do="_None()", end_do="Dropout(0.2)",
                 pre_act="RReLU", graph_act="RReLU", flat_act="RReLU", end_act="RReLU", graph_res=True):
        super().__init__()
        hid_dim = mol_in_dim * hid_dim_alpha
        self.mol_lin0 = LinearBlock(mol_in_dim, hid_dim, norm=pre_norm, dropout=pre_do, act=pre_act)
        self.pro_lin0 = LinearBlock(pro_in_dim, hid_dim, norm=pre_norm, dropout=pre_do, act=pre_act)
        self.mol_conv = MessageBlock(hid_dim, hid_dim, mol_edge_in_dim, norm=graph_norm, dropout=graph_do,
                                     conv=mol_block, act=graph_act, res=graph_res)
        self.pro_conv = MessageBlock(hid_dim, hid_dim, pro_edge_in_dim, norm=graph_norm, dropout=graph_do,
                                     conv=pro_block, act=graph_act, res=graph_res)
        self.message_steps = message_steps
        self.mol_readout = _readout(mol_readout, hid_dim)
        self.pro_readout = _readout(pro_readout, hid_dim)
        _mol_ro = 5 if mol_readout == "GlobalPool5" else 2
        _pro_ro = 5 if pro_readout == "GlobalPool5" else 2
        self.mol_flat = LinearBlock(_mol_ro * hid_dim, hid_dim, norm=flat_norm, dropout=flat_do, act=flat_act)
        self.pro_flat = LinearBlock(_pro_ro * hid_dim, hid_dim, norm=flat_norm, dropout=flat_do, act=flat_act)
        self.lin_out0 = LinearBlock(hid_dim * 2 + message_steps * 2, e_dim, norm=end_norm, dropout=end_do, act=end_act)
        self.lin_out1 = LinearBlock(e_dim, out_dim, norm=end_norm, dropout=end_do, act="_None")

    def forward(self, data_mol, data_pro):
        return graphs.graphed_call(self, self._eager_forward, data_mol, data_pro)      # (see Architecture.forward)

    def _eager_forward(self, data_mol, data_pro):
        with ops.weight_scope():
            return self._forward(data_mol, data_pro)

    def _forward(self, data_mol, data_pro):
        m, p = _Tower(self, "mol", data_mol), _Tower(self, "pro", data_pro)
        fusion = _fused_walk(self.message_steps, m, p, False,
                             lambda xm, xp: dot_and_global_pool2(xm, xp, data_mol.batch, data_pro.batch, with_identity=True))
        # (model.py:74-75; contiguous gradients for every piece from one launch)
        return self.lin_out1(self.lin_out0(ops.cat_cols([m.flat_out(), p.flat_out()] + fusion)))

    # ---- screening: a protein is encoded once, ligand batches stream against it ---------------------------------------------
    # The reference's screening set scores a whole library against ONE protein (src_2gi_dti_scr/dataset.py:297-318) and still
    # collates — and runs the protein tower on — one copy of it per pair.  Until the fusion nothing in the protein tower depends
    # on the ligand, and in eval mode nothing in it depends on the other graphs of the batch, with the exceptions refused below:
    #   slot given ``batch`` (pro_lin0 / pro_conv):  _None, _BatchNorm (running statistics: per row), _LayerNorm and _PairNorm
    #       (per graph) are fine; _GraphSizeNorm DROPS ``batch`` (layer.py:193-194) and scales by the batch's total row count.
    #   pro_flat's slot (no ``batch``):  _None and _BatchNorm are per row; _LayerNorm, _PairNorm and _GraphSizeNorm there take
    #       statistics (or the row count) over the whole [B, .] matrix: how often each protein is repeated changes them.
    def _protein_modules(self):
        return self.pro_lin0, self.pro_conv, self.pro_readout, self.pro_flat

    def _protein_stamp(self):
        """Changes whenever a protein-side parameter or buffer is written (version counters; storage addresses for ``.data`` swaps and
        ``.to()``; ``ops.PARAM_EPOCH`` for the optimizers that write through raw pointers)."""
        return _tower_stamp(self._protein_modules())

    def _screen_guard(self, what):
        _inference_guard(self, what, _DTI_WORDS)

    def _encoding_guard(self, what, enc):
        """The guard of a call that reads ``enc``: ``_screen_guard``, then the encoding is this model's and fresh."""
        self._screen_guard(what)
        _check_encoding(self, what, enc, ProteinEncoding, self._protein_stamp(), "rows", _DTI_WORDS)

    def encode_proteins(self, data_pro):
        """The protein tower, once, over the ``Q`` graphs of ``data_pro`` -> ``ProteinEncoding`` for ``screen``.  ``eval()`` mode under
        ``torch.no_grad()``; valid until a protein-side parameter or buffer changes."""
        self._screen_guard("encode_proteins")
        p = _Tower(self, "pro", data_pro)
        with ops.weight_scope():
            _embed(p)
            # (odd widths flow as [N, C] views of padded rows: compacted here, once)
            rows = [p.step().contiguous() for _ in range(self.message_steps)]
            sp = ops.segment_ptr(data_pro.batch, p.n)
            flat = p.flat_out()
        return ProteinEncoding(self, rows, sp, flat, self._protein_stamp())

    def screen(self, data_mol, enc, pro_of_pair=None, return_argmax=False):
        """``model(data_mol, B_pro)`` -> ``[P, out_dim]`` for ``B_pro`` = the proteins ``pro_of_pair`` of ``enc`` collated one per ligand,
        without building ``B_pro`` or running the protein tower: the ligand tower runs on ``data_mol``, every step's fusion reads the
        encoded residue rows of that step through the pair -> protein index (``ops.pair_pool_indexed``), ``enc.flat`` is gathered by it.
        ``pro_of_pair``: host integers, one per ligand (``ops.pair_index``); ``None`` when ``enc`` holds one protein.
        ``return_argmax``: also the per-step ``[P, 2]`` int32 contacts (row of ``data_mol.x``, row of the encoded proteins)."""
        out, contacts = self._screen("screen", data_mol, enc, pro_of_pair, return_argmax)[:2]
        return (out, contacts) if return_argmax else out

    def _screen(self, what, data_mol, enc, pro_of_pair, return_argmax):
        """``screen`` under the name ``what`` -> ``(out, contacts, fusion, rows, msp, index)``: also the steps' ``[P, 2]`` fusions, the
        ligand rows every step's fusion read (a step writes new rows: the earlier ones stay), the ligands' ``SegmentPtr`` and the
        validated index (``explain.explain_pair``)."""
        self._encoding_guard(what, enc)
        m = _Tower(self, "mol", data_mol)
        msp = ops.segment_ptr(data_mol.batch, m.n)
        index = ops.pair_index(pro_of_pair, msp.B, enc.num_graphs, default="single")       # host-side, before the first launch
        rows = []

        def fuse(x, i):
            rows.append(x)
            return dot_and_global_pool2_indexed(x, enc.rows[i], data_mol.batch, enc.sp, index, return_argmax)

        with ops.weight_scope():
            fusion, contacts = self._ligand_walk(m, return_argmax, fuse)
            outm = m.flat_out()
            outp = enc.flat.index_select(0, index.on(enc.flat.device))
            out = self.lin_out1(self.lin_out0(ops.cat_cols([outm, outp] + fusion)))
        return out, contacts, fusion, rows, msp, index

    def _ligand_walk(self, m, return_argmax, fuse):
        """The ligand tower ``m`` against an encoding: ``fuse(rows, step)`` after every step -> the steps' fusions and contacts."""
        def step_then_fuse(i):
            with ops.block_feeds_itself(i + 1 < self.message_steps):
                m.step()
            return fuse(m.x, i)

        _embed(m)
        return _step_fusions(self.message_steps, return_argmax, step_then_fuse)

    def _panel_head_in_one_pass(self):
        """Whether the head may run once over the ``L * Qs`` rows of a panel: both of its norms are per row in ``eval()`` (``_None``,
        ``_BatchNorm`` on running statistics).  The batch-less ``_LayerNorm`` / ``_PairNorm`` / ``_GraphSizeNorm`` take statistics (or the
        row count) over the whole matrix they are given, so they must see one protein column ``[L, .]`` at a time, as in ``screen``."""
        return _head_is_per_row(self)

    def _panel_walk(self, m, data_mol, enc, plan, return_argmax):
        """The walk of ``screen_panel`` (inside its weight scope): the ligand tower ``m`` step by step with the protein-stationary fusion
        of each step -> ``(fusion, contacts, outm [L, hid], outp [Qs, hid])``."""
        fusion, contacts = self._ligand_walk(m, return_argmax, lambda x, i: dot_and_global_pool2_panel(
            x, enc.rows[i], data_mol.batch, enc.sp, plan, None, enc.prosum[i], return_argmax))
        outm = m.flat_out()
        outp = enc.flat.index_select(0, plan.on(enc.flat.device)[0].long())                   # [Qs, hid]
        return fusion, contacts, outm, outp

    def screen_panel(self, data_mol, enc, proteins=None, return_argmax=False, head="rows"):
        """``[L, Qs, out_dim]``: column ``j`` is ``screen(data_mol, enc, pro_of_pair=[proteins[j]] * L)`` — every ligand of ``data_mol``
        against every protein of the selection — from ONE pass of the ligand tower and one protein-stationary fusion per step
        (``ops.pair_pool_panel`` on ``enc.rows[step]``).  Every step's fusion max and the contacts equal those of the ``screen`` calls
        bit for bit; the output sits within the fp32 parity bound of ``model(data_mol, B_pro)`` on the expanded batch.
        ``proteins``: host integers in ``[0, Q)``, any order, duplicates allowed (``ops.panel_plan``); ``None`` = all ``Q`` in order.
        ``return_argmax``: also the per-step ``[L, Qs, 2]`` int32 contacts (row of ``data_mol.x``, row of the encoded proteins).
        The first call on an encoding reads the proteins' sizes back once and sums their rows per step (``ProteinEncoding.panel``);
        after it, a call on the same encoding and selection does no host synchronisation of its own.
        ``head``: ``"rows"`` is the listed head over the ``L * Qs`` pair rows; ``"factored"`` sends it through ``ops.pair_head`` (no pair
        rows, no ``[L * Qs, e_dim]`` hidden matrix; within the same parity bound, not the bits of ``"rows"``) and is refused — before the
        first launch, with the reason — for a norm in the head, an ``end_act`` other than ``_None`` / ``ReLU`` / ``LeakyReLU`` / ``RReLU``
        and ``out_dim > 8``."""
        act = _table_guard(self, "screen_panel", enc, head)
        plan = enc.panel(proteins)                                 # host-side checks, before the first launch
        m = _Tower(self, "mol", data_mol)
        msp = ops.segment_ptr(data_mol.batch, m.n)
        L, Qs = msp.B, plan.Qs
        with ops.weight_scope():
            fusion, contacts, outm, outp = self._panel_walk(m, data_mol, enc, plan, return_argmax)
            if act and L and Qs:
                out = _table_head_factored(self, act, outm, outp, fusion, L, Qs)
            else:          # ligand-major rows, all in one block: row l * Qs + j = cat[outm[l], flat[sel[j]], fusion_0[l, j], ...]
                out = _table_head_rows(self, outm, outp, fusion, L, Qs, L if self._panel_head_in_one_pass() else 0)
        return (out, contacts) if return_argmax else out

    def classify_panel(self, data_mol, enc, proteins=None, classes=(), return_logits=False):
        """``screen_panel`` read as a classifier -> ``ops.ClassTable(cls, logp, sel, logits)`` over the ``[L, Qs]`` panel: per ligand and
        protein the called class (``torch.argmax`` of the head's output), its log-softmax, and the log-softmax of the classes ``classes``
        names (host ints in ``[0, out_dim)``, at most 8) — for the screening model ``classes=[1]`` and ``sel[..., 0].exp()`` is the
        ligand's probability of class 1.  The walk is ``screen_panel``'s; the head is ``ops.pair_head_classes`` (one side launch, one table
        launch): no pair rows, no hidden matrix and, unless ``return_logits`` asks for it, no ``[L, Qs, out_dim]`` table.  The logits are
        those of ``screen_panel(head="factored")`` bit for bit where that head exists (``out_dim <= 8``).  Refused, before the first
        launch: what ``head="factored"`` refuses in the head except its limit on ``out_dim`` (any of 2..1 024 is taken), and
        ``out_dim = 1``."""
        return self._classify_panel("classify_panel", data_mol, enc, proteins, classes, return_logits)

    def _classify_panel(self, what, data_mol, enc, proteins, classes, return_logits):
        act = _table_guard(self, what, enc, None, classes=True)
        chosen = ops.class_selection(classes, self.lin_out1.linear.out_features, what)
        plan = enc.panel(proteins)                                 # host-side checks, before the first launch
        m = _Tower(self, "mol", data_mol)
        msp = ops.segment_ptr(data_mol.batch, m.n)
        with ops.weight_scope():
            fusion, _, outm, outp = self._panel_walk(m, data_mol, enc, plan, False)
            return _table_head_classes(self, act, outm, outp, fusion, msp.B, plan.Qs, chosen, return_logits)

    def screen_top(self, batches, enc, proteins=None, k=100, task=0, largest=True, head="rows", score="logit"):
        """The best ``k`` ligands per selected protein of a whole library -> ``hits.HitList`` with one query per entry of the selection
        (duplicates allowed, as in ``ops.panel_plan``).  ``batches``: an iterable of ``data_mol`` or ``(data_mol, ids)``; every item goes
        through ``screen_panel(data_mol, enc, proteins)`` — all of its guards and refusals apply, with its own messages — and column
        ``task`` of its output is merged into the lists by stride (``HitList.update``: two launches, no copy).  ``ids``: the ligands' ids,
        host integers or an int32 device tensor; without them a ligand's id is its position in the stream.  Ids are not deduplicated.
        Memory is ``Qs x k`` however long the stream: no score tensor outlives its batch, and the loop adds no read-back to those of
        ``screen_panel`` (one per encoding).  ``k`` in 1..1024; ``largest``: whether a larger score is better.  ``head``: ``screen_panel``'s.
        ``score``: ``"logit"`` ranks by the raw output column ``task`` (the call described above); ``"logp"`` ranks by the log-softmax of class
        ``task`` over the model's classes — what a cross-entropy model's score is: every batch goes through the class head
        (``classify_panel`` with ``classes=[task]``, whose guards apply under this call's name; ``head`` is not consulted) and
        ``sel[..., 0]`` is merged in place."""
        k = hits.check_k(k, "screen_top")
        logp = _check_score("screen_top", score)
        _check_task("screen_top", task, self.lin_out1.linear.out_features)
        top = None
        for item in batches:
            data_mol, ids = item if isinstance(item, tuple) else (item, None)
            out, col = _top_scores(self._classify_panel, self.screen_panel, "screen_top", (data_mol, enc, proteins), task, head, logp)
            if top is None:
                top = hits.HitList(out.size(1), k, out.device, largest)
            top.update(out, ids, col)
        if top is None:          # an empty stream: empty lists, after the checks a first batch would have met
            _table_guard(self, "screen_top" if logp else "screen_panel", enc, head, classes=logp)
            top = hits.HitList(ops.panel_plan([0] * enc.num_graphs, proteins).Qs, k, enc.flat.device, largest)     # (host only: no read-back)
        return top

    # ---- training on shared proteins: the protein tower runs once per DISTINCT protein of the step ----------------------------
    def _shared_index(self, pro_of_pair, P, Q, device):
        return _shared_index(self, pro_of_pair, P, Q, device, default="single" if Q == 1 else "identity")

    def forward_shared(self, data_mol, data_pro, pro_of_pair=None):
        """``model(data_mol, B_pro)`` -> ``[P, out_dim]`` for ``B_pro`` = the proteins ``pro_of_pair`` of ``data_pro`` collated one per
        ligand — without building ``B_pro``: ``data_pro`` holds ``Q`` DISTINCT protein graphs, the protein tower runs on those, every
        step's fusion reads their residue rows through the pair -> protein index (``ops.pair_pool_shared``) and ``pro_flat(pro_readout(.))``
        is gathered by it (``ops.pair_rows``).  Unlike ``screen`` this call has a backward: it trains, with gradients to every parameter
        of both towers and the head; a protein's gradients are the sums over its pairs, in batch order (no atomics: two runs agree bit
        for bit).  ``pro_of_pair``: host integers, one per ligand, or a ``PairIndex`` (``ops.pair_index`` — keep ONE across the steps
        that use it: its device copies are made on the first, eager, visit, and a ``GraphedTrainStep`` capture needs them to exist);
        ``None`` = ligand i with protein i when ``Q == P``, every ligand with the one protein when ``Q == 1``.

        Contract.  Output and every parameter gradient equal those of ``model(data_mol, B_pro)`` within the fp32 parity bound WHENEVER
        nothing on the protein side is stochastic or depends on the rest of the batch: ``eval()``, or ``train()`` with ``_None()`` /
        ``Dropout(0)`` and non-random activations.  In ``train()`` with live Dropout / RReLU on the protein side the noise is drawn ONCE per
        distinct protein and shared by all its pairs; the reference draws it per copy.  That is another (equally valid) regulariser, not
        the reference's — which is why this is a call of its own and ``model(data_mol, data_pro)`` is untouched.  Refused, before any
        launch: the protein-side norms ``encode_proteins`` refuses (``_GraphSizeNorm``; ``_LayerNorm`` / ``_PairNorm`` in ``pro_flat``'s slot),
        and a protein-side ``_BatchNorm`` while training (batch statistics weigh each protein by how often it is repeated).
        Always eager by itself (no graphed-call route); inside a ``GraphedTrainStep`` it is captured with the step."""
        _shared_guard(self, _DTI_WORDS)
        m, p = _Tower(self, "mol", data_mol), _Tower(self, "pro", data_pro)
        index = None
        if m.n is not None and p.n is not None:          # (a collated Batch knows its counts: the index is checked before the first launch)
            index = self._shared_index(pro_of_pair, m.n, p.n, data_mol.x.device)
        msp, psp = ops.segment_ptr(data_mol.batch, m.n), ops.segment_ptr(data_pro.batch, p.n)
        if index is None:
            index = self._shared_index(pro_of_pair, msp.B, psp.B, data_mol.x.device)
        with ops.weight_scope():
            fusion = _fused_walk(self.message_steps, m, p, False,
                                 lambda xm, xp: dot_and_global_pool2_shared(xm, xp, data_mol.batch, psp, index, with_identity=True))
            outm = m.flat_out()
            return self.lin_out1(self.lin_out0(ops.cat_cols([outm, ops.pair_rows(p.flat_out(), index)] + fusion)))

    # ---- training on a label table: both towers run once, the fusion is the panel's ------------------------------------------
    def _panel_plan(self, data_pro, psp, proteins):
        """The ``ops.PanelPlan`` of ``proteins`` over the graphs of ``data_pro``, kept ON the batch object (per selection): the first
        call reads the proteins' sizes back once, a later step — or a capture — on the same batch finds the plan and its device copies."""
        cache = data_pro.__dict__.setdefault("_glam_panel_plans", {"sizes": None, "plans": {}})

        def sizes():          # (kept with the plans, and read again when the batch no longer holds what they say)
            if cache["sizes"] is None or len(cache["sizes"]) != psp.B or int(cache["sizes"].sum()) != psp.N:
                cache["sizes"] = _segment_sizes(psp)
            return cache["sizes"]

        return _cached_plan(cache["plans"], ops.panel_plan, psp.B, proteins, sizes, stale=lambda plan: plan.Q != psp.B or plan.N != psp.N)

    def forward_panel(self, data_mol, data_pro, proteins=None, plan=None):
        """``model(M, P)`` as a table -> ``[L, Qs, out_dim]``: entry ``[l, j]`` is row ``l * Qs + j`` of the expanded batch ``M`` = ligand
        ``l`` of ``data_mol`` repeated ``Qs`` times, ``P`` = the proteins ``sel`` of ``data_pro`` tiled ``L`` times — without building
        either: ``data_pro`` holds ``Q`` DISTINCT protein graphs, BOTH towers run once (``L`` ligand graphs, ``Q`` protein graphs), every
        step's fusion is the protein-stationary panel with a backward (``ops.pair_pool_panel_shared``), and the head runs over the
        ``L * Qs`` ligand-major rows ``cat[mol_flat[l], pro_flat[sel[j]], fusion...]``, both flat matrices expanded by ``ops.pair_rows``.
        It trains: gradients to every parameter of both towers and the head; a ligand's gradients are the sums over its ``Qs`` pairs, a
        protein's over every pair that names it, in the batch order of the expanded pair list (no atomics: two runs agree bit for bit).
        ``proteins``: host integers in ``[0, Q)``, any order, duplicates allowed (``ops.panel_plan``); ``None`` = all ``Q`` in order.
        ``plan``: the ``ops.PanelPlan`` of the selection over the proteins' sizes, kept by the caller across the steps that use it
        (``proteins`` is then left ``None``); without one the proteins' sizes are read back once and the plan is kept on ``data_pro``.
        Either way its device copies are made on the first, eager, visit, and a ``GraphedTrainStep`` capture needs them to exist.

        Contract.  Output and every parameter gradient equal those of ``model(M, P)`` within the fp32 parity bound WHENEVER nothing in
        a tower is stochastic or depends on the rest of the batch: ``eval()``, or ``train()`` with ``_None()`` / ``Dropout(0)`` and
        non-random activations.  In ``train()`` with live Dropout / RReLU in a tower the noise is drawn ONCE per ligand and ONCE per
        protein and shared by all their pairs; the reference draws it per copy.  That is another (equally valid) regulariser, not the
        reference's — which is why this is a call of its own and ``model(data_mol, data_pro)`` is untouched.  Refused, before any
        launch, on EITHER tower: ``_GraphSizeNorm``; ``_LayerNorm`` / ``_PairNorm`` in a ``*_flat`` slot; a ``_BatchNorm`` while training
        (batch statistics weigh each graph by how often it is repeated); and a ``plan`` made for other sizes.  The head's norms are not
        refused: the head sees exactly the expanded rows.  Always eager by itself (no graphed-call route); inside a
        ``GraphedTrainStep`` it is captured with the step."""
        _shared_guard(self, _DTI_PANEL_WORDS, "forward_panel")
        m, p = _Tower(self, "mol", data_mol), _Tower(self, "pro", data_pro)
        if plan is not None:
            ops._require_plan("forward_panel", plan, ops.PanelPlan, "panel_plan")
            if proteins is not None:
                raise GlamHipError("forward_panel: pass the selection (proteins) or the plan made from it, not both")
            if (p.n is not None and plan.Q != p.n) or plan.N != data_pro.x.size(0):
                raise GlamHipError(f"forward_panel: the plan was made for {plan.Q} proteins of {plan.N} residue rows, data_pro holds "
                                   f"{p.n if p.n is not None else '?'} of {data_pro.x.size(0)}")
        msp, psp = ops.segment_ptr(data_mol.batch, m.n), ops.segment_ptr(data_pro.batch, p.n)
        if plan is None:
            plan = self._panel_plan(data_pro, psp, proteins)
        L, Qs = msp.B, plan.Qs
        lig, col = plan.row_index(L)
        with ops.weight_scope():
            fusion = _fused_walk(self.message_steps, m, p, False, lambda xm, xp: dot_and_global_pool2_panel_shared(
                xm, xp, data_mol.batch, psp, plan, with_identity=True))
            outm, outp = m.flat_out(), p.flat_out()
            if L == 0 or Qs == 0:
                return outm.new_zeros(L, Qs, self.lin_out1.linear.out_features)
            # ligand-major rows: row l * Qs + j = cat[mol_flat[l], pro_flat[sel[j]], fusion_0[l, j], ...]
            return self.lin_out1(self.lin_out0(_table_rows(ops.pair_rows(outm, lig), ops.pair_rows(outp, col), fusion))).view(L, Qs, -1)


class DrugEncoding:
    """What ``ArchitectureDDI.encode_drugs`` keeps of ``Q`` molecule graphs for ``score_pairs``: ``rows1[s]`` / ``rows2[s]`` the rows of
    tower 1 / tower 2 after message step ``s`` (contiguous, as the fusion reads them), ``sp`` their one ``SegmentPtr``, ``flat1`` /
    ``flat2`` = ``molK_flat(molK_readout(.))`` ``[Q, hid]``, ``num_graphs`` = Q, and the stamp of the tower parameters it was computed
    from (``model`` is a weak reference).

    What the first ``score_matrix`` call on it adds (``grid()``; ``encode_drugs`` and ``score_pairs`` never touch these): ``sizes_host``, the
    drugs' row counts on the host — ONE read-back of ``sp.ptr`` per encoding; ``sum1[s]`` / ``sum2[s]`` ``[Q, hid]``, the column sums of
    ``rows1[s]`` / ``rows2[s]`` per drug (the two halves of the mean column: one segment-sum launch per step and tower); ``plans``, a small
    cache of ``ops.GridPlan`` keyed by the column selection."""

    _MAX_PLANS = 16

    def __init__(self, model, rows1, rows2, sp, flat1, flat2, stamp):
        self.model, self.rows1, self.rows2, self.sp = weakref.ref(model), rows1, rows2, sp
        self.flat1, self.flat2, self.stamp = flat1, flat2, stamp
        self.num_graphs = sp.B
        self.sizes_host, self.sum1, self.sum2, self.plans = None, None, None, {}

    def grid(self, cols=None):
        """``ops.GridPlan`` of the column selection ``cols`` (``ops.grid_plan``: ``None`` = every drug in order) — from the cache when this
        selection was planned before — after filling ``sizes_host`` (the one read-back) and ``sum1`` / ``sum2`` if this is the encoding's
        first matrix call.  The selection is validated on the host before anything is launched or read back."""
        plan = _cached_plan(self.plans, ops.grid_plan, self.num_graphs, cols, lambda: _host_sizes(self), self._MAX_PLANS)
        if self.sum1 is None:
            self.sum1 = [ops.segment_pool(r, self.sp, "sum") for r in self.rows1]
            self.sum2 = [ops.segment_pool(r, self.sp, "sum") for r in self.rows2]
        return plan


class ArchitectureDDI(torch.nn.Module):
    """Two-drug model: two ligand towers with their own parameters and per-pair fusion (src_2gi_ddi/model.py:9-62; checkpoint keys
    ``mol1_lin0.*``, ``mol2_lin0.*``, ``mol1_conv.*``, ``mol2_conv.*``, ``mol1_readout.*``, ``mol2_readout.*``, ``mol1_flat.*``,
    ``mol2_flat.*``, ``lin_out0.*``, ``lin_out1.*``; parameter creation order = the reference's, so seeded inits agree)."""

    def __init__(self, mol_in_dim=15, mol_edge_in_dim=4, hid_dim_alpha=4, e_dim=1024, out_dim=1, mol_block="_NNConv", message_steps=3,
                 mol_readout="GlobalPool5",
                 pre_norm="_None", graph_norm="_None", flat_norm="_None", end_norm="_None",
                 pre_do="_None()", graph_do="Dropout(0.2)", flat_do="_None()", end_do="Dropout(0.2)",
                 pre_act="RReLU", graph_act="RReLU", flat_act="RReLU", end_act="RReLU", graph_res=True):
        super().__init__()
        hid_dim = mol_in_dim * hid_dim_alpha
        self.mol1_lin0 = LinearBlock(mol_in_dim, hid_dim, norm=pre_norm, dropout=pre_do, act=pre_act)
        self.mol2_lin0 = LinearBlock(mol_in_dim, hid_dim, norm=pre_norm, dropout=pre_do, act=pre_act)
        self.mol1_conv = MessageBlock(hid_dim, hid_dim, mol_edge_in_dim, norm=graph_norm, dropout=graph_do, conv=mol_block,
                                      act=graph_act, res=graph_res)
        self.mol2_conv = MessageBlock(hid_dim, hid_dim, mol_edge_in_dim, norm=graph_norm, dropout=graph_do, conv=mol_block,
                                      act=graph_act, res=graph_res)
        self.message_steps = message_steps
        self.mol1_readout = _readout(mol_readout, hid_dim)
        self.mol2_readout = _readout(mol_readout, hid_dim)
        _mol_ro = 5 if mol_readout == "GlobalPool5" else 2
        self.mol1_flat = LinearBlock(_mol_ro * hid_dim, hid_dim, norm=flat_norm, dropout=flat_do, act=flat_act)
        self.mol2_flat = LinearBlock(_mol_ro * hid_dim, hid_dim, norm=flat_norm, dropout=flat_do, act=flat_act)
        self.lin_out0 = LinearBlock(hid_dim * 2 + message_steps * 2, e_dim, norm=end_norm, dropout=end_do, act=end_act)
        self.lin_out1 = LinearBlock(e_dim, out_dim, norm=end_norm, dropout=end_do, act="_None")

    def forward(self, mol1, mol2):
        return graphs.graphed_call(self, self._eager_forward, mol1, mol2)              # (see Architecture.forward)

    def _eager_forward(self, mol1, mol2):
        with ops.weight_scope():
            return self._forward(mol1, mol2)

    def _forward(self, mol1, mol2):
        t1, t2 = _Tower(self, "mol1", mol1), _Tower(self, "mol2", mol2)
        fusion = _fused_walk(self.message_steps, t1, t2, True,
                             lambda x1, x2: dot_and_global_pool2(x1, x2, mol1.batch, mol2.batch, with_identity=True))
        return self.lin_out1(self.lin_out0(ops.cat_cols([t1.flat_out(), t2.flat_out()] + fusion)))

    # ---- pair scoring: every drug is encoded once, a pair is two indices -----------------------------------------------------
    # The reference builds its pairs by looking both drugs up in one dictionary of molecule graphs (src_2gi_ddi/dataset.py:170-176) and
    # runs both towers on every copy.  Nothing in either tower depends on the partner drug: dot_and_global_pool2 reads both towers'
    # rows after each step and hands two scalars per pair to the head (src_2gi_ddi/model.py:47-59).  In eval mode nothing in a tower
    # depends on the other graphs of the batch either, with the exceptions of ``ArchitectureDTI._screen_guard`` — applied here to BOTH
    # towers.  The head's norms (``end_norm``) see the same [P, .] matrix as ``model(mol1, mol2)`` would: nothing is refused there.
    def _drug_modules(self):
        return (self.mol1_lin0, self.mol2_lin0, self.mol1_conv, self.mol2_conv, self.mol1_readout, self.mol2_readout, self.mol1_flat,
                self.mol2_flat)

    def _drug_stamp(self):
        """Changes whenever a parameter or buffer of either tower (lin0, conv, readout, flat) is written; the head is not part of it."""
        return _tower_stamp(self._drug_modules())

    def _pairs_guard(self, what):
        _inference_guard(self, what, _DDI_WORDS)

    def _encoding_guard(self, what, enc):
        """The guard of a call that reads ``enc``: ``_pairs_guard``, then the encoding is this model's and fresh."""
        self._pairs_guard(what)
        _check_encoding(self, what, enc, DrugEncoding, self._drug_stamp(), "rows1", _DDI_WORDS)

    def encode_drugs(self, data):
        """Both towers, once, over the ``Q`` graphs of ``data`` -> ``DrugEncoding`` for ``score_pairs``.  ``eval()`` mode under
        ``torch.no_grad()``; valid until a parameter or buffer of either tower changes."""
        self._pairs_guard("encode_drugs")
        t1, t2 = _Tower(self, "mol1", data), _Tower(self, "mol2", data)
        with ops.weight_scope():
            _embed(t1, t2)
            rows1, rows2 = [], []
            for i in range(self.message_steps):
                with ops.block_feeds_itself(i + 1 < self.message_steps):      # (the routes of _forward: the rows are its rows bit for bit)
                    t1.step()
                    t2.step()
                rows1.append(t1.x.contiguous())       # (odd widths flow as [N, C] views of padded rows: compacted here, once)
                rows2.append(t2.x.contiguous())
            sp = ops.segment_ptr(data.batch, t1.n)
            flat1, flat2 = t1.flat_out(), t2.flat_out()
        return DrugEncoding(self, rows1, rows2, sp, flat1, flat2, self._drug_stamp())

    def score_pairs(self, enc, first, second, return_argmax=False):
        """``model(B1, B2)`` -> ``[P, out_dim]`` for ``B1`` = the drugs ``first`` and ``B2`` = the drugs ``second`` of ``enc``, collated one
        per pair — without building either batch or running a tower: every step's fusion reads the encoded rows of that step through both
        indices (``ops.pair_pool_gather``), the two ``flat`` matrices are gathered by them, then the head.  ``first`` / ``second``: host
        integers in ``[0, enc.num_graphs)``, one per pair (``ops.pair_index``).  The head's norms take their statistics over the ``P``
        pairs of THIS call, as ``model(B1, B2)`` does over its batch: the equality holds per call, for the P pairs of that call (with
        ``end_norm="_LayerNorm"`` a chunk scored alone differs from the same pairs scored inside a longer call).
        ``return_argmax``: also the per-step ``[P, 2]`` int32 contacts (row of ``enc.rows1[s]``, row of ``enc.rows2[s]``)."""
        out, contacts, _, _, _ = self._score_pairs("score_pairs", enc, first, second, return_argmax)
        return (out, contacts) if return_argmax else out

    def _score_pairs(self, what, enc, first, second, return_argmax):
        """``score_pairs`` under the name ``what`` -> ``(out, contacts, fusion, i1, i2)``: the steps' ``[P, 2]`` fusions and the two validated
        indices kept (``explain.explain_pair``)."""
        self._encoding_guard(what, enc)
        Q = enc.num_graphs
        P = ops.pair_count(first)
        i1 = ops.pair_index(first, P, Q, name="first", over="drugs")               # host-side, before the first launch
        i2 = ops.pair_index(second, P, Q, name="second", over="drugs")
        fusion, contacts = _step_fusions(self.message_steps, return_argmax, lambda s: dot_and_global_pool2_gather(
            enc.rows1[s], enc.rows2[s], enc.sp, enc.sp, i1, i2, return_argmax))
        dev = enc.flat1.device
        o1 = enc.flat1.index_select(0, i1.on(dev))
        o2 = enc.flat2.index_select(0, i2.on(dev))
        with ops.weight_scope():
            out = self.lin_out1(self.lin_out0(ops.cat_cols([o1, o2] + fusion)))
        return out, contacts, fusion, i1, i2

    # ---- the whole table: every selected drug (tower 1) against every selected drug (tower 2) ---------------------------------
    # The head's hidden matrix is [pairs, e_dim]: at 2 000 x 2 000 drugs and e_dim = 1 024 it would be 16 GB in one piece.  The head
    # therefore runs over blocks of consecutive row drugs whose hidden matrix stays under this cap — a design choice (room for the
    # block's input, hidden and output beside a resident encoding on any device this runs on), NOT a measurement.
    _MATRIX_BLOCK_BYTES = 512 << 20

    def _matrix_head_in_one_pass(self):
        """Whether the head may run over rows of SEVERAL column drugs at once: both of its norms are per row in ``eval()`` (the condition of
        ``ArchitectureDTI._panel_head_in_one_pass``).  A batch-less ``_LayerNorm`` / ``_PairNorm`` / ``_GraphSizeNorm`` must see one column
        ``[R, .]`` at a time: that is the ``[P, .]`` matrix of ``score_pairs(enc, rows, [cols[j]] * R)``."""
        return _head_is_per_row(self)

    def _matrix_block_rows(self, block_pairs, R, Cs):
        """Row drugs per head block: at most ``block_pairs`` pair rows, or with 0 the largest whole number whose hidden matrix
        ``rows * Cs * e_dim * 4`` bytes stays within ``_MATRIX_BLOCK_BYTES``; at least one row drug."""
        if isinstance(block_pairs, bool) or not isinstance(block_pairs, int) or block_pairs < 0:
            raise GlamHipError(f"score_matrix: block_pairs = {block_pairs!r} must be 0 (choose) or the pair rows per head block")
        if block_pairs == 0:
            block_pairs = self._MATRIX_BLOCK_BYTES // (4 * self.lin_out0.linear.out_features)
        return max(1, min(R, block_pairs // max(Cs, 1)))

    @staticmethod
    def _matrix_selection(enc, rows, cols):
        """``(R, Cs, index, sel)`` of a table's ``rows`` / ``cols`` — host-side, before the first launch and before the read-back."""
        Q = enc.num_graphs
        R = ops.pair_count(rows, None, Q)
        index = None if rows is None else ops.pair_index(rows, R, Q, name="rows", over="drugs")
        sel = None if cols is None else ops.grid_plan([0] * Q, cols).sel
        return R, (Q if sel is None else int(sel.shape[0])), index, sel

    def _matrix_walk(self, enc, index, sel, return_argmax):
        """The fusion walk of ``score_matrix``: one second-side-stationary fusion per step over the whole table ->
        ``(fusion, contacts, o1 [R, hid], o2 [Cs, hid])``."""
        plan = enc.grid(sel)
        fusion, contacts = _step_fusions(self.message_steps, return_argmax, lambda s: dot_and_global_pool2_grid(
            enc.rows1[s], enc.rows2[s], enc.sp, enc.sp, plan, index, enc.sum1[s], enc.sum2[s], return_argmax))
        dev = enc.flat1.device
        o1 = enc.flat1 if index is None else enc.flat1.index_select(0, index.on(dev))              # [R, hid]
        o2 = enc.flat2.index_select(0, plan.on(dev)[0])                                            # [Cs, hid]
        return fusion, contacts, o1, o2

    def score_matrix(self, enc, rows=None, cols=None, return_argmax=False, block_pairs=0, head="rows"):
        """``[R, Cs, out_dim]``: entry ``[i, j]`` is ``score_pairs(enc, [rows[i]], [cols[j]])`` — tower 1 for the row drug, tower 2 for the
        column drug, so the matrix is not symmetric — from one second-side-stationary fusion per step over the whole table
        (``ops.pair_pool_grid`` on ``enc.rows1[step]`` / ``enc.rows2[step]``: several small drugs share the lanes of a wave) instead of
        ``R * Cs`` listed pairs.  Every step's fusion max and the contacts equal those of ``score_pairs`` bit for bit; the output sits
        within the fp32 parity bound of ``model(B1, B2)`` on the expanded batches.  ``rows`` / ``cols``: host integers in ``[0, Q)``, any
        order, duplicates allowed (``ops.pair_index`` / ``ops.grid_plan``); ``None`` = all ``Q`` in order.  With per-row head norms
        (``_None``, ``_BatchNorm``) the head runs over blocks of consecutive row drugs of at most ``block_pairs`` pair rows each (0 = as
        many row drugs as keep the block's hidden matrix within 512 MiB; at least one): the ``[R * Cs, e_dim]`` matrix is never built in
        one piece.  With a batch-less norm in the head it runs once per column on ``[R, .]`` — what ``score_pairs(enc, rows, [cols[j]] *
        R)`` computes.  ``return_argmax``: also the per-step ``[R, Cs, 2]`` int32 contacts (row of ``enc.rows1[s]``, row of
        ``enc.rows2[s]``).  The first call on an encoding reads the drugs' sizes back once and sums their rows per step and tower
        (``DrugEncoding.grid``); after it, a call on the same encoding and column selection does no host synchronisation of its own.
        ``head``: ``"rows"`` is the head described above; ``"factored"`` sends it through ``ops.pair_head`` — the first linear layer as a row
        part + a column part + the fusion columns' part, so neither the pair rows nor the hidden matrix exist and an entry's bits do not
        depend on the selection around it; within the same parity bound, not the bits of ``"rows"``.  It is refused — before the first
        launch, with the reason — for a norm in the head, an ``end_act`` other than ``_None`` / ``ReLU`` / ``LeakyReLU`` / ``RReLU``,
        ``out_dim > 8`` and ``block_pairs != 0`` (it has no blocks)."""
        act = _table_guard(self, "score_matrix", enc, head, block_pairs=block_pairs)
        R, Cs, index, sel = self._matrix_selection(enc, rows, cols)
        per_block = None if act else self._matrix_block_rows(block_pairs, R, Cs)
        fusion, contacts, o1, o2 = self._matrix_walk(enc, index, sel, return_argmax)
        with ops.weight_scope():
            if act and R and Cs:
                out = _table_head_factored(self, act, o1, o2, fusion, R, Cs)
            else:          # row-major pair rows: row (i - i0) * Cs + j of a block = cat[flat1[rows[i]], flat2[cols[j]], fusion_0[i, j], ...]
                out = _table_head_rows(self, o1, o2, fusion, R, Cs, per_block if self._matrix_head_in_one_pass() else 0)
        return (out, contacts) if return_argmax else out

    def classify_matrix(self, enc, rows=None, cols=None, classes=(), return_logits=False):
        """``score_matrix`` read as a classifier -> ``ops.ClassTable(cls, logp, sel, logits)`` over the ``[R, Cs]`` table: per pair of drugs
        the called class (``torch.argmax`` of the head's output — the interaction type), its log-softmax (how sure), and the log-softmax
        of the classes ``classes`` names (host ints in ``[0, out_dim)``, at most 8, duplicates allowed, order kept).  The fusion walk is
        ``score_matrix``'s; the head is ``ops.pair_head_classes`` (one side launch, one table launch): no pair rows, no ``[pairs, e_dim]``
        hidden matrix and, unless ``return_logits`` asks for it, no ``[R, Cs, out_dim]`` table — for ANY ``out_dim`` in 2..1 024.  An entry's
        results do not depend on the selection around it; its logits are those of ``score_matrix(head="factored")`` bit for bit where
        that head exists (``out_dim <= 8``).  Refused, before the first launch: what ``head="factored"`` refuses in the head except its
        limit on ``out_dim``, and ``out_dim = 1``."""
        return self._classify_matrix("classify_matrix", enc, rows, cols, classes, return_logits)

    def _classify_matrix(self, what, enc, rows, cols, classes, return_logits):
        act = _table_guard(self, what, enc, None, classes=True)
        chosen = ops.class_selection(classes, self.lin_out1.linear.out_features, what)
        R, Cs, index, sel = self._matrix_selection(enc, rows, cols)
        fusion, _, o1, o2 = self._matrix_walk(enc, index, sel, False)
        with ops.weight_scope():
            return _table_head_classes(self, act, o1, o2, fusion, R, Cs, chosen, return_logits)

    # ---- partner lists: the best row drugs per column drug, without the table -------------------------------------------------
    # Pair rows per block of row drugs when the caller leaves the choice (block_rows = 0): 2^22 — a design choice (a block's scores and
    # fusion columns stay in the tens of MiB whatever the library's size, and a block is still thousands of waves), NOT a measurement.
    _TOP_BLOCK_PAIRS = 1 << 22

    def matrix_top(self, enc, rows=None, cols=None, k=100, task=0, largest=True, block_rows=0, head="factored", score="logit"):
        """The best ``k`` row drugs (tower 1) for every selected column drug (tower 2) -> ``hits.HitList`` with one query per entry of
        ``cols`` (duplicates allowed) — without the ``[R, Cs]`` table ever existing.  ``rows`` is walked in blocks of ``block_rows`` row drugs
        (0 = as many as keep a block within ``2^22`` pair rows, at least one); every block goes through ``score_matrix(enc, block, cols,
        head=head)`` — all of its guards and refusals apply, with its own messages — and column ``task`` of its output is merged into the
        lists (``HitList.update``: two launches, no copy) under the ids of the block's drugs, so a drug that ``rows`` names twice can hold two
        slots.  With ``head="factored"`` an entry's bits do not depend on the block it is scored in: the lists are those of the whole
        table.  Memory is ``Cs x k`` plus one block however long ``rows`` is.  ``k`` in 1..1024; ``largest``: whether a larger score is
        better.  An empty ``rows`` gives empty lists, after the checks a first block would have met.
        ``score``: ``"logit"`` ranks by the raw output column ``task`` (the call described above); ``"logp"`` ranks by the log-softmax of class
        ``task`` over the model's classes — what a cross-entropy model's score is: every block goes through the class head
        (``classify_matrix`` with ``classes=[task]``, whose guards apply under this call's name; ``head`` is not consulted) and
        ``sel[..., 0]`` is merged in place.  Its entries do not depend on the block either."""
        k = hits.check_k(k, "matrix_top")
        logp = _check_score("matrix_top", score)
        _check_task("matrix_top", task, self.lin_out1.linear.out_features)
        if isinstance(block_rows, bool) or not isinstance(block_rows, int) or block_rows < 0:
            raise GlamHipError(f"matrix_top: block_rows = {block_rows!r} must be 0 (choose) or the row drugs per block")
        what = "matrix_top" if logp else "score_matrix"
        _table_guard(self, what, enc, head, classes=logp)
        R, Cs, index, sel = self._matrix_selection(enc, rows, cols)                              # host-side, before the first launch
        ids = ops.host_index(index or ops.pair_index(None, R, R), "matrix_top",                  # (rows=None: every drug in order)
                             "rows as the host integers that were loaded into it")
        per_block = block_rows or max(1, min(R, self._TOP_BLOCK_PAIRS // max(Cs, 1)))
        top = hits.HitList(Cs, k, enc.flat1.device, largest)
        for i0 in range(0, R, per_block):
            block = ids[i0:i0 + per_block]
            out, col = _top_scores(self._classify_matrix, self.score_matrix, what, (enc, block, sel), task, head, logp)
            top.update(out, block, col)
        return top

    # ---- training on shared drugs: each tower runs once per DISTINCT drug of its side of the step ----------------------------
    def _shared_index(self, given, P, Q, device, name):
        return _shared_index(self, given, P, Q, device, name=name, over="drugs")

    def forward_shared(self, mol1, mol2, first=None, second=None):
        """``model(B1, B2)`` -> ``[P, out_dim]`` for ``B1`` = the drugs ``first`` of ``mol1`` and ``B2`` = the drugs ``second`` of ``mol2``
        collated one per pair — without building either batch: ``mol1`` holds the ``Q1`` DISTINCT first-side drugs of the step, ``mol2`` the
        ``Q2`` distinct second-side drugs (the same ``Batch`` may be passed for both), tower 1 runs on ``mol1`` and tower 2 on ``mol2``, each
        once, every step's fusion reads both towers' rows through the two indices (``ops.pair_pool_gather_shared``) and
        ``mol1_flat(mol1_readout(.))`` / ``mol2_flat(mol2_readout(.))`` are gathered by them (``ops.pair_rows``).  Unlike ``score_pairs`` this
        call has a backward: it trains, with gradients to every parameter of both towers and the head; a drug's gradients are the sums
        over its pairs, in batch order (no atomics: two runs agree bit for bit).  ``first`` / ``second``: host integers, one per pair, or a
        ``PairIndex`` (``ops.pair_index`` — keep ONE per side across the steps that use it: its device copies are made on the first, eager,
        visit, and a ``GraphedTrainStep`` capture needs them to exist); ``None`` = pair i takes drug i of that side (needs ``Q == P``).

        Contract.  Output and every parameter gradient equal those of ``model(B1, B2)`` within the fp32 parity bound WHENEVER nothing in
        a tower is stochastic or depends on the rest of the batch: ``eval()``, or ``train()`` with ``_None()`` / ``Dropout(0)`` and
        non-random activations.  In ``train()`` with live Dropout / RReLU in a tower the noise is drawn ONCE per distinct drug and shared
        by all its pairs; the reference draws it per copy.  That is another (equally valid) regulariser, not the reference's — which is
        why this is a call of its own and ``model(mol1, mol2)`` is untouched.  Refused, before any launch: the tower norms ``encode_drugs``
        refuses, on BOTH towers (``_GraphSizeNorm``; ``_LayerNorm`` / ``_PairNorm`` in a ``molK_flat`` slot), and a ``_BatchNorm`` in a
        tower slot while training (batch statistics weigh each drug by how often it is repeated).  The head's norms are not refused: they
        see the same ``[P, .]`` matrix.  Always eager by itself (no graphed-call route); inside a ``GraphedTrainStep`` it is captured with
        the step."""
        _shared_guard(self, _DDI_WORDS)
        t1, t2 = _Tower(self, "mol1", mol1), _Tower(self, "mol2", mol2)
        n1, n2, P, dev = t1.n, t2.n, ops.pair_count(first, second), mol1.x.device
        i1 = i2 = None
        if n1 is not None and n2 is not None:          # (a collated Batch knows its counts: the indices are checked before the first launch)
            P = n1 if P is None else P
            i1, i2 = self._shared_index(first, P, n1, dev, "first"), self._shared_index(second, P, n2, dev, "second")
        sp1, sp2 = ops.segment_ptr(mol1.batch, n1), ops.segment_ptr(mol2.batch, n2)
        if i1 is None:
            P = sp1.B if P is None else P
            i1, i2 = self._shared_index(first, P, sp1.B, dev, "first"), self._shared_index(second, P, sp2.B, dev, "second")
        with ops.weight_scope():
            fusion = _fused_walk(self.message_steps, t1, t2, True,
                                 lambda x1, x2: dot_and_global_pool2_gather_shared(x1, x2, sp1, sp2, i1, i2, with_identity=True))
            o1 = ops.pair_rows(t1.flat_out(), i1)
            o2 = ops.pair_rows(t2.flat_out(), i2)
            return self.lin_out1(self.lin_out0(ops.cat_cols([o1, o2] + fusion)))


class SharedStep(torch.nn.Module):
    """``forward(batch)`` = ``model.forward_shared`` on a resident pair batch (``glam_amd.data.ResidentPairs.dti_batch`` / ``ddi_batch``):
    what a ``GraphedTrainStep`` calls as its model, so that an epoch of shuffled pairs is one captured step replayed — DTI:
    ``forward_shared(batch.mol, batch.pro, batch.index)``, DDI: ``forward_shared(batch.mol1, batch.mol2, batch.first, batch.second)``.
    ``model`` is a submodule: parameters and checkpoint keys sit under the one prefix ``model.``."""

    def __init__(self, model):
        super().__init__()
        if not isinstance(model, (ArchitectureDTI, ArchitectureDDI)):
            raise GlamHipError(f"SharedStep wraps a model with forward_shared (ArchitectureDTI / ArchitectureDDI), got {type(model).__name__}")
        self.model = model

    def forward(self, batch):
        if isinstance(self.model, ArchitectureDTI):
            return self.model.forward_shared(batch.mol, batch.pro, batch.index)
        return self.model.forward_shared(batch.mol1, batch.mol2, batch.first, batch.second)
