"""CPU: the host side of the attention export (``glam_amd.explain``) — its three C-ABI entry points are declared, bound and checked
like every other, they reject what they do not cover before any launch, ``explain()`` refuses CPU tensors and training-mode models,
and ``Explanation``'s views work on plain tensors."""
import ctypes
import os
import re

import pytest
import torch

from glam_amd import _lib, explain, layer, model
from glam_amd.data import synth_batch
from tests.conftest import ROOT

NAMES = ("glam_edge_attention", "glam_edge_attention_sent", "glam_segment_softmax")


def test_entry_points_are_declared_bound_and_checked():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glam_hip.h")).read(), flags=re.S)
    api, raw = _lib.api(), _lib.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), f"{n} is not declared in include/glam_hip.h"
        assert n in _lib.SIGNATURES and _lib.SIGNATURES[n][0] is ctypes.c_int
        assert n not in _lib.VALUE_RETURNS
        assert getattr(api, n).errcheck is not None and getattr(raw, n).errcheck is None
    assert raw.glam_abi_version() == _lib.ABI_VERSION == 4          # three entry points MORE: no exported signature changed
    assert "attn_export.hip" in open(os.path.join(ROOT, "glam_amd", "csrc", "Makefile")).read()


def test_abi_rejects_what_it_does_not_cover_and_accepts_empty_problems_without_a_launch():
    lib = _lib.load()
    U = _lib.GLAM_E_UNSUPPORTED
    assert lib.glam_edge_attention(None, None, None, None, None, None, 10, 10, 5, 4, 0.2, None, None) == U        # heads > 4
    assert lib.glam_edge_attention(None, None, None, None, None, None, 10, 10, 0, 4, 0.2, None, None) == U
    assert lib.glam_edge_attention(None, None, None, None, None, None, 10, 10, 3, 5, 0.2, None, None) == U        # De not in {4, 8}
    assert b"De=5" in lib.glam_last_error()
    assert lib.glam_edge_attention(None, None, None, None, None, None, 10, 10, 3, 4, 0.2, None, None) == _lib.GLAM_E_INVALID   # null pointers
    assert lib.glam_edge_attention(None, None, None, None, None, None, 0, 0, 3, 4, 0.2, None, None) == 0
    assert lib.glam_edge_attention(None, None, None, None, None, None, 10, 0, 3, 8, 0.2, None, None) == 0         # E == 0: nothing to write
    assert lib.glam_edge_attention(None, None, None, None, None, None, -1, 0, 3, 4, 0.2, None, None) == _lib.GLAM_E_INVALID
    assert lib.glam_edge_attention_sent(None, None, None, 0, 0, 3, None, None) == 0
    assert lib.glam_edge_attention_sent(None, None, None, 10, 0, 3, None, None) == 0                            # E == 0 with N > 0: no launch
    assert lib.glam_edge_attention_sent(None, None, None, 10, 10, 5, None, None) == U
    assert lib.glam_edge_attention_sent(None, None, None, 10, 10, 3, None, None) == _lib.GLAM_E_INVALID
    assert lib.glam_segment_softmax(None, None, None, None, 0, 3, 16, 16, None, None) == 0
    assert lib.glam_segment_softmax(None, None, None, None, 10, 0, 16, 16, None, None) == 0
    for D, ld in ((130, 132), (15, 15), (17, 16), (0, 16)):           # the shapes of glam_s2s_attn_fwd: ld % 4 == 0, ld <= 128, D <= ld
        assert lib.glam_segment_softmax(None, None, None, None, 10, 2, D, ld, None, None) == U, (D, ld)
    assert lib.glam_segment_softmax(None, None, None, None, 10, 2, 15, 16, None, None) == _lib.GLAM_E_INVALID     # covered shape, null pointers
    with pytest.raises(_lib.GlamHipError, match=r"^glam_segment_softmax failed \(code -2\)"):
        _lib.api().glam_segment_softmax(None, None, None, None, 10, 2, 130, 132, None, None)


def test_explain_refuses_cpu_batches_training_mode_and_other_models():
    b = synth_batch(3, seed=1)
    m = model.Architecture(mol_block="_TripletMessage", mol_readout="GlobalLAPool", hid_dim_alpha=1, e_dim=32)
    with pytest.raises(_lib.GlamHipError, match="training mode"):
        explain.explain(m, b)
    m.eval()
    with pytest.raises(_lib.GlamHipError, match="CPU tensor"):
        explain.explain(m, b)
    assert not m.mol_conv.conv.conv._forward_pre_hooks and not m.mol_readout._forward_pre_hooks
    with pytest.raises(_lib.GlamHipError, match="Architecture"):
        explain.explain(model.ArchitectureDDI(hid_dim_alpha=1, e_dim=32).eval(), b)


def test_modules_without_attention_raise():
    b = synth_batch(2, seed=2)
    x = torch.randn(b.x.size(0), 16)
    for conv in (layer._NNConv(16, 16, 4), layer._GCNConv(16, 16, 4), layer.GCNConv(16, 16)):
        with pytest.raises(_lib.GlamHipError, match="no attention weights"):
            explain.conv_attention(conv, x, b.edge_index, b.edge_attr)
    with pytest.raises(_lib.GlamHipError, match="no attention weights"):
        explain.readout_attention(layer.GlobalPool5(), x, b.batch)
    with pytest.raises(_lib.GlamHipError, match="CPU tensor"):           # a conv WITH attention: the usual refusal of CPU tensors
        explain.conv_attention(layer.TripletMessage(16, 4), x, b.edge_index, b.edge_attr)
    with pytest.raises(_lib.GlamHipError, match="CPU tensor"):
        explain.readout_attention(layer.GlobalLAPool(16), x, b.batch)
    with pytest.raises(_lib.GlamHipError, match="CPU tensor"):
        explain.edge_attention(torch.zeros(3, 8), torch.zeros(0, 4), torch.zeros(4, 4), None, 3)


def _hand_made():
    # two molecules of 3 and 2 atoms; edges given out of molecule order on purpose (a GATConv list ends with its self loops)
    ei = torch.tensor([[0, 3, 1, 4, 2, 0], [1, 4, 0, 3, 1, 2]])
    hidden = torch.arange(20, dtype=torch.float32).view(5, 4)
    alpha = torch.tensor([[1.0], [1.0], [1.0], [1.0], [0.0], [1.0]])
    sent = torch.tensor([[2.0, 0.0], [1.0, 1.0], [0.0, 0.5], [1.0, 0.0], [1.0, 2.0]])
    return explain.Explanation(out=torch.zeros(2, 1), hidden=hidden, edge_index=ei, edge_attention=[alpha], atom_sent=[sent],
                               readout_attention=None, ptr=torch.tensor([0, 3, 5], dtype=torch.int32))


def test_explanation_weights():
    ex = _hand_made()
    assert torch.equal(ex.weights("hidden_node"), ex.hidden.mean(-1)) and torch.equal(ex.weights(), ex.weights("hidden_node"))
    assert torch.equal(ex.weights("edge_attention"), torch.tensor([1.0, 1.0, 0.25, 0.5, 1.5]))
    for content in ("lapool_attention", "set2set_attention", "something_else"):
        with pytest.raises(ValueError):
            ex.weights(content)
    ex.readout_attention = torch.tensor([0.2, 0.3, 0.5, 0.4, 0.6])
    assert ex.weights("lapool_attention") is ex.readout_attention
    with pytest.raises(ValueError):
        ex.weights("set2set_attention")
    ex.readout_attention = torch.stack([torch.zeros(5), torch.tensor([0.2, 0.3, 0.5, 0.4, 0.6])])
    assert torch.equal(ex.weights("set2set_attention"), ex.readout_attention[1])
    ex.atom_sent = [None]
    with pytest.raises(ValueError):
        ex.weights("edge_attention")


def test_explanation_per_molecule():
    ex = _hand_made()
    nodes = ex.per_molecule(ex.hidden)
    assert [t.shape for t in nodes] == [(3, 4), (2, 4)] and torch.equal(torch.cat(nodes), ex.hidden)
    per_atom = ex.per_molecule(ex.weights("hidden_node"))
    assert [t.tolist() for t in per_atom] == [[1.5, 5.5, 9.5], [13.5, 17.5]]
    tag = torch.arange(6)
    edges = ex.per_molecule(tag)                         # 6 edges, 5 nodes: inferred as per edge; an edge goes with its target's molecule
    assert [t.tolist() for t in edges] == [[0, 2, 4, 5], [1, 3]]
    assert [t.tolist() for t in ex.per_molecule(ex.edge_index.t(), per="edge")[1]] == [[3, 4], [4, 3]]
    with pytest.raises(ValueError):
        ex.per_molecule(torch.zeros(7))
    with pytest.raises(ValueError):
        ex.per_molecule(torch.zeros(6), per="node")


def test_subclasses_of_the_attention_convs_are_recognised():
    class MyTriplet(layer.TripletMessage):
        pass

    b = synth_batch(2, seed=2)
    with pytest.raises(_lib.GlamHipError, match="CPU tensor"):           # recognised as a conv with attention: refused for the device only
        explain.conv_attention(MyTriplet(16, 4), torch.randn(b.x.size(0), 16), b.edge_index, b.edge_attr)


def test_separable_attention_weights_by_head_group():
    """``TripletMessage._attention_weights(h0, h1)`` on every group of four is the slice of the all-heads algebra, and is what
    ``_staged_weights`` stages; the logits it gives are those of the concatenated form (src_1gp/layer.py:48-49)."""
    torch.manual_seed(0)
    conv = layer.TripletMessage(12, 3, heads=6).double()
    C, H, De = 12, 6, 3
    x, ea = torch.randn(5, C, dtype=torch.float64), torch.randn(5, De, dtype=torch.float64)
    xw, ew = (x @ conv.weight_node).view(5, H, C), (ea @ conv.weight_edge).view(5, H, C)
    att = conv.weight_triplet_att[0]
    for h0 in (0, 4):
        h1 = min(h0 + 4, H)
        Wa, M = conv._attention_weights(h0, h1)
        assert Wa.shape == (C, 8) and M.shape == (4, 4)
        a = x @ Wa
        k = h1 - h0
        assert torch.allclose(a[:, :k], (xw[:, h0:h1] * att[h0:h1, :C]).sum(-1), atol=1e-12)
        assert torch.allclose(a[:, 4:4 + k], (xw[:, h0:h1] * att[h0:h1, 2 * C:]).sum(-1), atol=1e-12)
        assert torch.allclose((ea @ M[:De])[:, :k], (ew[:, h0:h1] * att[h0:h1, C:2 * C]).sum(-1), atol=1e-12)
        assert bool((Wa[:, k:4] == 0).all()) and bool((Wa[:, 4 + k:] == 0).all()) and bool((M[:, k:] == 0).all()) and bool((M[De:] == 0).all())
    small = layer.TripletMessage(12, 3)
    staged = small._staged_weights()
    Wa, M = small._attention_weights(0, 3)
    assert torch.equal(staged[1], Wa) and torch.equal(staged[3], M)
    light = layer.TripletMessageLight(12, 3).double()
    Wa, M = light._attention_weights()
    att, xw = light.weight_triplet_att[0], x @ light.weight_node
    a = x @ Wa
    assert torch.allclose(a[:, 0], xw @ att[:C], atol=1e-12) and torch.allclose(a[:, 4], xw @ att[C + De:], atol=1e-12)
    assert torch.allclose((ea @ M[:De])[:, 0], ea @ att[C:C + De], atol=1e-12)
