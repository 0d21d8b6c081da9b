"""NNConv over continuous edge features (csrc/nnconv_ec.hip), host side: the C ABI additions and the algebra the kernels rest on."""
import os
import re

import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib
from glam_amd.data import synth_protein_batch
from tests.conftest import ROOT, assert_close

NEW = ["glam_nnconv_ec_supported", "glam_nnconv_ec_workspace_bytes", "glam_nnconv_ec_stack", "glam_nnconv_ec_unstack",
       "glam_nnconv_ec_fwd", "glam_nnconv_ec_bwd"]


def test_new_symbols_are_declared_and_bound_without_an_abi_bump():
    header = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define GLAM_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4


@pytest.mark.parametrize("C", [15, 30, 32, 45, 60, 90])
@pytest.mark.parametrize("De", [1, 4, 8, 16])
def test_supported_shapes(C, De):
    assert _lib.load().glam_nnconv_ec_supported(De, 32, C, C) == 1


@pytest.mark.parametrize("De,hidden,Cin,Cout", [(8, 16, 60, 60), (8, 64, 60, 60), (17, 32, 60, 60), (0, 32, 60, 60),
                                                (8, 32, 97, 60), (8, 32, 60, 128), (8, 32, 0, 60)])
def test_unsupported_shapes(De, hidden, Cin, Cout):
    lib = _lib.load()
    assert lib.glam_nnconv_ec_supported(De, hidden, Cin, Cout) == 0
    if hidden == 32:          # (the workspace query has no hidden width: the edge network's width is fixed at 32)
        assert lib.glam_nnconv_ec_workspace_bytes(100, 600, De, Cin, Cout, 1) == 0


def test_workspace_holds_the_slot_buffer():
    lib = _lib.load()
    N, Cin = 1000, 60
    fwd, bwd = lib.glam_nnconv_ec_workspace_bytes(N, 6 * N, 8, Cin, Cin, 0), lib.glam_nnconv_ec_workspace_bytes(N, 6 * N, 8, Cin, Cin, 1)
    assert fwd == N * 34 * Cin * 4 and bwd > fwd


def _wstack(w1, b1, root):
    """The kernels' stacked weight, rows k*Cin + ci: W1[ci*Cout + co, k] (k < 32), b1 (k = 32), root (k = 33)."""
    Cin, Cout = root.shape
    A = w1.view(Cin, Cout, 32).permute(2, 0, 1)                       # A_k[ci, co]
    return torch.cat([A, b1.view(1, Cin, Cout), root.view(1, Cin, Cout)], 0).reshape(34 * Cin, Cout)


@pytest.mark.parametrize("C,De,mean", [(15, 8, True), (30, 4, False), (45, 8, True)])
def test_factorised_formula_matches_the_per_edge_weights_in_fp64(C, De, mean):
    """out = [S | x] @ Wstack + bias reproduces NNConv with per-edge weights nn(e) (the oracle), in fp64, incl. zero in-degree."""
    torch.manual_seed(3)
    b = synth_protein_batch(2, seed=5, n_min=20, n_max=40)
    N, E = b.x.size(0), b.edge_index.size(1)
    ei = b.edge_index[:, 3:]                                           # drop a few edges: some nodes may lose all in-edges
    ea = torch.rand(ei.size(1), De, dtype=torch.float64)
    x = torch.randn(N, C, dtype=torch.float64)
    w0, b0 = torch.randn(32, De, dtype=torch.float64), torch.randn(32, dtype=torch.float64)
    w1, b1 = torch.randn(C * C, 32, dtype=torch.float64) * 0.1, torch.randn(C * C, dtype=torch.float64) * 0.1
    root, bias = torch.randn(C, C, dtype=torch.float64), torch.randn(C, dtype=torch.float64)
    src, dst = ei[0], ei[1]
    h = torch.relu(ea @ w0.t() + b0)
    h1 = torch.cat([h, torch.ones(h.size(0), 1, dtype=torch.float64)], 1)                  # [E, 33]
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.numel(), dtype=torch.float64))
    msg = h1.unsqueeze(2) * x[src].unsqueeze(1)                                             # [E, 33, C]
    S = torch.zeros(N, 33, C, dtype=torch.float64).index_add_(0, dst, msg)
    if mean:
        S = S / deg.clamp(min=1).view(N, 1, 1)
    Sx = torch.cat([S, x.unsqueeze(1)], 1).reshape(N, 34 * C)
    got = Sx @ _wstack(w1, b1, root) + bias
    if mean:
        ref = O.nnconv_mean(x, ei, ea, w0, b0, w1, b1, root, bias)
    else:
        w_e = (torch.relu(ea @ w0.t() + b0) @ w1.t() + b1).view(-1, C, C)
        ref = torch.zeros(N, C, dtype=torch.float64).index_add_(0, dst, torch.bmm(x[src].unsqueeze(1), w_e).squeeze(1)) + x @ root + bias
    assert_close(got, ref, 1e-10, "factorised NNConv")
    assert E > ei.size(1)
