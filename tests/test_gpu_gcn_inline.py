"""csrc/gcn.hip on the GPU: ``ops.gcn_aggregate`` forward and backward against the numpy restatement of tests/gcn_cases.py inside the
fp64-twin bound (``assert_twin_parity``, k = 8, forward 1e-5) on every case and width; ``layer.GCNConv`` on a marked edge list against the
oracle and against the same module on an unmarked copy; two runs of every launch bit-equal; which kernel ran is read back from
``_lib.kernel_timer().records()``; the unmarked route launches what it launched before."""
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, layer, ops
from tests import gcn_cases as G
from tests.conftest import assert_twin_parity

pytestmark = pytest.mark.gpu

K_BLOCK = 256


def _labels(records):
    return [r[0] for r in records]


def _gcn_launches(records):
    return [(r[0], r[1]) for r in records if r[0].startswith("k_gcn")]


def _layouts(xw, layout):
    """``xw`` on the device as the layout asks: contiguous, rows off a 16-byte boundary, or rows of a wider buffer."""
    N, D = xw.shape
    if layout == "unaligned":
        buf = torch.empty(N * D + 1, device=xw.device)
        v = buf[1:].view(N, D)
        assert v.data_ptr() % 16 == 4
    elif layout == "wide":
        v = torch.zeros(N, D + 4, device=xw.device)[:, :D]
    else:
        return xw.clone()
    v.copy_(xw)
    return v


def _check(device, case, D, layout="plain"):
    ei, N = G.cases()[case]
    xw0, cot = G.inputs(N, D)
    ei_d = ei.to(device)
    gi = ops.GraphIndex(ei_d, N)
    gi.transpose()
    runs = []
    for _ in range(2):
        xw = _layouts(xw0.to(device), layout).requires_grad_(True)
        with _lib.kernel_timer() as kt:
            out = ops.gcn_aggregate(xw, gi)
            (d_xw,) = torch.autograd.grad((out * cot.to(device)).sum(), [xw])
            torch.cuda.synchronize()
        runs.append((out.detach(), d_xw, kt.records()))
    (o1, d1, _), (o2, d2, rec) = runs
    assert torch.equal(o1, o2) and torch.equal(d1, d2), "two runs differ"
    assert_twin_parity(lambda dt: G.run_ref(xw0, cot, ei, dt), o1, [d1], f"gcn {case} D={D} {layout}", ["xw"])
    grid = -(-N // (K_BLOCK // (16 if D <= 64 else 32)))
    assert _gcn_launches(rec) == [("k_gcn_scale", -(-N // 16)), ("k_gcn_fwd", grid), ("k_gcn_bwd", grid)], rec
    assert all(us > 0 for _n, _g, us in rec)
    return o1


@pytest.mark.parametrize("case", ["main", "single"])
@pytest.mark.parametrize("D", G.WIDTHS)
def test_aggregate_against_the_restatement(device, case, D):
    _check(device, case, D)


@pytest.mark.parametrize("layout", ["unaligned", "wide"])
def test_rows_off_the_16_byte_path_and_rows_of_a_wider_buffer(device, layout):
    """D = 60 on rows that start 4 bytes off a 16-byte boundary (the scalar path) and on the first 60 columns of 64-float rows (the
    16-byte path with ld != D): the same numbers as the contiguous rows within the bound, each against the restatement."""
    _check(device, "main", 60, layout)


def _conv_run(conv, x0, ei_d, cot, device, identity):
    x = x0.to(device).requires_grad_(True)
    with _lib.kernel_timer() as kt, ops.weight_scope():
        if identity:
            out, ident = conv.forward_with_identity(x, ei_d)
            loss = (out * cot.to(device)).sum() + ident.sum()
        else:
            out = conv(x, ei_d)
            loss = (out * cot.to(device)).sum()
        # (forward_with_identity leaves the bias to the caller: no gradient reaches it)
        gs = list(torch.autograd.grad(loss, [x, conv.weight] + ([] if identity else [conv.bias])))
        torch.cuda.synchronize()
    return out.detach(), gs, kt.records()


@pytest.mark.parametrize("C", [60, 30])
@pytest.mark.parametrize("identity", [False, True])
def test_gcnconv_marked_against_unmarked_and_the_oracle(device, C, identity):
    """``layer.GCNConv(C, C)`` on the main case: the marked edge list takes the inline route (``k_gcn_*`` launches, no derived edge list on
    the index), the unmarked copy takes the cached route with the launches it had (``k_edge_wsum*``, no ``k_gcn_*``); both sit inside the
    fp64-twin bound of ``oracle.gcn_conv``; two marked runs are bit-equal."""
    ei, N = G.main_case()
    torch.manual_seed(3)
    conv = layer.GCNConv(C, C)
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5)
    x0, cot = torch.randn(N, C), torch.randn(N, C)
    params = [p.detach().clone() for p in conv.parameters()]

    def run(dt):
        leaves = [x0.to(dt).requires_grad_(True)] + [p.to(dt).requires_grad_(True) for p in params]
        out = O.gcn_conv(leaves[0], ei, leaves[1], torch.zeros_like(leaves[2]) if identity else leaves[2])
        loss = (out * cot.to(dt)).sum() + (leaves[0].sum() if identity else 0)
        return out.detach(), list(torch.autograd.grad(loss, leaves[:2] if identity else leaves))

    conv = conv.to(device)
    marked, plain = ops.mark_gcn_inline(ei.to(device)), ei.to(device)
    names = ["x", "weight", "bias"]
    o_m, g_m, rec_m = _conv_run(conv, x0, marked, cot, device, identity)
    o_m2, g_m2, _ = _conv_run(conv, x0, marked, cot, device, identity)
    assert torch.equal(o_m, o_m2) and all(torch.equal(a, b) for a, b in zip(g_m, g_m2)), "two marked runs differ"
    o_p, g_p, _ = _conv_run(conv, x0, plain, cot, device, identity)
    o_p2, g_p2, rec_p = _conv_run(conv, x0, plain, cot, device, identity)
    assert torch.equal(o_p, o_p2)
    for what, o, g in (("marked", o_m, g_m), ("unmarked", o_p, g_p)):
        assert_twin_parity(run, o, g, f"GCNConv({C}) {what}", names)
    assert [n for n, _ in _gcn_launches(rec_m)] == ["k_gcn_scale", "k_gcn_fwd", "k_gcn_bwd"], rec_m
    assert not any(n.startswith("k_edge_wsum") for n in _labels(rec_m))
    assert "_derived" not in ops.graph_index(marked, N).__dict__                    # nothing derived from the content is kept
    lp = _labels(rec_p)
    assert not _gcn_launches(rec_p) and sum(n.startswith("k_edge_wsum") for n in lp) == 2, lp
    assert "_derived" in ops.graph_index(plain, N).__dict__


def test_edge_weights_keep_the_cached_route(device):
    """A marked edge list with ``edge_weight`` given takes today's route: the closed form holds for unit weights only."""
    ei, N = G.main_case()
    torch.manual_seed(4)
    conv = layer.GCNConv(8, 8).to(device)
    marked = ops.mark_gcn_inline(ei.to(device))
    with _lib.kernel_timer() as kt:
        conv(torch.randn(N, 8, device=device), marked, edge_weight=torch.rand(ei.size(1), device=device))
        torch.cuda.synchronize()
    assert not _gcn_launches(kt.records())


def test_scale_once_per_edge_list_and_pass(device):
    """Inside one ``ops.weight_scope`` two applications on one edge list compute ``dis`` once; the next scope computes it again."""
    ei, N = G.main_case()
    torch.manual_seed(5)
    conv = layer.GCNConv(60, 60).to(device)
    marked = ops.mark_gcn_inline(ei.to(device))
    x = torch.randn(N, 60, device=device)
    conv(x, marked)
    for _ in range(2):
        with _lib.kernel_timer() as kt, ops.weight_scope():
            conv(conv(x, marked), marked)
            torch.cuda.synchronize()
        names = [n for n, _ in _gcn_launches(kt.records())]
        assert names.count("k_gcn_scale") == 1 and names.count("k_gcn_fwd") == 2, names
