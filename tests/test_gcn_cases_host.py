"""The numpy restatement of csrc/gcn.hip (tests/gcn_cases.py) against ``oracle.glam_oracle.gcn_conv`` and its autograd, on every case
the GPU test runs; six subtly wrong variants must FAIL that test's bound (``assert_fp32_parity``, k = 8, forward 1e-5); the cases hold
what their docstrings say.  No GPU."""
import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from tests import gcn_cases as G
from tests.conftest import assert_fp32_parity


def _oracle(xw, cot, ei):
    """``gcn_conv`` with an identity weight and a zero bias IS the aggregation (fp64: the product with I is exact)."""
    x = xw.double().requires_grad_(True)
    D = x.size(1)
    out = O.gcn_conv(x, ei, torch.eye(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64))
    (d,) = torch.autograd.grad((out * cot.double()).sum(), [x])
    return out.detach(), d


@pytest.mark.parametrize("case", ["main", "single"])
@pytest.mark.parametrize("D", G.WIDTHS)
def test_restatement_equals_the_oracle_and_its_autograd(case, D):
    ei, N = G.cases()[case]
    xw, cot = G.inputs(N, D)
    out, (d_xw,) = G.run_ref(xw, cot, ei, torch.float64)
    o_ref, d_ref = _oracle(xw, cot, ei)
    assert float((out - o_ref).abs().max()) <= 1e-13 * max(1.0, float(o_ref.abs().max()))
    assert float((d_xw - d_ref).abs().max()) <= 1e-13 * max(1.0, float(d_ref.abs().max()))


@pytest.mark.parametrize("name", sorted(G.WRONG))
def test_wrong_variants_fail_the_gpu_bound(name):
    ei, N = G.main_case()
    xw, cot = G.inputs(N, 60)
    o32, _ = G.run_ref(xw, cot, ei, torch.float32)
    o64, _ = G.run_ref(xw, cot, ei, torch.float64)
    assert_fp32_parity(o32, o64, o32, "the fp32 restatement itself", out_tol=1e-5)          # (the bound admits a right answer)
    bad = torch.from_numpy(G.gcn_ref(xw.numpy(), ei.numpy(), np.float64, **dict(G.WRONG[name])))
    with pytest.raises(AssertionError):
        assert_fp32_parity(bad, o64, o32, name, out_tol=1e-5)


def test_at_least_six_wrong_variants():
    assert len(G.WRONG) >= 6


def test_main_case_holds_what_it_says():
    ei, N = G.main_case()
    src, dst = ei.numpy()
    real = src != dst
    indeg = np.bincount(dst[real], minlength=N)
    alldeg = np.bincount(dst, minlength=N)
    assert indeg[0] == 0 and alldeg[0] == 0 and not (src == 0).any()                          # isolated
    assert indeg[1] == 0 and alldeg[1] == 1                                                   # only in-edge: a self-loop
    assert indeg[2] == 1 and not ((src == 2) & (dst == 1)).any()                              # in-degree 1, one-way
    assert [int(indeg[n]) for n in (3, 4, 5, 6)] == [63, 64, 65, 300]
    assert [int(indeg[n]) for n in range(20, 28)] == [15, 16, 17, 31, 32, 33, 47, 48]
    assert alldeg[7] - indeg[7] == 200 and indeg[7] == 3 and int(((src == 8) & (dst == 7)).sum()) == 2      # the run, a duplicate
    at7 = np.flatnonzero(dst == 7)
    assert int(at7[-1] - at7[0]) == at7.size - 1                                              # consecutive in the list
    pairs, counts = np.unique(np.stack([src[real], dst[real]]), axis=1, return_counts=True)
    assert int(counts.max()) >= 2


def test_single_case():
    ei, N = G.single_case()
    xw, cot = G.inputs(N, 4)
    out, (d,) = G.run_ref(xw, cot, ei, torch.float64)
    assert torch.equal(out, xw.double()) and torch.equal(d, cot.double())                     # an isolated node returns xw[i]
