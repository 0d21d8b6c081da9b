"""CPU: keeps the per-graph bound of tests/graph_norm_cases.py honest without a GPU.

The GPU tests hold every graph of a launch within ``8 * max(noise_g, 4 ulp)`` of the fp64 oracle, ``noise_g`` being the fp32 oracle's
own error on that graph.  That is only meaningful if an INDEPENDENT correct fp32 evaluation of the same inputs sits well inside it.  For
every (size list, D, setting) the GPU file uses, a second fp32 sample of the oracle — the rows of each graph in reversed order, so that
every segment sum runs the other way — must sit within half the bound, for the output and for the input gradient.  This is a condition
on the inputs, not a measurement of a kernel: a new D or size list passes here before it is used on the GPU."""
import pytest
import torch

from tests import graph_norm_cases as C

HALF = 0.5


def _reversed_sample(sizes_name, D, setting, identity=False):
    x, cot, cot_id = C.inputs(sizes_name, D)
    sizes = C.SIZE_LISTS[sizes_name]
    perm = C.reverse_rows(sizes)
    y, dx = C.run_oracle(setting, sizes, x[perm], cot[perm], torch.float32, cot_id[perm] if identity else None)
    return y[perm], dx[perm]                                   # the permutation is its own inverse


def test_reverse_rows_is_an_involution_inside_each_graph():
    sizes = [0, 3, 1, 0, 4]
    perm = C.reverse_rows(sizes)
    assert perm.tolist() == [2, 1, 0, 3, 7, 6, 5, 4]
    assert torch.equal(perm[perm], torch.arange(8))
    assert torch.equal(C.batch_of(sizes)[perm], C.batch_of(sizes))


def test_the_bound_is_taken_per_graph():
    """An error that one max-norm over the tensor would pass (it is small beside the large graph's magnitude) fails the graph it sits in;
    the failure names that graph."""
    sizes = [1, 0, 400]
    batch = C.batch_of(sizes)
    ref = torch.randn(401, 8, dtype=torch.float64) * torch.where(batch == 0, 1e-3, 1e3).view(-1, 1)
    ref32 = ref.float()
    got = ref32.clone()
    C.assert_per_graph_parity(got, ref, ref32, sizes, "clean")
    got[0, 3] += 1e-4                                          # 10 % of the 1-row graph's values, 1e-7 of the tensor's scale
    assert (got.double() - ref).abs().max() <= 8 * 4 * C.EPS32 * ref.abs().max()      # the whole-tensor rule lets it through
    with pytest.raises(AssertionError, match=r"worst graph 0 \(1 rows\)"):
        C.assert_per_graph_parity(got, ref, ref32, sizes, "one wrong 1-row graph")
    got = ref32.clone()
    got[5, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"worst graph 2 \(400 rows\)"):
        C.assert_per_graph_parity(got, ref, ref32, sizes, "nan")


@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("sizes_name,D", C.ALL_CASES)
def test_a_second_fp32_sample_sits_within_half_the_bound(sizes_name, D, setting):
    sizes = C.SIZE_LISTS[sizes_name]
    ref = C.reference(sizes_name, D, setting)
    y, dx = _reversed_sample(sizes_name, D, setting)
    what = f"{sizes_name} D={D} {C.setting_id(setting)} reversed rows"
    C.assert_per_graph_parity(y, ref[torch.float64][0], ref[torch.float32][0], sizes, what + " out", cap=HALF)
    C.assert_per_graph_parity(dx, ref[torch.float64][1], ref[torch.float32][1], sizes, what + " grad.x", cap=HALF)
    if sizes_name.startswith("ZERO"):                          # the all-zero graph: output exactly 0 in both modes and precisions
        zero = C.batch_of(sizes) == 1
        for dt in (torch.float64, torch.float32):
            assert (ref[dt][0][zero] == 0).all()
        assert (y[zero] == 0).all()
    if setting[0] == "pair":                                   # a 1-row graph under PairNorm: x' = 0, so y = 0 and dx = 0
        one = torch.tensor(sizes)[C.batch_of(sizes)] == 1
        for dt in (torch.float64, torch.float32):
            assert (ref[dt][0][one] == 0).all() and (ref[dt][1][one] == 0).all()


@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("sizes_name,D", C.IDENTITY_CASES)
def test_identity_path_second_sample(sizes_name, D, setting):
    """The same condition for the gradient with the identity output's cotangent added (the addend of glam_graph_norm_bwd_add)."""
    sizes = C.SIZE_LISTS[sizes_name]
    ref = C.reference(sizes_name, D, setting, True)
    _, dx = _reversed_sample(sizes_name, D, setting, True)
    C.assert_per_graph_parity(dx, ref[torch.float64][1], ref[torch.float32][1], sizes,
                              f"{sizes_name} D={D} {C.setting_id(setting)} identity grad.x", cap=HALF)
