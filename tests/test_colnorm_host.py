"""CPU: the column norms' host side — C ABI symbols, the ops, CPU tensors on the unchanged torch route, checkpoint
keys, and the premise of the offset-column GPU test (a float32 sum-of-squares variance misses the bound the centred oracle sets)."""
import copy
import os

import torch

from glam_amd import _lib, layer, model, ops
from tests.conftest import ROOT, assert_fp32_parity

SYMBOLS = ["glam_colnorm_workspace_bytes", "glam_batch_norm_fwd", "glam_batch_norm_eval_fwd", "glam_batch_norm_bwd",
           "glam_layer_norm_flat_fwd", "glam_layer_norm_flat_bwd"]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "glam_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 4          # new entry points only: no exported signature changed
    # sized by the shape alone: 2 floats per (128-row slab, column), or per 4096-element chunk
    assert lib.glam_colnorm_workspace_bytes(300, 60) == 3 * 2 * 60 * 4
    assert lib.glam_colnorm_workspace_bytes(1, 300) == 2 * 300 * 4
    assert lib.glam_colnorm_workspace_bytes(0, 60) == 0


def test_entry_points_reject_bad_arguments_before_any_launch():
    raw = _lib.load()
    assert raw.glam_batch_norm_fwd(None, None, None, None, None, 4, 0, 0.1, 1e-5, None, None, None, None, 0, 0, 0, None) == _lib.GLAM_E_INVALID
    assert raw.glam_batch_norm_fwd(None, None, None, None, None, 4, 8, 0.1, 1e-5, None, None, None, None, 0, 0, 0, None) == _lib.GLAM_E_INVALID
    assert b"null pointer" in raw.glam_last_error()
    assert raw.glam_layer_norm_flat_fwd(None, None, None, 1 << 20, 1 << 12, 1e-5, None, None, None, 0, 0, 0, None) == _lib.GLAM_E_UNSUPPORTED
    assert raw.glam_batch_norm_bwd(None, None, None, None, None, 4, 8, 0, None, None, None, None, 0, 3, 0, None) == _lib.GLAM_E_INVALID


def test_ops_exist_and_refuse_cpu_tensors():
    assert ops.COLUMN_NORM is True
    x, w = torch.randn(4, 8), torch.ones(8)
    for call in (lambda: ops.batch_norm(x, w, w, w.clone(), w.clone(), True, 0.1, 1e-5), lambda: ops.layer_norm_flat(x, w, w, 1e-5)):
        try:
            call()
        except _lib.GlamHipError as e:
            assert "HIP device only" in str(e)
        else:
            raise AssertionError("a CPU tensor must not reach the kernels")


def test_cpu_tensors_take_the_unchanged_torch_route():
    torch.manual_seed(0)
    x = torch.randn(33, 60) * 2 + 1
    m = layer._BatchNorm(60)
    ref = copy.deepcopy(m.norm.module)
    for _ in range(2):
        assert torch.equal(m(x), ref(x))
    for name in ("running_mean", "running_var", "num_batches_tracked"):
        assert torch.equal(getattr(m.norm.module, name), getattr(ref, name))
    m.eval(), ref.eval()
    assert torch.equal(m(x), ref(x))
    ln = layer._LayerNorm(60)
    with torch.no_grad():
        ln.norm.weight.normal_()
        ln.norm.bias.normal_()
    c = x - x.mean()
    want = (c / (c.std(unbiased=False) + ln.norm.eps)) * ln.norm.weight + ln.norm.bias
    assert torch.equal(ln(x), want) and torch.equal(ln(x, None), want)
    out, ident = ln(x, None, with_identity=True)
    assert torch.equal(out, want) and ident is x


def test_state_dict_keys_are_the_parents():
    keys = list(model.Architecture(pre_norm="_BatchNorm", flat_norm="_LayerNorm").state_dict().keys())
    assert keys == ['mol_lin0.norm.norm.module.weight', 'mol_lin0.norm.norm.module.bias', 'mol_lin0.norm.norm.module.running_mean',
                    'mol_lin0.norm.norm.module.running_var', 'mol_lin0.norm.norm.module.num_batches_tracked', 'mol_lin0.linear.weight',
                    'mol_lin0.linear.bias', 'mol_conv.conv.conv.root', 'mol_conv.conv.conv.bias', 'mol_conv.conv.conv.nn.0.weight',
                    'mol_conv.conv.conv.nn.0.bias', 'mol_conv.conv.conv.nn.2.weight', 'mol_conv.conv.conv.nn.2.bias', 'mol_conv.gru.weight_ih_l0',
                    'mol_conv.gru.weight_hh_l0', 'mol_conv.gru.bias_ih_l0', 'mol_conv.gru.bias_hh_l0', 'mol_flat.norm.norm.weight',
                    'mol_flat.norm.norm.bias', 'mol_flat.linear.weight', 'mol_flat.linear.bias', 'lin_out1.linear.weight', 'lin_out1.linear.bias']


def test_offset_columns_separate_centred_from_sum_of_squares_variance():
    """The premise of test_gpu_colnorm.test_batch_norm_offset_columns, at its inputs (x = 100 + scaled randn): the float32 CPU oracle is
    within the fp64-twin bound by construction, a float32 E[x^2] - E[x]^2 restatement is not — at offset 100, which therefore stands."""
    for N, C in ((300, 60), (32, 1024)):
        g = torch.Generator().manual_seed(11 + C)
        x = torch.randn(N, C, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5) + 100.0
        w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
        outs = {}
        for dt in (torch.float32, torch.float64):
            m = torch.nn.BatchNorm1d(C).to(dt)
            with torch.no_grad():
                m.weight.copy_(w)
                m.bias.copy_(b)
            outs[dt] = m(x.to(dt)).detach()
        assert_fp32_parity(outs[torch.float32], outs[torch.float64], outs[torch.float32], "oracle", out_tol=1e-5)
        var = (x * x).mean(0) - x.mean(0) ** 2                     # float32 throughout
        naive = (x - x.mean(0)) / torch.sqrt(var + 1e-5) * w + b
        try:
            assert_fp32_parity(naive, outs[torch.float64], outs[torch.float32], "naive", out_tol=1e-5)
        except AssertionError:
            continue
        raise AssertionError(f"E[x^2] - E[x]^2 in float32 passes at ({N}, {C}): raise the offset")
