"""_BatchNorm and the batch-less _LayerNorm on csrc/colnorm.hip: every dispatch form against the CPU oracle in fp32 and
fp64 (``torch.nn.BatchNorm1d``, which is what PyG's BatchNorm wraps; the four-line expression of PyG's graph LayerNorm with
``batch=None``), running statistics, fallbacks, determinism and the captured step."""
import copy

import pytest
import torch

from glam_amd import layer, model, ops
from glam_amd.data import synth_batch
from tests.conftest import assert_fp32_parity, assert_twin_parity

pytestmark = pytest.mark.gpu

NAMES = ["x", "weight", "bias"]


def _inputs(N, C, seed, offset=None):
    """Seeded normal columns with a per-column offset in [-2, 2] (or ``offset`` everywhere) and scale in [0.5, 2]; random affine and
    cotangent."""
    g = torch.Generator().manual_seed(seed)
    off = torch.rand(C, generator=g) * 4 - 2 if offset is None else torch.full((C,), float(offset))
    x = torch.randn(N, C, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5) + off
    return x, torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(N, C, generator=g)


def _bn_oracle(x, w, b, cot, training=True, state=None):
    """``run(dtype) -> (out, [dx, dw, db])`` on a CPU ``torch.nn.BatchNorm1d``; the modules it built, per dtype, in ``mods``."""
    mods = {}

    def run(dt):
        m = torch.nn.BatchNorm1d(x.size(1)).to(dt)
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
            if state is not None:
                m.running_mean.copy_(state[0])
                m.running_var.copy_(state[1])
        m.train(training)
        xx = x.to(dt).requires_grad_(True)
        out = m(xx)
        mods[dt] = m
        return out.detach(), list(torch.autograd.grad(out, [xx, m.weight, m.bias], cot.to(dt)))

    return run, mods


def _bn_module(C, w, b, device):
    m = layer._BatchNorm(C).to(device)
    with torch.no_grad():
        m.norm.module.weight.copy_(w)
        m.norm.module.bias.copy_(b)
    return m


def _check_bn_training(device, N, C, seed, offset=None, form=0, max_blocks=0, misalign=False):
    x, w, b, cot = _inputs(N, C, seed, offset)
    run, mods = _bn_oracle(x, w, b, cot)
    m = _bn_module(C, w, b, device)
    bn = m.norm.module
    if misalign:        # a contiguous [N, C] whose rows start 4 bytes off a 16-byte boundary: the scalar path
        xd = torch.empty(N * C + 1, device=device)[1:].view(N, C).copy_(x).requires_grad_(True)
        assert xd.data_ptr() % 16 == 4
    else:
        xd = x.to(device).requires_grad_(True)
    if form or max_blocks or misalign:
        out = ops.batch_norm(xd, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, bn.momentum, bn.eps, form, max_blocks)
    else:
        out = m(xd)
    grads = torch.autograd.grad(out, [xd, bn.weight, bn.bias], cot.to(device))
    what = f"batch_norm[{N}x{C} form {form} cap {max_blocks}]"
    assert_twin_parity(run, out, grads, what, NAMES)
    m32, m64 = mods[torch.float32], mods[torch.float64]
    assert_fp32_parity(bn.running_mean, m64.running_mean, m32.running_mean, what + " running_mean")
    assert_fp32_parity(bn.running_var, m64.running_var, m32.running_var, what + " running_var")
    return out, grads


# the issue's shapes; 256 | 257 rows: either side of the column-owner / row-split boundary; (257, 90) and (300, 60): three slabs of 128
# rows with a ragged last one; (700, 20): six slabs, scalar path
BN_SHAPES = [(2, 15), (67, 15), (300, 60), (257, 90), (33, 300), (32, 1024), (4, 2048), (7, 75), (256, 60), (257, 60), (700, 20)]


@pytest.mark.parametrize("N,C", BN_SHAPES)
def test_batch_norm_training(device, N, C):
    _check_bn_training(device, N, C, seed=N * 7 + C)


@pytest.mark.parametrize("N,C,form,cap,misalign", [
    (300, 60, 2, 2, False),       # row-split, 3 work items on 2 blocks: the grid-stride loops of both launches take a second trip
    (300, 90, 2, 5, False),       # ... scalar path: 3 slabs x 6 column tiles on 5 blocks
    (33, 300, 1, 2, False),       # column-owner, 5 column tiles on 2 blocks
    (33, 75, 1, 3, False),        # ... scalar path, 5 tiles on 3 blocks
    (300, 60, 1, 0, False),       # the other form at a row-split shape
    (67, 60, 2, 0, False),        # ... and at a column-owner shape (one ragged slab)
    (300, 60, 0, 0, True),        # C % 4 == 0 on a misaligned base: scalar accesses
    (40, 64, 0, 0, True),
])
def test_batch_norm_forms_and_grid_stride(device, N, C, form, cap, misalign):
    _check_bn_training(device, N, C, seed=N + C + form + cap, form=form, max_blocks=cap, misalign=misalign)


@pytest.mark.parametrize("N,C", [(300, 60), (32, 1024)])
def test_batch_norm_offset_columns(device, N, C):
    """x = 100 + randn: the centred CPU oracle's fp32 noise stays near the spacing of the values around 100, and so must the kernels'
    (offset used: 100; tests/test_colnorm_host.py checks on the CPU that a float32 E[x^2] - E[x]^2 restatement misses this bound)."""
    _check_bn_training(device, N, C, seed=11 + C, offset=100.0)


def test_batch_norm_running_statistics_and_eval(device):
    N, C = 300, 60
    x4 = [_inputs(N, C, seed=40 + i) for i in range(4)]
    w, b = x4[0][1], x4[0][2]
    m = _bn_module(C, w, b, device)
    bn = m.norm.module
    ref = {dt: torch.nn.BatchNorm1d(C).to(dt) for dt in (torch.float32, torch.float64)}
    for dt, r in ref.items():
        with torch.no_grad():
            r.weight.copy_(w)
            r.bias.copy_(b)
    for x, _, _, _ in x4[:3]:
        m(x.to(device))
        for dt, r in ref.items():
            r(x.to(dt))
    assert int(bn.num_batches_tracked) == 3 == int(ref[torch.float32].num_batches_tracked)
    for name in ("running_mean", "running_var"):
        assert_fp32_parity(getattr(bn, name), getattr(ref[torch.float64], name), getattr(ref[torch.float32], name), name)
    x, _, _, cot = x4[3]
    m.eval()

    def run(dt):
        r = ref[dt].eval()
        xx = x.to(dt).requires_grad_(True)
        out = r(xx)
        return out.detach(), list(torch.autograd.grad(out, [xx, r.weight, r.bias], cot.to(dt)))

    before = bn.running_mean.clone(), bn.running_var.clone()
    for form, cap in ((0, 0), (1, 0), (2, 2)):
        xd = x.to(device).requires_grad_(True)
        out = m(xd) if form == 0 else ops.batch_norm(xd, bn.weight, bn.bias, bn.running_mean, bn.running_var, False, bn.momentum, bn.eps, form, cap)
        grads = torch.autograd.grad(out, [xd, bn.weight, bn.bias], cot.to(device))
        assert_twin_parity(run, out, grads, f"batch_norm eval form {form}", NAMES)
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and int(bn.num_batches_tracked) == 3


def test_batch_norm_fallbacks_keep_their_behaviour(device):
    C = 60
    x, w, b, _ = _inputs(300, C, seed=5)
    m = _bn_module(C, w, b, device)
    with pytest.raises(ValueError):
        m(x[:1].to(device))
    # an fp64 input through an fp64 module, and momentum=None (cumulative average): torch's own results
    m64 = copy.deepcopy(m).double()
    ref64 = copy.deepcopy(m64.norm.module)
    assert torch.equal(m64(x.to(device).double()), ref64(x.to(device).double()))
    mn = layer.BatchNorm(C, momentum=None).to(device)
    refn = copy.deepcopy(mn.module)
    assert torch.equal(mn(x.to(device)), refn(x.to(device))) and torch.equal(mn.module.running_mean, refn.running_mean)
    # the A/B switch: the parent's route, bit for bit
    ma, mb = copy.deepcopy(m), copy.deepcopy(m.norm.module)
    ops.COLUMN_NORM = False
    try:
        got = ma(x.to(device))
    finally:
        ops.COLUMN_NORM = True
    assert torch.equal(got, mb(x.to(device))) and torch.equal(ma.norm.module.running_var, mb.running_var)


def test_batch_norm_takes_the_hip_route(device, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("torch.nn.functional.batch_norm was called")

    monkeypatch.setattr(torch.nn.functional, "batch_norm", boom)
    x = torch.randn(300, 60, device=device)
    for training in (True, False):
        m = layer._BatchNorm(60).to(device).train(training)
        xd = x.clone().requires_grad_(True)
        out = m(xd)
        out.sum().backward()
        assert xd.grad is not None and m.norm.module.weight.grad is not None and torch.isfinite(out).all()


def _ln_oracle(x, w, b, cot, eps=1e-5):
    def run(dt):
        xx, ww, bb = (t.to(dt).requires_grad_(True) for t in (x, w, b))
        c = xx - xx.mean()
        out = c / (c.std(unbiased=False) + eps)
        out = out * ww + bb
        return out.detach(), list(torch.autograd.grad(out, [xx, ww, bb], cot.to(dt)))

    return run


def _check_ln(device, N, C, seed, offset=None, form=0, max_blocks=0, shift=0.0):
    x, w, b, cot = _inputs(N, C, seed, offset)
    x = x + shift
    m = layer._LayerNorm(C).to(device)
    with torch.no_grad():
        m.norm.weight.copy_(w)
        m.norm.bias.copy_(b)
    xd = x.to(device).requires_grad_(True)
    if form or max_blocks:
        out = ops.layer_norm_flat(xd, m.norm.weight, m.norm.bias, m.norm.eps, form, max_blocks)
    else:
        out = m(xd)
        assert torch.equal(out, m(xd, None))
    grads = torch.autograd.grad(out, [xd, m.norm.weight, m.norm.bias], cot.to(device))
    assert_twin_parity(_ln_oracle(x, w, b, cot), out, grads, f"layer_norm_flat[{N}x{C} form {form} cap {max_blocks}]", NAMES)
    return out, grads


# the issue's shapes; (64, 256) | (65, 256): 16384 | 16640 elements, either side of the one-block boundary; (50, 330): scalar path, two launches
LN_SHAPES = [(1, 300), (32, 300), (33, 75), (32, 1024), (1024, 450), (64, 256), (65, 256), (50, 330)]


@pytest.mark.parametrize("N,C", LN_SHAPES)
def test_layer_norm_flat(device, N, C):
    _check_ln(device, N, C, seed=N * 3 + C)


@pytest.mark.parametrize("N,C,form,cap,shift", [
    (65, 256, 2, 2, 0.0),         # 5 chunks, 1 slab x 4 column tiles on 2 blocks: every grid-stride loop takes further trips
    (300, 75, 2, 3, 0.0),         # scalar path: 6 chunks, 3 slabs x 5 tiles on 3 blocks
    (32, 300, 2, 0, 0.0),         # the two-launch form at a one-block shape
    (65, 256, 1, 0, 0.0),         # one block past the boundary
    (32, 300, 0, 0, 100.0),       # the whole tensor offset by 100
    (1024, 450, 0, 0, 100.0),
])
def test_layer_norm_flat_forms_and_offset(device, N, C, form, cap, shift):
    _check_ln(device, N, C, seed=N + C + form + cap, form=form, max_blocks=cap, shift=shift)


def test_two_runs_are_bit_identical(device):
    for check, N, C in ((_check_bn_training, 257, 90), (_check_bn_training, 4, 2048), (_check_bn_training, 300, 60), (_check_ln, 1024, 450)):
        (o1, g1), (o2, g2) = check(device, N, C, seed=77), check(device, N, C, seed=77)
        assert torch.equal(o1, o2)
        for a, r in zip(g1, g2):
            assert torch.equal(a, r)


def test_captured_step_equals_the_eager_step(device):
    """All four norm slots on the column norms, the same batch four times (eager, eager on the static copy, capture + replay, replay):
    outputs, gradients and BatchNorm buffers equal the eager model's after every call — the same kernels in the same order."""
    torch.manual_seed(13)
    net = model.Architecture(pre_norm="_BatchNorm", graph_norm="_BatchNorm", flat_norm="_LayerNorm", end_norm="_BatchNorm", pre_act="ReLU",
                             graph_act="ReLU", flat_act="ReLU", graph_do="_None()", end_do="_None()", mol_block="_TripletMessage").to(device)
    ref = copy.deepcopy(net)
    ref.graphed_call = False
    b = synth_batch(8, seed=3).to(device)
    for visit in range(4):
        outs = []
        for m in (net, ref):
            m.zero_grad(set_to_none=True)
            out = m(b)
            torch.nn.functional.mse_loss(out.view(-1), b.y.view(-1).float()).backward()
            outs.append(out.detach().clone())
        assert torch.equal(outs[0], outs[1]), visit
        for (n, p), q in zip(net.named_parameters(), ref.parameters()):
            assert p.grad is not None and torch.equal(p.grad, q.grad), (visit, n)
        for (n, u), v in zip(net.named_buffers(), ref.buffers()):
            assert torch.equal(u, v), (visit, n)
    assert net.__dict__["_glam_graphed_route"].graphs() == 2
    tracked = [int(u) for n, u in net.named_buffers() if n.endswith("num_batches_tracked")]
    # (the message block's norm runs once per message step)
    assert tracked == [4, 4 * net.message_steps, 4], tracked
