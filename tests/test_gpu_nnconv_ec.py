"""NNConv over continuous edge features on HIP (csrc/nnconv_ec.hip, ``ops.nnconv_edge_conditioned``): the protein tower's
``_NNConv`` (src_2gi_dti_scr/glam.py) against the fp64 twin of the oracle, without the per-edge weight tensor [E, C*C]."""
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import layer, model, ops
from glam_amd.data import Batch, Data, synth_protein_batch
from tests.conftest import assert_twin_parity

pytestmark = pytest.mark.gpu


def _grads(out, cot, tensors):
    gs = torch.autograd.grad((out * cot).sum(), tensors, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(gs, tensors)]


def _nnconv_ref(x, ei, ea, w0, b0, w1, b1, root, bias, mean):
    if mean:
        return O.nnconv_mean(x, ei, ea, w0, b0, w1, b1, root, bias)
    w_e = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(ea, w0, b0)), w1, b1).view(-1, x.size(1), root.size(1))
    msg = torch.matmul(x.index_select(0, ei[0]).unsqueeze(1), w_e).squeeze(1)
    return torch.zeros(x.size(0), root.size(1), dtype=x.dtype).index_add_(0, ei[1], msg) + x @ root + bias


def _hub_graph():
    """50 nodes: node 0 has in-degree 240, nodes 1..20 form a chain, nodes 40..49 have no edges at all (isolated)."""
    src = torch.arange(1, 41).repeat(6)[:240] % 40
    src[src == 0] = 1
    hub = torch.stack([src, torch.zeros_like(src)])
    chain = torch.stack([torch.arange(1, 20), torch.arange(2, 21)])
    return 50, torch.cat([hub, chain, chain.flip(0)], 1)


def _graph(kind, De, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "proteins":
        b = synth_protein_batch(4, seed=seed + 1, n_min=60, n_max=200)
        ei, N = b.edge_index, b.x.size(0)
    elif kind == "hub":
        N, ei = _hub_graph()
    else:                                    # no edges
        N, ei = 10, torch.zeros(2, 0, dtype=torch.int64)
    return N, ei, torch.rand(ei.size(1), De, generator=g)


def _layer(C, De, mean):
    conv = layer._NNConv(C, C, De).conv if mean else layer.NNConv(C, C, torch.nn.Sequential(
        torch.nn.Linear(De, 32), torch.nn.ReLU(), torch.nn.Linear(32, C * C)), aggr="add")
    with torch.no_grad():
        conv.bias.uniform_(-0.1, 0.1)
    return conv


def _check_layer(device, C, De, mean, kind):
    torch.manual_seed(C + De)
    N, ei, ea = _graph(kind, De, seed=C)
    conv = _layer(C, De, mean)
    x0, cot = torch.randn(N, C), torch.randn(N, C)
    sd0 = {k: v.detach().clone() for k, v in conv.state_dict().items()}
    names = list(sd0)

    def run(dt):
        sd = {k: v.to(dt).requires_grad_(True) for k, v in sd0.items()}
        xo = x0.to(dt).requires_grad_(True)
        o = _nnconv_ref(xo, ei, ea.to(dt), sd["nn.0.weight"], sd["nn.0.bias"], sd["nn.2.weight"], sd["nn.2.bias"], sd["root"], sd["bias"], mean)
        return o, _grads(o, cot.to(dt), [xo] + [sd[k] for k in names])
    conv = conv.to(device)
    x = x0.to(device).requires_grad_(True)
    out = conv(x, ei.to(device), ea.to(device))
    params = dict(conv.named_parameters())
    assert_twin_parity(run, out, _grads(out, cot.to(device), [x] + [params[k] for k in names]), f"nnconv_ec C={C} De={De} {kind}",
                       ["x"] + names)


@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("De", [4, 8])
@pytest.mark.parametrize("C", [15, 30, 60, 90])
def test_layer_parity_on_proteins(device, C, De, mean):
    _check_layer(device, C, De, mean, "proteins")


@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("kind", ["hub", "empty"])
@pytest.mark.parametrize("C", [15, 45])
def test_layer_parity_on_edge_cases(device, C, kind, mean):
    """isolated nodes, in-degree 240, N < 64; and a graph with no edges at all (E = 0)."""
    _check_layer(device, C, 8, mean, kind)


def test_op_matches_the_layer_and_the_torch_operator(device):
    """``ops.nnconv_edge_conditioned`` and ``torch.ops.glam.nnconv_ec`` compute what the routed layer computes, bit for bit."""
    from glam_amd import torch_ext
    torch.manual_seed(2)
    N, ei, ea = _graph("proteins", 8, seed=3)
    conv = _layer(30, 8, True).to(device)
    ei, ea = ei.to(device), ea.to(device)
    x = torch.randn(N, 30, device=device)
    gi = ops.graph_index(ei, N)
    l0, l2 = conv.nn[0], conv.nn[2]
    with torch.no_grad():
        a = conv(x, ei, ea)
        b = ops.nnconv_edge_conditioned(x, ea, gi, l0.weight, l0.bias, l2.weight, l2.bias, conv.root, conv.bias, mean=True)
        c = torch_ext.load().nnconv_ec(x, ea, l0.weight, l0.bias, l2.weight, l2.bias, conv.root, conv.bias, gi.rowptr, gi.src, gi.eid,
                                       *gi.transpose(), True)
    assert torch.equal(a, b) and torch.equal(a, c)
    xg = x.clone().requires_grad_(True)
    ps = [xg, l0.weight, l0.bias, l2.weight, l2.bias, conv.root, conv.bias]
    g1 = torch.autograd.grad(conv(xg, ei, ea).square().sum(), ps)
    g2 = torch.autograd.grad(torch_ext.load().nnconv_ec(xg, ea, l0.weight, l0.bias, l2.weight, l2.bias, conv.root, conv.bias, gi.rowptr,
                                                        gi.src, gi.eid, *gi.transpose(), True).square().sum(), ps)
    for u, v in zip(g1, g2):
        assert torch.equal(u, v)


def test_message_block_three_shared_applications(device):
    """MessageBlock(conv='_NNConv', res=True) on 8 continuous edge features, applied 3 times with the same weights (the
    forward_with_identity path: the skip connection's gradient joins the conv's backward launch)."""
    torch.manual_seed(7)
    b = synth_protein_batch(4, seed=9, n_min=60, n_max=160)
    C = 30
    blk = layer.MessageBlock(C, C, 8, norm="_None", dropout="_None()", conv="_NNConv", act="ReLU()", res=True).eval()
    x0, cot = torch.randn(b.x.size(0), C), torch.randn(b.x.size(0), C)
    names = [n for n, _ in blk.named_parameters()]
    sd0 = {k: v.detach().clone() for k, v in blk.state_dict().items()}

    def run(dt):
        sd = {k: v.to(dt).requires_grad_(True) for k, v in sd0.items()}
        xo = x0.to(dt).requires_grad_(True)
        y, h = xo, None
        for _ in range(3):
            y, h = O.message_block(sd, "", y, b.edge_index, b.edge_attr.to(dt), h, b.batch, 4, "_NNConv", "_None", "ReLU")
        return y, _grads(y, cot.to(dt), [xo] + [sd[n] for n in names])
    blk = blk.to(device)
    bd = b.to(device)
    x = x0.to(device).requires_grad_(True)
    with ops.weight_scope():
        y, h = x, None
        for _ in range(3):
            y, h = blk(y, bd.edge_index, bd.edge_attr, h=h, batch=bd.batch)
    assert_twin_parity(run, y, _grads(y, cot.to(device), [x] + [p for _, p in blk.named_parameters()]), "block", ["x"] + names)


def test_two_tower_model_with_nnconv_proteins(device):
    torch.manual_seed(12)
    from glam_amd.data import synth_batch
    mb = synth_batch(4, seed=3)
    pb = synth_protein_batch(4, seed=4, n_min=40, n_max=130)
    kw = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU")
    net = model.ArchitectureDTI(pro_block="_NNConv", e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **kw).eval()
    names = [n for n, _ in net.named_parameters()]
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ref = O.architecture_dti({k: v.clone() for k, v in sd0.items()}, mb, pb, 4, message_steps=2, pro_block="_NNConv", **kw)
    cot = torch.randn(ref.shape)
    net = net.to(device)
    out = net(mb.to(device), pb.to(device))
    gs = torch.autograd.grad((out * cot.to(device)).sum(), [p for _, p in net.named_parameters()], allow_unused=True)

    def run(dt):
        sd_ = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd0.items()}
        cast = lambda b: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)
        o = O.architecture_dti(sd_, cast(mb), cast(pb), 4, message_steps=2, pro_block="_NNConv", **kw)
        return o.detach(), torch.autograd.grad((o * cot.to(dt)).sum(), [sd_[n] for n in names], allow_unused=True)
    assert_twin_parity(run, out, gs, "dti nnconv proteins", names)


def _big(device):
    b = synth_protein_batch(32, seed=1).to(device)
    torch.manual_seed(0)
    conv = layer._NNConv(60, 60, 8).to(device)
    return b, conv


def test_no_per_edge_weight_tensor(device):
    """The peak-memory rise of one forward + backward at C = 60 on 32 proteins stays below a quarter of the E * C^2 tensor the
    per-edge route allocates."""
    b, conv = _big(device)
    E = b.edge_index.size(1)
    x = torch.randn(b.x.size(0), 60, device=device, requires_grad=True)
    ops.graph_index(b.edge_index, b.x.size(0))          # (the CSR is staged once per edge list: not part of the layer's working set)
    conv(x, b.edge_index, b.edge_attr).sum().backward()  # (and the transpose)
    x.grad = None
    for p in conv.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    conv(x, b.edge_index, b.edge_attr).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < E * 60 * 60 * 4 / 4, f"peak rise {rise / 2**20:.1f} MiB vs E*C^2/4 = {E * 3600 / 2**20:.1f} MiB"


def test_no_library_kernel_on_rows_of_the_graph(device):
    from torch.utils._python_dispatch import TorchDispatchMode
    b, conv = _big(device)
    N, E = b.x.size(0), b.edge_index.size(1)
    x = torch.randn(N, 60, device=device, requires_grad=True)
    bad = []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func)
            if any(name.startswith("aten." + k + ".") or name == "aten." + k for k in ("bmm", "mm", "addmm", "matmul", "linear")):
                if any(isinstance(a, torch.Tensor) and a.dim() >= 1 and a.size(0) in (N, E) for a in args):
                    bad.append(name)
            return func(*args, **(kwargs or {}))
    with Log():
        conv(x, b.edge_index, b.edge_attr).sum().backward()
    torch.cuda.synchronize()
    assert not bad, bad


def test_bit_identical_runs(device):
    b, conv = _big(device)
    x0 = torch.randn(b.x.size(0), 60, device=device)
    cot = torch.randn(b.x.size(0), 60, device=device)
    res = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        out = conv(x, b.edge_index, b.edge_attr)
        res.append([out.detach()] + list(torch.autograd.grad((out * cot).sum(), [x] + list(conv.parameters()))))
    for u, v in zip(*res):
        assert torch.equal(u, v)


def test_graph_capture_replays_like_eager(device):
    torch.manual_seed(4)
    b = synth_protein_batch(4, seed=2, n_min=60, n_max=200).to(device)
    conv = layer._NNConv(45, 45, 8).to(device)
    params = list(conv.parameters())
    N = b.x.size(0)
    x_static = torch.randn(N, 45, device=device, requires_grad=True)

    def step():
        out = conv(x_static, b.edge_index, b.edge_attr)
        return [out] + list(torch.autograd.grad(out.square().sum(), [x_static] + params))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_out = step()
    for seed in (10, 11):
        torch.manual_seed(seed)
        xn = torch.randn(N, 45, device=device)
        with torch.no_grad():
            x_static.copy_(xn)
        g.replay()
        torch.cuda.synchronize()
        eager = step()
        for u, v in zip(static_out, eager):
            assert torch.equal(u, v)
