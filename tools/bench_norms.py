"""Forward + backward of _BatchNorm and the batch-less _LayerNorm under a hipGraph, column-norm kernels (ops.COLUMN_NORM = True) against the
torch route (False) in one process: warm-up, windows of replays alternating between the two routes, median per route.
usage: bench_norms.py [--replays 200] [--windows 7] [--forms]      (--forms: also both forced forms of the C ABI, for the dispatch rule)"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from glam_amd import layer, ops

ap = argparse.ArgumentParser()
ap.add_argument("--replays", type=int, default=200)
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--forms", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda")

BN_SHAPES = [(20686, 15), (20686, 60), (20686, 90), (646, 60), (1024, 300), (1024, 1024), (32, 300), (32, 1024), (32, 2048)]
LN_SHAPES = [(1024, 300), (1024, 1024), (32, 300), (32, 1024)]


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    return g


def step_of(kind, N, C, column_norm, form):
    torch.manual_seed(0)
    m = (layer._BatchNorm(C) if kind == "bn" else layer._LayerNorm(C)).to(dev)
    x = (torch.randn(N, C, device=dev) * 1.5 + 0.5).requires_grad_(True)
    cot = torch.randn(N, C, device=dev)
    params = [x] + list(m.parameters())

    def fn():
        ops.COLUMN_NORM = column_norm
        try:
            if form == 0:
                out = m(x)
            elif kind == "bn":
                bn = m.norm.module
                out = ops.batch_norm(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, bn.momentum, bn.eps, form)
            else:
                out = ops.layer_norm_flat(x, m.norm.weight, m.norm.bias, m.norm.eps, form)
            return torch.autograd.grad(out, params, cot)
        finally:
            ops.COLUMN_NORM = True

    return fn


def us_per_replay(graphs):
    """Median over the windows of each graph's time per replay; the graphs take turns inside every window."""
    times = [[] for _ in graphs]
    for _ in range(args.windows):
        for k, g in enumerate(graphs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.replays):
                g.replay()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.replays * 1e6)
    return [statistics.median(t) for t in times], [max(t) - min(t) for t in times]


print(f"forward + backward under a hipGraph, us per replay (median of {args.windows} windows of {args.replays} replays; spread = max - min)")
head = f"{'module':10s} {'N':>6s} {'C':>5s} {'torch':>8s} {'hip':>8s} {'hip/torch':>9s} {'spread t/h':>12s}"
print(head + ("   form1   form2" if args.forms else ""))
for kind, shapes in (("bn", BN_SHAPES), ("ln", LN_SHAPES)):
    for N, C in shapes:
        routes = [(False, 0), (True, 0)] + ([(True, 1), (True, 2)] if args.forms else [])
        graphs = [graph_of(step_of(kind, N, C, cn, form)) for cn, form in routes]
        med, spread = us_per_replay(graphs)
        line = (f"{'_BatchNorm' if kind == 'bn' else '_LayerNorm':10s} {N:6d} {C:5d} {med[0]:8.2f} {med[1]:8.2f} {med[1] / med[0]:9.2f} "
                f"{spread[0]:5.2f}/{spread[1]:5.2f}")
        if args.forms:
            line += f" {med[2]:7.2f} {med[3]:7.2f}"
        print(line, flush=True)
