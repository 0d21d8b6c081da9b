"""Microseconds per forward + backward of each criterion of glam_amd.loss on its HIP route against torch's module, eager and inside a
captured torch.cuda.graph.  One JSON line per (criterion, shape, route, launch).

    python tools/bench_loss.py [--iters N]

Shapes: the screening head (C = 2) at B = 32 and 1024, C = 86 at B = 1024 (a DDI-sized head); the elementwise criteria at
n = 32, 1024 and 631 808.  The root gradient is a kept tensor (``backward(gradient=one)``), as in a captured training step."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from glam_amd import loss

ITERS = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 200
dev = torch.device("cuda")
torch.manual_seed(0)
one = torch.ones((), device=dev)
w2 = torch.tensor([0.6, 3.1], device=dev)


def class_case(B, C):
    y = torch.randint(0, C, (B,), device=dev)
    return torch.randn(B, C, device=dev), y


def elem_case(n, prob=False):
    p, t = torch.randn(n, device=dev), torch.randn(n, device=dev)
    return (torch.sigmoid(p), (t > 0).float()) if prob else (p, t)


def focal_torch(x, y, alpha=0.25, gamma=2):
    ce = torch.nn.functional.cross_entropy(x, y, reduction='none')
    pt = torch.exp(-ce)
    return (alpha * (1 - pt) ** gamma * ce).mean()


cases = []
for B, C in ((32, 2), (1024, 2), (1024, 86)):
    x, y = class_case(B, C)
    w = w2 if C == 2 else torch.rand(C, device=dev) + 0.5
    cases += [("ce", f"B={B} C={C}", loss.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(), x, y),
              ("wce", f"B={B} C={C}", loss.CrossEntropyLoss(weight=w), torch.nn.CrossEntropyLoss(weight=w), x, y),
              ("focal", f"B={B} C={C}", loss.FocalLoss(), focal_torch, x, y)]
for n in (32, 1024, 631808):
    p, t = elem_case(n)
    pb, tb = elem_case(n, prob=True)
    cases += [("mae", f"n={n}", loss.L1Loss(), torch.nn.L1Loss(), p, t),
              ("huber", f"n={n}", loss.SmoothL1Loss(), torch.nn.SmoothL1Loss(), p, t),
              ("bce", f"n={n}", loss.BCELoss(), torch.nn.BCELoss(), pb, tb)]


def timed(step):
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e6


for name, shape, hip, ref, a, b in cases:
    res = {}
    for route, crit in (("hip", hip), ("torch", ref)):
        x = a.clone().requires_grad_(True)

        def body(x=x, crit=crit):
            x.grad = None
            crit(x, b).backward(gradient=one)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                body()
        torch.cuda.current_stream().wait_stream(side)
        eager = timed(body)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        graph = timed(g.replay)
        res[route] = (eager, graph)
        print(json.dumps({"criterion": name, "shape": shape, "route": route, "eager_us": round(eager, 2),
                          "graph_us": round(graph, 2)}), flush=True)
    print(json.dumps({"criterion": name, "shape": shape, "speedup_eager": round(res["torch"][0] / res["hip"][0], 2),
                      "speedup_graph": round(res["torch"][1] / res["hip"][1], 2)}), flush=True)
