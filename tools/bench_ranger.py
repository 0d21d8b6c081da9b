"""Developer aid: one Ranger step on a default-shaped model's parameter list (run under rocprofv3 --kernel-trace for the kernel time).
    ranger-eager     glam_amd.optim.Ranger, step() called from Python
    ranger-graph     glam_amd.optim.Ranger, 20 steps captured in one hipGraph
    reference-loop   the reference's per-tensor loop (src_1gp/ranger.py:117-205), restated below, step() called from Python
    adam-graph       glam_amd.optim.Adam, 20 steps captured in one hipGraph (for scale)
Usage: python tools/bench_ranger.py [case ...]   (default: all four)"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from glam_amd import model, optim


class LoopRanger(torch.optim.Optimizer):
    """The reference's arithmetic as it runs there: a Python loop over the tensors, ATen operations per tensor, a host int step."""

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0):
        super().__init__(params, dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                                      weight_decay=weight_decay))
        self.alpha, self.N_sma_threshhold = alpha, N_sma_threshhold

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad.data.float()
                x = p.data.float()
                st = self.state[p]
                if not st:
                    st.update(step=0, exp_avg=torch.zeros_like(x), exp_avg_sq=torch.zeros_like(x), slow_buffer=p.data.clone())
                if g.dim() > 1:
                    g.add_(-g.mean(dim=tuple(range(1, g.dim())), keepdim=True))
                st["step"] += 1
                s, m, v = st["step"], st["exp_avg"], st["exp_avg_sq"]
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                m.mul_(b1).add_(g, alpha=1 - b1)
                b2t = b2 ** s
                n_max = 2 / (1 - b2) - 1
                n_sma = n_max - 2 * s * b2t / (1 - b2t)
                if n_sma > self.N_sma_threshhold:
                    step_size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** s)
                    G = m / v.sqrt().add_(group["eps"])
                else:
                    step_size = 1.0 / (1 - b1 ** s)
                    G = m
                if group["weight_decay"] != 0:
                    G.add_(x, alpha=group["weight_decay"])
                x.add_(G, alpha=-step_size * group["lr"])
                p.data.copy_(x)
                if s % group["k"] == 0:
                    slow = st["slow_buffer"]
                    slow.add_(p.data - slow, alpha=self.alpha)
                    p.data.copy_(slow)


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cases = sys.argv[1:] or ["ranger-eager", "ranger-graph", "reference-loop", "adam-graph"]
    for case in cases:
        net = model.Architecture(mol_block="_TripletMessage").to(dev)
        params = list(net.parameters())
        opt = {"ranger-eager": lambda: optim.Ranger(params, lr=1e-3),
               "ranger-graph": lambda: optim.Ranger(params, lr=1e-3),
               "reference-loop": lambda: LoopRanger(params, lr=1e-3),
               "adam-graph": lambda: optim.Adam(params, lr=1e-3)}[case]()
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        for _ in range(5):
            opt.step()
        torch.cuda.synchronize()
        if case.endswith("graph"):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(20):
                    opt.step()
            g.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(50):
                g.replay()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / 1000 * 1e6
        else:
            t0 = time.perf_counter()
            for _ in range(200):
                opt.step()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / 200 * 1e6
        print(f"{case}: {us:.2f} us per optimizer step, {sum(p.numel() for p in params)} parameters in {len(params)} tensors", flush=True)


if __name__ == "__main__":
    main()
