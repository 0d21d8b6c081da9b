"""Training steps of the two-drug model on pairs that SHARE drugs (a DDI set has far fewer distinct drugs than pairs):
  (a) model(B1, B2)                                       — one graph per pair and side, as the reference collates it (the yardstick)
  (b) model.forward_shared(drugs1, drugs2, first, second) — every distinct drug once per tower, the fusion and its backward through both indices
on default ArchitectureDDI() in train() (RReLU, Dropout(0.2)): forward + backward + glam_amd.optim.Adam on one cached batch, each leg
eager and under GraphedTrainStep.  The eager call of (a) goes through the model's own graphed-call route, as a trainer's does (a batch seen
before is replayed from hipGraphs); forward_shared has no such route, so "a eager, route off" (model.graphed_call = False) is timed as
well: that is the like-for-like eager launch sequence.  A case is PAIRS:DRUGS — the pairs are drawn uniformly (seeded) from one set of
DRUGS synthetic molecules, both sides from the same set; (b) passes each tower the distinct drugs of its own side.  All legs
alternate inside one process (every leg sees the same state of the box); a window is timed by the host clock and ends in a device
synchronise; reported: the median of the rounds and their min .. max.  Every leg has its own copy of the same initial model and its own
optimizer.  Also: max |a - b| of the two outputs in eval() on the timed batch.

usage: bench_ddi_shared.py [--rounds R] [--window SECONDS] [--out FILE] [--pairs P --drugs Q | P:Q ...]      (default 32:16 1024:256 1024:1024)"""
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glam_amd import loss as glam_loss, model, ops, optim
from glam_amd.data import Batch, synth_molecule
from glam_amd.graphs import GraphedTrainStep

_opts = {"--rounds": "5", "--window": "0.3", "--out": "", "--pairs": "", "--drugs": ""}
_args, _cases = sys.argv[1:], []
while _args:
    a = _args.pop(0)
    if a in _opts:
        _opts[a] = _args.pop(0)
    else:
        _cases.append(tuple(int(v) for v in a.split(":")))
if _opts["--pairs"] or _opts["--drugs"]:
    _cases.append((int(_opts["--pairs"] or 1024), int(_opts["--drugs"] or 256)))
CASES = _cases or [(32, 16), (1024, 256), (1024, 1024)]
ROUNDS, WINDOW = int(_opts["--rounds"]), float(_opts["--window"])
dev = torch.device("cuda")


class Pairs:
    def __init__(self, mol1, mol2, y, first=None, second=None):
        self.mol1, self.mol2, self.first, self.second, self.y = mol1, mol2, first, second, y


class Replicated(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, b):
        return self.net(b.mol1, b.mol2)


class Shared(Replicated):
    def forward(self, b):
        return self.net.forward_shared(b.mol1, b.mol2, b.first, b.second)


def loss_fn(out, b):
    return glam_loss.mse_loss(out.view(-1), b.y)


def make_leg(wrapper, net0, batch, graphed, route=True):
    mod = wrapper(copy.deepcopy(net0))
    if not route:
        mod.net.graphed_call = False
    opt = optim.Adam(mod.parameters(), lr=1e-3)
    if graphed:
        stepper = GraphedTrainStep(mod, opt, loss_fn)
        return lambda: stepper(batch)

    def step():
        opt.zero_grad(set_to_none=True)
        loss_fn(mod(batch), batch).backward()
        opt.step()
    return step


def window(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


lines = []
for P, Q in CASES:
    torch.manual_seed(0)
    ops.manual_seed(0, dev)
    rng = np.random.default_rng(P * 7919 + Q)
    net0 = model.ArchitectureDDI().to(dev).train()
    pool = [synth_molecule(rng) for _ in range(Q)]
    first, second = rng.integers(0, Q, P), rng.integers(0, Q, P)
    used1, first_in = np.unique(first, return_inverse=True)           # the distinct drugs of THIS step, side by side
    used2, second_in = np.unique(second, return_inverse=True)
    y = torch.from_numpy(rng.standard_normal(P).astype(np.float32)).to(dev)
    rep = Pairs(Batch.from_data_list([pool[q] for q in first]).to(dev), Batch.from_data_list([pool[q] for q in second]).to(dev), y)
    sha = Pairs(Batch.from_data_list([pool[q] for q in used1]).to(dev), Batch.from_data_list([pool[q] for q in used2]).to(dev), y,
                ops.pair_index(first_in, P, used1.size, name="first", over="drugs"),
                ops.pair_index(second_in, P, used2.size, name="second", over="drugs"))
    with torch.no_grad():
        ev = copy.deepcopy(net0).eval()
        diff = (ev(rep.mol1, rep.mol2) - ev.forward_shared(sha.mol1, sha.mol2, sha.first, sha.second)).abs().max().item()
        del ev
    legs = {"a eager": make_leg(Replicated, net0, rep, False), "a eager, route off": make_leg(Replicated, net0, rep, False, route=False),
            "b eager": make_leg(Shared, net0, sha, False),
            "a graphed": make_leg(Replicated, net0, rep, True), "b graphed": make_leg(Shared, net0, sha, True)}
    steps = {}
    for k, step in legs.items():
        window(step, 4)                                   # first visits, the capture, code objects
        steps[k] = max(5, min(400, int(WINDOW / window(step, 3))))
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, step in legs.items():                      # alternating
            times[k].append(window(step, steps[k]))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = {"workload": f"default ArchitectureDDI train(), fwd+bwd+Adam, {P} pairs over a set of {Q} drugs ({int(used1.size)} occur first, {int(used2.size)} second)",
           "rows_a": [int(rep.mol1.x.size(0)), int(rep.mol2.x.size(0))], "rows_b": [int(sha.mol1.x.size(0)), int(sha.mol2.x.size(0))], "rounds": ROUNDS, "steps_per_window": steps,
           "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
           "a_over_b_eager": round(med["a eager"] / med["b eager"], 3),
           "a_route_off_over_b_eager": round(med["a eager, route off"] / med["b eager"], 3), "a_over_b_graphed": round(med["a graphed"] / med["b graphed"], 3),
           "max_abs_diff_a_b_eval": diff, "peak_mem_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)
    del legs, rep, sha, net0
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
if _opts["--out"]:
    with open(_opts["--out"], "w") as f:
        f.write("\n".join(lines) + "\n")
