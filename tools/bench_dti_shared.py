"""Training steps of the two-tower model on pairs that SHARE proteins (a LIT-PCBA step: every ligand of the batch against one target):
  (a) model(ligands, replicated protein batch)        — one copy of the protein per pair, as the reference collates it (the yardstick)
  (b) model.forward_shared(ligands, proteins, index)  — every distinct protein once, the fusion and its backward through the index
on default ArchitectureDTI() in train() (RReLU, Dropout(0.2)): forward + backward + glam_amd.optim.Adam on one cached batch, each leg
eager and under GraphedTrainStep.  The eager call of (a) goes through the model's own graphed-call route, as a trainer's does (a batch seen
before is replayed from hipGraphs); forward_shared has no such route, so "a eager, route off" (model.graphed_call = False) is timed as
well: that is the like-for-like eager launch sequence.  Cases: B = 32 and B = 1 024 ligands against ONE 500-residue protein, and
B = 32 against 8 distinct proteins (4 pairs each).  All legs alternate inside one process (every leg sees the same state of the box); a window is timed by the
host clock and ends in a device synchronise; reported: the median of the rounds and their min .. max.  Every leg has its own copy of
the same initial model and its own optimizer.  Also: max |a - b| of the two outputs in eval() on the timed batch.

usage: bench_dti_shared.py [--rounds R] [--window SECONDS] [--residues N] [--out FILE] [B:Q ...]        (default 32:1 32:8 1024:1)"""
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
from glam_amd.data import Batch, synth_batch, synth_protein
from glam_amd.graphs import GraphedTrainStep

_opts = {"--rounds": "5", "--window": "0.3", "--residues": "500", "--out": ""}
_args, _cases = sys.argv[1:], []
while _args:
    a = _args.pop(0)
    if a in _opts:
        _opts[a] = _args.pop(0)
    else:
        _cases.append(tuple(int(v) for v in a.split(":")))
CASES = _cases or [(32, 1), (32, 8), (1024, 1)]
ROUNDS, WINDOW, RES = int(_opts["--rounds"]), float(_opts["--window"]), int(_opts["--residues"])
dev = torch.device("cuda")
rng = np.random.default_rng(0)


class Pairs:
    def __init__(self, mol, pro, index=None):
        self.mol, self.pro, self.index, self.y = mol, pro, index, mol.y.view(-1)


class Replicated(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, b):
        return self.net(b.mol, b.pro)


class Shared(Replicated):
    def forward(self, b):
        return self.net.forward_shared(b.mol, b.pro, b.index)


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
for B, Q in CASES:
    torch.manual_seed(0)
    ops.manual_seed(0, dev)
    net0 = model.ArchitectureDTI().to(dev).train()
    proteins = [synth_protein(rng, RES, RES) for _ in range(Q)]
    idx = [i % Q for i in range(B)]
    mol = synth_batch(B, seed=B).to(dev)
    rep = Pairs(mol, Batch.from_data_list([proteins[q] for q in idx]).to(dev))
    sha = Pairs(mol, Batch.from_data_list(proteins).to(dev), ops.pair_index(idx, B, Q))
    with torch.no_grad():
        ev = copy.deepcopy(net0).eval()
        diff = (ev(rep.mol, rep.pro) - ev.forward_shared(sha.mol, sha.pro, sha.index)).abs().max().item()
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
    row = {"workload": f"default ArchitectureDTI train(), fwd+bwd+Adam, B={B} ligands x {Q} distinct {RES}-residue protein(s)",
           "residue_rows_a": int(rep.pro.x.size(0)), "residue_rows_b": int(sha.pro.x.size(0)), "rounds": ROUNDS, "steps_per_window": steps,
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
