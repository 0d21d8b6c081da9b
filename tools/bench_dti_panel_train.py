"""Training steps of the two-tower model on a ligand x protein LABEL TABLE (a selectivity panel: every ligand measured on every target):
  (a) model.forward_shared(expanded ligands, proteins, index)  — the proteins once, but one ligand graph per PAIR (ligand l repeated Qs
      times) and the indexed fusion with its backward: the only training route before forward_panel (the yardstick)
  (b) model.forward_panel(ligands, proteins, plan=plan)        — both towers once, the protein-stationary panel fusion and its one-launch
      backward (glam_pair_pool_panel_bwd), the head over the same L * Qs rows
on default ArchitectureDTI() in train() (RReLU, Dropout(0.2)): forward + backward + glam_amd.optim.Adam on one cached batch, each leg
eager and under GraphedTrainStep (neither call has a graphed-call route of its own).  Cases L:Qs — 32 x 15, 64 x 15 and 1 024 x 1 by
default — against Qs distinct proteins of 500 residues.  All legs alternate inside one process (every leg sees the same state of the
box); a window is timed by the host clock and ends in a device synchronise; reported: the median of the rounds and their min .. max.
Every leg has its own copy of the same initial model and its own optimizer.  Also: max |a - b| of the two outputs in eval() on the timed
batch, and the fusion backward's own time per launch from the kernel timer (k_pair_shared_bwd of (a), k_pair_panel_bwd of (b): median
and min .. max over the launches of a few eager steps; message_steps launches a step).

usage: bench_dti_panel_train.py [--rounds R] [--window SECONDS] [--residues N] [--out FILE] [L:Qs ...]        (default 32:15 64:15 1024:1)"""
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glam_amd import _lib, loss as glam_loss, model, ops, optim
from glam_amd.data import Batch, synth_molecule, synth_protein
from glam_amd.graphs import GraphedTrainStep

_opts = {"--rounds": "5", "--window": "0.3", "--residues": "500", "--out": ""}
_args, _cases = sys.argv[1:], []
while _args:
    a = _args.pop(0)
    if a in _opts:
        _opts[a] = _args.pop(0)
    else:
        _cases.append(tuple(int(v) for v in a.split(":")))
CASES = _cases or [(32, 15), (64, 15), (1024, 1)]
ROUNDS, WINDOW, RES = int(_opts["--rounds"]), float(_opts["--window"]), int(_opts["--residues"])
if ROUNDS < 3:
    sys.exit("bench_dti_panel_train.py: at least 3 rounds")
dev = torch.device("cuda")
rng = np.random.default_rng(0)


class Table:
    def __init__(self, mol, pro, y, index=None, plan=None):
        self.mol, self.pro, self.y, self.index, self.plan = mol, pro, y, index, plan


class Shared(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, b):
        return self.net.forward_shared(b.mol, b.pro, b.index)


class Panel(Shared):
    def forward(self, b):
        return self.net.forward_panel(b.mol, b.pro, plan=b.plan)


def loss_fn(out, b):
    return glam_loss.mse_loss(out.view(-1), b.y)


def make_leg(wrapper, net0, batch, graphed):
    mod = wrapper(copy.deepcopy(net0))
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


def kernel_us(step, kernel, steps=3):
    """The durations of ``kernel``'s launches over ``steps`` eager steps, from the per-launch kernel timer."""
    us = []
    for _ in range(steps):
        with _lib.kernel_timer() as kt:
            step()
            torch.cuda.synchronize()
        us += [r[2] for r in kt.records() if r[0].startswith(kernel)]          # (a template launch is recorded with its arguments)
    if not us:
        return {"launches_per_step": 0}
    return {"launches_per_step": len(us) // steps, "median_us": round(statistics.median(us), 2), "min_max_us": [round(min(us), 2), round(max(us), 2)]}


lines = []
for L, Qs in CASES:
    torch.manual_seed(0)
    ops.manual_seed(0, dev)
    net0 = model.ArchitectureDTI().to(dev).train()
    proteins = [synth_protein(rng, RES, RES) for _ in range(Qs)]
    ligands = [synth_molecule(rng) for _ in range(L)]
    y = torch.randn(L * Qs, device=dev)
    pro = Batch.from_data_list(proteins).to(dev)
    # (a): ligand l repeated Qs times, pair l * Qs + j against protein j — the rows of (b)'s table, in its order
    sha = Table(Batch.from_data_list([ligands[l] for l in range(L) for _ in range(Qs)]).to(dev), pro, y,
                index=ops.pair_index(list(range(Qs)) * L, L * Qs, Qs))
    pan = Table(Batch.from_data_list(ligands).to(dev), pro, y, plan=ops.panel_plan([RES] * Qs))
    with torch.no_grad():
        ev = copy.deepcopy(net0).eval()
        diff = (ev.forward_shared(sha.mol, sha.pro, sha.index).view(L, Qs, -1) - ev.forward_panel(pan.mol, pan.pro, plan=pan.plan)).abs().max().item()
        del ev
    legs = {"a eager": make_leg(Shared, net0, sha, False), "b eager": make_leg(Panel, net0, pan, False),
            "a graphed": make_leg(Shared, net0, sha, True), "b graphed": make_leg(Panel, net0, pan, True)}
    steps = {}
    for k, step in legs.items():
        window(step, 4)                                   # first visits, the capture, code objects
        steps[k] = max(5, min(400, int(WINDOW / window(step, 3))))
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, step in legs.items():                      # alternating
            times[k].append(window(step, steps[k]))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = {"workload": f"default ArchitectureDTI train(), fwd+bwd+Adam, table of {L} ligands x {Qs} distinct {RES}-residue protein(s)",
           "ligand_graphs_a": L * Qs, "ligand_graphs_b": L, "rounds": ROUNDS, "steps_per_window": steps,
           "median_ms": {k: round(v * 1e3, 4) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)] for k, v in times.items()},
           "a_over_b_eager": round(med["a eager"] / med["b eager"], 3), "a_over_b_graphed": round(med["a graphed"] / med["b graphed"], 3),
           "fusion_backward": {"a k_pair_shared_bwd": kernel_us(legs["a eager"], "k_pair_shared_bwd"),
                               "b k_pair_panel_bwd": kernel_us(legs["b eager"], "k_pair_panel_bwd")},
           "max_abs_diff_a_b_eval": diff, "peak_mem_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)
    del legs, sha, pan, net0
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
if _opts["--out"]:
    with open(_opts["--out"], "w") as f:
        f.write("\n".join(lines) + "\n")
