"""Screening a ligand library against a PANEL of cached proteins (selectivity: every ligand against every target), per ligand batch:
  (a) Q calls of model.screen(ligands, enc, [q] * L)   — the route before screen_panel: the ligand tower runs Q times, the indexed
      fusion loads a protein's residue rows once per ligand
  (b) one model.screen_panel(ligands, enc)             — the ligand tower once, one protein-stationary fusion per step
on default ArchitectureDTI() in eval() under no_grad, Q synthetic proteins of 500 residues encoded once, fresh shuffled ligand batches
from a device-resident loader, L in {32, 1 024} x Q in {1, 15}.  The two legs alternate inside one process; timed like
tools/bench_screen.py (host clock around a window that ends in a device synchronise), median of the rounds and their spread
(max - min).  Also: max |a - b| of the two outputs on one batch, and the panel fusion's own kernel time (k_pair_panel + finish) per
step from glam_prof_* (a separate, untimed call), next to the indexed fusion's of leg (a).

usage: bench_panel.py [--L 32,1024] [--Q 1,15] [--steps N] [--rounds R] [--residues N] [--out FILE]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glam_amd import _lib, model
from glam_amd.data import Batch, DataLoader, synth_molecule, synth_protein

_opts = {"--L": "32,1024", "--Q": "1,15", "--steps": "12", "--rounds": "3", "--residues": "500", "--out": ""}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    if a not in _opts:
        sys.exit(__doc__)
    _opts[a] = _args.pop(0)
LS, QS = [int(v) for v in _opts["--L"].split(",")], [int(v) for v in _opts["--Q"].split(",")]
STEPS, ROUNDS, RES = int(_opts["--steps"]), int(_opts["--rounds"]), int(_opts["--residues"])
dev = torch.device("cuda")
torch.manual_seed(0)
net = model.ArchitectureDTI().to(dev).eval()
net.graphed_call = False
rng = np.random.default_rng(0)
proteins = [synth_protein(rng, RES, RES) for _ in range(max(QS))]
lines = []


def batches(loader):
    while True:                      # (every epoch is a fresh shuffle: no batch repeats)
        yield from loader


def window(step, feed, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step(next(feed))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


with torch.no_grad():
    for L in LS:
        library = [synth_molecule(rng) for _ in range(8 * L)]
        feed = batches(DataLoader(library, batch_size=L, shuffle=True, device=dev, resident=True))
        for Q in QS:
            enc = net.encode_proteins(Batch.from_data_list(proteins[:Q]).to(dev))
            index = [[q] * L for q in range(Q)]

            def by_screen(mol):
                return torch.stack([net.screen(mol, enc, index[q]) for q in range(Q)], 1)

            def by_panel(mol):
                return net.screen_panel(mol, enc)
            legs = {"a: Q x screen": by_screen, "b: screen_panel": by_panel}
            mol = next(feed)
            diff = (by_screen(mol) - by_panel(mol)).abs().max().item()
            times = {k: [] for k in legs}
            for k, step in legs.items():
                window(step, feed, 3)                                # warm-up of every shape of the window
            for _ in range(ROUNDS):
                for k, step in legs.items():                         # alternating: both legs see the same state of the box
                    times[k].append(window(step, feed, STEPS))
            kernels = {}
            for k, step in legs.items():
                with _lib.kernel_timer() as kt:
                    step(mol)
                    torch.cuda.synchronize()
                kernels[k] = kt.records()
            panel_us = sum(us for name, _g, us in kernels["b: screen_panel"] if "k_pair_panel" in name)
            indexed_us = sum(us for name, _g, us in kernels["a: Q x screen"] if "k_pair_" in name)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            a, b = med["a: Q x screen"], med["b: screen_panel"]
            lines.append(json.dumps({
                "workload": f"default ArchitectureDTI eval, L={L} ligands x Q={Q} proteins of {RES} residues, {STEPS} steps x {ROUNDS} rounds",
                "a_ms_per_batch": a * 1e3, "a_scores_per_s": L * Q / a, "a_spread_ms": spread["a: Q x screen"] * 1e3,
                "b_ms_per_batch": b * 1e3, "b_scores_per_s": L * Q / b, "b_spread_ms": spread["b: screen_panel"] * 1e3,
                "b_over_a_speedup": a / b, "b_beats_a_by_more_than_the_spread": bool(a - b > max(spread.values())),
                "rounds_ms": {k: [round(t * 1e3, 4) for t in v] for k, v in times.items()},
                "max_abs_diff_a_b": diff,
                "panel_fusion_kernels_us_per_step": panel_us / net.message_steps, "panel_fusion_kernels_us_per_batch": panel_us,
                "indexed_fusion_kernels_us_per_batch_leg_a": indexed_us,
                "all_glam_kernels_us_per_batch": {k: sum(r[2] for r in v) for k, v in kernels.items()},
                "glam_launches_per_batch": {k: len(v) for k, v in kernels.items()}}))
            print(lines[-1], flush=True)
            del enc
        del feed, library
        torch.cuda.empty_cache()
if _opts["--out"]:
    os.makedirs(os.path.dirname(os.path.abspath(_opts["--out"])), exist_ok=True)
    with open(_opts["--out"], "w") as f:
        f.write("\n".join(lines) + "\n")
