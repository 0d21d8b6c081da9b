"""Screening a ligand library against ONE protein (the LIT-PCBA walk, src_2gi_dti_scr/dataset.py:297-318): ligands / s of
  (a) model(ligands, replicated protein batch)   — one copy of the protein per pair, as the reference collates it; the replicated batch is
      collated and staged ONCE, outside the timing, and the model's graphed-call route is off (a walk never repeats a batch, the route
      would only add a fingerprint and its read-back per call): both favour (a)
  (b) enc = model.encode_proteins(protein) once, then model.screen(ligands, enc)
on default ArchitectureDTI() in eval() under no_grad, one 500-residue protein, fresh shuffled ligand batches from a device-resident
loader, B = 32 and B = 1 024.  The two legs alternate inside one process; timed like tools/bench_dti.py (host clock around a window
that ends in a device synchronise), median of the rounds.  Also: max |a - b| of the two outputs on one batch, and the indexed
fusion's own kernel time per screen() call from glam_prof_* (a separate, untimed call).

usage: bench_screen.py [B ...] [--steps N] [--rounds R] [--residues N]"""
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

_opts = {"--steps": "24", "--rounds": "3", "--residues": "500"}
_args, _sizes = sys.argv[1:], []
while _args:
    a = _args.pop(0)
    if a in _opts:
        _opts[a] = _args.pop(0)
    else:
        _sizes.append(int(a))
SIZES = _sizes or [32, 1024]
STEPS, ROUNDS, RES = int(_opts["--steps"]), int(_opts["--rounds"]), int(_opts["--residues"])
dev = torch.device("cuda")
torch.manual_seed(0)
net = model.ArchitectureDTI().to(dev).eval()
net.graphed_call = False
rng = np.random.default_rng(0)
protein = synth_protein(rng, RES, RES)


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
    for B in SIZES:
        library = [synth_molecule(rng) for _ in range(8 * B)]
        feed = batches(DataLoader(library, batch_size=B, shuffle=True, device=dev, resident=True))
        replicated = Batch.from_data_list([protein] * B).to(dev)
        enc = net.encode_proteins(Batch.from_data_list([protein]).to(dev))
        legs = {"a: model(ligands, replicated)": lambda mol: net(mol, replicated), "b: screen(ligands, enc)": lambda mol: net.screen(mol, enc)}
        mol = next(feed)
        diff = (net(mol, replicated) - net.screen(mol, enc)).abs().max().item()
        times = {k: [] for k in legs}
        for k, step in legs.items():
            window(step, feed, 5)                                # warm-up of every shape of the window
        for _ in range(ROUNDS):
            for k, step in legs.items():                         # alternating: both legs see the same state of the box
                times[k].append(window(step, feed, STEPS))
        t0 = time.perf_counter()
        net.encode_proteins(Batch.from_data_list([protein]).to(dev))
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        with _lib.kernel_timer() as kt:
            net.screen(mol, enc)
            torch.cuda.synchronize()
        recs = kt.records()
        fusion_us = sum(us for name, _g, us in recs if "k_pair_" in name)
        med = {k: statistics.median(v) for k, v in times.items()}
        a, b = med["a: model(ligands, replicated)"], med["b: screen(ligands, enc)"]
        print(json.dumps({"workload": f"default ArchitectureDTI eval, B={B} ligands x one {RES}-residue protein, {STEPS} steps x {ROUNDS} rounds",
                          "a_ms_per_step": a * 1e3, "a_ligands_per_s": B / a, "b_ms_per_step": b * 1e3, "b_ligands_per_s": B / b,
                          "b_over_a_speedup": a / b, "rounds_ms": {k: [round(t * 1e3, 4) for t in v] for k, v in times.items()},
                          "encode_proteins_ms_once": t_enc * 1e3, "max_abs_diff_a_b": diff,
                          "indexed_fusion_kernels_us_per_call": fusion_us, "all_glam_kernels_us_per_screen_call": sum(r[2] for r in recs),
                          "glam_launches_per_screen_call": len(recs)}), flush=True)
        del replicated, feed, library
        torch.cuda.empty_cache()
