"""What the interaction maps of explain.explain_pair cost, and what the route a user had before them costs: ms per call of
  (a) the score alone              — model.screen(ligands, enc) / model.score_pairs(enc, first, second)
  (b) explain.explain_pair(...)    — the same pass plus ONE ops.pair_map launch per message step (both marginals of every pair)
  (c) the score plus a torch loop  — the same pass, and per pair and step S = x1[seg] @ x2[seg].T with .max(1), .argmax(1), .mean(1)
      both ways, on the same rows the kernel reads (the only way to the maps without ops.pair_map)
on default ArchitectureDTI() against ONE protein of 500 residues at 32 and 1 024 ligands, and on default ArchitectureDDI() at 1 024 pairs
over 1 024 drugs of 12-28 atoms; eval() under no_grad.  One process, the legs alternate within a round; timed with the host clock around
a window of calls that ends in a device synchronise; median and spread (min .. max) of the rounds.  Also: the k_pair_map launch alone,
microseconds from glam_prof_* (separate, untimed calls), and (b) against (c) over EVERY step: whether all maxima and means agree to 1e-4
(a matmul sums the channels in another order than the fmaf chain), and the share of rows whose arg is the same row (near-ties may differ).

usage: bench_pair_map.py [--ligands L[,L...]] [--residues N] [--pairs P] [--drugs Q] [--rounds R] [--calls K] [--out FILE]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glam_amd import _lib, explain, model
from glam_amd.data import Batch, synth_batch, synth_molecule, synth_protein

_opts = {"--ligands": "32,1024", "--residues": "500", "--pairs": "1024", "--drugs": "1024", "--rounds": "5", "--calls": "10",
         "--out": os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pair_map_bench.txt")}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    if a not in _opts:
        sys.exit(__doc__)
    _opts[a] = _args.pop(0)
LIGANDS = [int(c) for c in _opts["--ligands"].split(",")]
NRES, P, Q, ROUNDS, CALLS = (int(_opts[k]) for k in ("--residues", "--pairs", "--drugs", "--rounds", "--calls"))
dev = torch.device("cuda")
lines = []


def torch_maps(x1, x2, bounds1, bounds2, a, b):
    """Route (c) for one step: per pair the score matrix and its two marginals (the args as rows of the other matrix), as six lists."""
    out = []
    for i in range(len(a)):
        m0, p0 = bounds1[a[i]], bounds2[b[i]]
        S = x1[m0:bounds1[a[i] + 1]] @ x2[p0:bounds2[b[i] + 1]].T
        out.append((S.max(1).values, S.argmax(1) + p0, S.mean(1), S.max(0).values, S.argmax(0) + m0, S.mean(0)))
    return out


def window(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e3


def measure(workload, legs, agree):
    for step in legs.values():
        step()                                                   # warm-up of every shape of the window
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, step in legs.items():                             # alternating: the legs see the same state of the machine
            times[k].append(window(step))
    with _lib.kernel_timer() as kt:
        legs["b"]()
        torch.cuda.synchronize()
    maps_us = [us for name, _g, us in kt.records() if name == "k_pair_map"]
    row = {"workload": workload, "rounds": ROUNDS, "calls_per_window": CALLS}
    for k, name in (("a", "a_score_alone"), ("b", "b_explain_pair"), ("c", "c_score_plus_torch_loop")):
        row[name + "_ms"] = {"median": round(statistics.median(times[k]), 3), "min": round(min(times[k]), 3), "max": round(max(times[k]), 3)}
    row["k_pair_map_us_per_launch"] = [round(u, 1) for u in maps_us]
    row["b_and_c_max_mean_agree_every_step"], row["b_and_c_same_arg_share"] = agree
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)


def agreement(maps, loops):
    """The kernel's maps against the loop's, over every step -> (all maxima and means within 1e-4, share of rows with the same arg)."""
    close, same, rows = True, 0, 0
    for pm, loop in zip(maps, loops):
        cat = [torch.cat([t[k] for t in loop]) for k in range(6)]
        close = close and all(torch.allclose(got, want, rtol=1e-4, atol=1e-4)
                              for got, want in ((pm.max1, cat[0]), (pm.mean1, cat[2]), (pm.max2, cat[3]), (pm.mean2, cat[5])))
        same += int((pm.arg1 == cat[1]).sum()) + int((pm.arg2 == cat[4]).sum())
        rows += pm.arg1.numel() + pm.arg2.numel()
    return bool(close and len(maps) == len(loops)), round(same / max(rows, 1), 6)


with torch.no_grad():
    # ---- DTI: one target, a batch of ligands ----
    torch.manual_seed(0)
    dti = model.ArchitectureDTI().to(dev).eval()
    dti.graphed_call = False
    enc = dti.encode_proteins(Batch.from_data_list([synth_protein(np.random.default_rng(0), NRES, NRES)]).to(dev))
    pro_bounds = [0, NRES]
    for L in LIGANDS:
        mb = synth_batch(L, seed=1).to(dev)
        lig_bounds = np.concatenate([[0], np.cumsum(np.bincount(mb.batch.cpu().numpy(), minlength=L))]).tolist()
        ids, zeros = list(range(L)), [0] * L

        def leg_c():
            out, contacts, fusion, rows, msp, index = dti._screen("bench", mb, enc, None, True)
            return out, [torch_maps(x, r, lig_bounds, pro_bounds, ids, zeros) for x, r in zip(rows, enc.rows)]

        ex = explain.explain_pair(dti, mb, enc)
        measure(f"default ArchitectureDTI eval, 1 protein of {NRES} residues, {L} ligands, {dti.message_steps} steps",
                {"a": lambda: dti.screen(mb, enc), "b": lambda: explain.explain_pair(dti, mb, enc), "c": leg_c},
                agreement(ex.maps, leg_c()[1]))
    # ---- DDI: pairs over drugs held once ----
    torch.manual_seed(0)
    ddi = model.ArchitectureDDI().to(dev).eval()
    ddi.graphed_call = False
    rng = np.random.default_rng(0)
    denc = ddi.encode_drugs(Batch.from_data_list([synth_molecule(rng) for _ in range(Q)]).to(dev))
    first, second = rng.integers(0, Q, size=P), rng.integers(0, Q, size=P)
    bounds = denc.sp.ptr.cpu().tolist()

    def ddi_c():
        out = ddi.score_pairs(denc, first, second, return_argmax=True)
        return out, [torch_maps(r1, r2, bounds, bounds, first, second) for r1, r2 in zip(denc.rows1, denc.rows2)]

    ex = explain.explain_pair(ddi, denc, first, second)
    measure(f"default ArchitectureDDI eval, {Q} drugs of 12-28 atoms, {P} pairs, {ddi.message_steps} steps",
            {"a": lambda: ddi.score_pairs(denc, first, second), "b": lambda: explain.explain_pair(ddi, denc, first, second), "c": ddi_c},
            agreement(ex.maps, ddi_c()[1]))

os.makedirs(os.path.dirname(os.path.abspath(_opts["--out"])), exist_ok=True)
with open(_opts["--out"], "w") as f:
    f.write("# tools/bench_pair_map.py " + " ".join(f"{k} {v}" for k, v in _opts.items() if k != "--out") + "\n" + "\n".join(lines) + "\n")
