"""Shuffled DTI training over a protein set too large to hold in one batch: 1 000 synthetic proteins of 200 - 800
residues, every step other pairs AND other proteins, default ArchitectureDTI (pro_block="_GCNConv") in train(), forward + backward +
glam_amd.optim.Adam, at B = 32 / Qb = 32 and B = 256 / Qb = 64:
  (a) the refillable batch: ONE ResidentDTIRefillBatch, load(ids, launch=False) per step (host tables, one pinned copy), then
      GraphedTrainStep(SharedStep(model)) — one captured graph that holds both collates, the pair lists and the label gather;
  (b) what a trainer had before: eager forward_shared per step on a FRESH ligand batch, a FRESH batch of the step's distinct proteins
      (DeviceDataset.collate: one launch each) and a fresh ops.pair_index — code this change does not touch;
  (c) a GraphedTrainStep replaying ONE frozen load of a batch of the same capacity: the floor (a) pays its loads on top of.
A step's pairs name at most Qb proteins: B / Qb pairs of each of Qb drawn proteins, in shuffled order.  All legs alternate inside one
process; a window is timed by the host clock and ends in a device synchronise; reported: the median of the rounds and their min .. max.
Also per case: the share of phantom and filler residue rows, the three GCN launches' kernel times from the kernel timer (median over 10
eager steps), and layer.GCNConv(60, 60) forward + backward on one FRESH protein batch per call, inline route (ops.gcn_aggregate) against
the cached route (derived edge list + second index + norm on first sight), host clock, median of 10 fresh batches.

usage: bench_protein_refill.py [--rounds R] [--window SECONDS] [--proteins N] [--out FILE]"""
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glam_amd import _lib, data, layer, loss as glam_loss, model, ops, optim
from glam_amd.data import Data, DeviceDataset, synth_molecule, synth_protein
from glam_amd.graphs import GraphedTrainStep, padded_loss

_opts = {"--rounds": "5", "--window": "0.3", "--proteins": "1000", "--out": ""}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    _opts[a] = _args.pop(0)
ROUNDS, WINDOW, N_PRO = int(_opts["--rounds"]), float(_opts["--window"]), int(_opts["--proteins"])
CASES = [(32, 32), (256, 64)]
EPOCH, PER_PROTEIN = 48, 16
dev = torch.device("cuda")


class Fixed:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def loss_fn(out, b):
    return glam_loss.mse_loss(out.view(-1), b.y.view(-1))


def window(step, n, k0=0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        step(k0 + k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def graphed(net0, batch_of):
    step = model.SharedStep(copy.deepcopy(net0))
    stepper = GraphedTrainStep(step, optim.Adam(step.parameters(), lr=1e-3), padded_loss(loss_fn))
    return lambda k: stepper(batch_of(k))


def eager(net0, batch_of):
    step = model.SharedStep(copy.deepcopy(net0))
    opt = optim.Adam(step.parameters(), lr=1e-3)

    def run(k):
        b = batch_of(k)
        opt.zero_grad(set_to_none=True)
        loss_fn(step(b), b).backward()
        opt.step()
    return run


def measure(workload, legs, extra):
    steps = {}
    for k, step in legs.items():
        window(step, 4)                                   # first visits, the capture, code objects
        steps[k] = max(5, min(400, int(WINDOW / window(step, 3, 4))))
    times, at = {k: [] for k in legs}, {k: 7 for k in legs}
    for _ in range(ROUNDS):
        for k, step in legs.items():                      # alternating
            times[k].append(window(step, steps[k], at[k]))
            at[k] += steps[k]
    med = {k: statistics.median(v) for k, v in times.items()}
    lo, hi = {k: min(v) for k, v in times.items()}, {k: max(v) for k, v in times.items()}
    ms = lambda v: round(v * 1e3, 4)                       # noqa: E731
    row = {"workload": workload, "rounds": ROUNDS, "steps_per_window": steps, "median_ms": {k: ms(v) for k, v in med.items()},
           "min_max_ms": {k: [ms(lo[k]), ms(hi[k])] for k in legs},
           "a_over_b": round(med["a"] / med["b"], 3), "a_over_b_range": [round(lo["a"] / hi["b"], 3), round(hi["a"] / lo["b"], 3)],
           "a_minus_c_ms": ms(med["a"] - med["c"]), "a_minus_c_range_ms": [ms(lo["a"] - hi["c"]), ms(hi["a"] - lo["c"])]}
    row.update(extra)
    row["peak_mem_mib"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(row), flush=True)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return json.dumps(row)


def gcn_kernel_us(net0, batch, lists):
    step = model.SharedStep(copy.deepcopy(net0))
    per = {}
    for ids in lists[:10]:
        batch.load(ids)
        with _lib.kernel_timer(16384) as kt:
            loss_fn(step(batch)[:batch.num_real_graphs], batch).backward()
            torch.cuda.synchronize()
        for name, _grid, us in kt.records():
            if name.startswith("k_gcn"):
                per.setdefault(name, []).append(us)
    return {k: round(statistics.median(v), 2) for k, v in per.items()}


def conv_first_sight(proteins, lists, second):
    """``GCNConv(60, 60)`` forward + backward on a fresh protein batch per call: ms by the host clock, inline against cached."""
    torch.manual_seed(1)
    conv = layer.GCNConv(60, 60).to(dev)
    out = {}
    for route in ("inline", "cached", "inline", "cached"):
        ts = []
        for ids in lists[:10]:
            b = proteins.collate(np.unique(second[ids]))
            if route == "inline":
                ops.mark_gcn_inline(b.edge_index)
            x = torch.randn(b.x.size(0), 60, device=dev, requires_grad=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with ops.weight_scope():
                conv(x, b.edge_index).sum().backward()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[route] = round(statistics.median(ts) * 1e3, 4)      # (the second pass of each route: code objects loaded)
    return out


rng = np.random.default_rng(2024)
ligs = [Data(m.x, m.edge_index, m.edge_attr) for m in (synth_molecule(rng) for _ in range(2048))]
pros = [Data(p.x, p.edge_index, p.edge_attr) for p in (synth_protein(rng, 200, 800) for _ in range(N_PRO))]
ligands, proteins = DeviceDataset(ligs, dev), DeviceDataset(pros, dev)
del ligs, pros
n_pairs = PER_PROTEIN * N_PRO
second = rng.permutation(np.repeat(np.arange(N_PRO), PER_PROTEIN))
first = rng.integers(0, ligands.n, n_pairs)
y = rng.standard_normal((n_pairs, 1)).astype(np.float32)
y_dev = torch.from_numpy(y).to(dev)
pairs = data.ResidentPairs(first, second, y, dev)
of_protein = [np.flatnonzero(second == q) for q in range(N_PRO)]

lines = []
for B, Qb in CASES:
    torch.manual_seed(0)
    ops.manual_seed(0, dev)
    net0 = model.ArchitectureDTI().to(dev).train()
    per = B // Qb
    lists = [np.concatenate([rng.permutation(of_protein[q])[:per] for q in rng.permutation(N_PRO)[:Qb]])[rng.permutation(B)] for _ in range(EPOCH)]
    m = int(proteins.ns.max())
    make = lambda: pairs.dti_batch(ligands, proteins, B, phantom_rows=int(ligands.ns.max()), protein_slots=Qb, protein_phantom_rows=m)  # noqa: E731
    ba, bc, probe = make(), make(), make()
    bc.load(lists[0])

    def fresh(k):
        ids = lists[k % EPOCH]
        u, keys = np.unique(second[ids], return_inverse=True)
        return Fixed(mol=ligands.collate(first[ids]), pro=proteins.collate(u), index=ops.pair_index(keys, B, len(u)),
                     y=y_dev[torch.from_numpy(ids).to(dev)])
    legs = {"a": graphed(net0, lambda k: ba.load(lists[k % EPOCH], launch=False)), "b": eager(net0, fresh), "c": graphed(net0, lambda k: bc)}
    n_cap = ba.pro.capacity[0]
    real = float(np.mean([proteins.ns[np.unique(second[ids])].sum() for ids in lists]))
    filler = float(np.mean([proteins.ns[s[U:]].sum() for s, _keys, U in (data.protein_slot_ids(second[ids], proteins.ns, Qb) for ids in lists)]))
    extra = {"gcn_kernel_us": gcn_kernel_us(net0, probe, lists),
             "gcnconv_fresh_batch_ms": conv_first_sight(proteins, lists, second),
             "protein_padding": {"N_cap": int(n_cap), "phantom_graphs": int(ba.pro.num_phantom_graphs), "mean_real_rows": round(real, 1),
                                 "mean_filler_rows": round(filler, 1), "phantom_and_filler_share": round(1 - real / n_cap, 4),
                                 "mean_distinct_proteins": round(float(np.mean([np.unique(second[i]).size for i in lists])), 2)}}
    lines.append(measure(f"default ArchitectureDTI train(), fwd+bwd+Adam, shuffled: B={B} pairs, Qb={Qb} protein slots, {N_PRO} proteins of "
                         f"200-800 residues, {n_pairs} pairs", legs, extra))
    del legs, ba, bc, probe, net0

if _opts["--out"]:
    with open(_opts["--out"], "w") as f:
        f.write("\n".join(lines) + "\n")
