"""Training steps on SHUFFLED pairs — every step other pair ids, as every real DTI / DDI epoch has them — on the shapes of
tools/bench_dti_shared.py and tools/bench_ddi_shared.py:
  (a) the resident pair batch: ONE ResidentDTIBatch / ResidentDDIBatch, load(ids, launch=False) per step (host table, one pinned copy),
      then GraphedTrainStep(SharedStep(model)) — one captured graph that holds the loads' launches.  "a load_many": the epoch's tables
      uploaded at once, load(step=i) per step (a device-to-device copy);
  (b) what a trainer had before: eager forward_shared per step on a FRESH ligand batch (DeviceDataset.collate of the step's ligands: one
      launch, the fastest fresh batch there is) and a fresh ops.pair_index of the step's proteins — DDI: fresh indices into the held drugs;
  (c) a GraphedTrainStep replaying ONE fixed batch of the same composition over and over: what the shared benchmarks time, and the floor
      (a) pays its load on top of.
Default models in train() (RReLU, Dropout(0.2)): forward + backward + glam_amd.optim.Adam; every leg has its own copy of the same initial
model and its own optimizer.  All legs alternate inside one process; a window is timed by the host clock and ends in a device synchronise;
reported: the median of the rounds and their min .. max, (a) / (b) and (a) - (c) from the medians with the range the rounds' extremes
give.  Also per case: the time of glam_pair_list_load (and, DTI, of the padded collate) per launch from the kernel timer — median of 20
eager loads — and the padding share: phantom node rows over N_cap and phantom pair slots over P.

usage: bench_pair_shuffle.py [--rounds R] [--window SECONDS] [--residues N] [--out FILE]"""
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glam_amd import _lib, data, loss as glam_loss, model, ops, optim
from glam_amd.data import Batch, Data, DeviceDataset, synth_molecule, synth_protein
from glam_amd.graphs import GraphedTrainStep, padded_loss

_opts = {"--rounds": "5", "--window": "0.3", "--residues": "500", "--out": ""}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    _opts[a] = _args.pop(0)
ROUNDS, WINDOW, RES = int(_opts["--rounds"]), float(_opts["--window"]), int(_opts["--residues"])
DTI_CASES, DDI_CASES = [(32, 1), (32, 8), (1024, 1)], [(1024, 256), (1024, 1024)]
EPOCH = 64                      # distinct shuffled id lists a leg cycles through
dev = torch.device("cuda")


class Fixed:
    """A batch of leg (b) / (c): plain fields, as a trainer holds them."""

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


def kernel_us(load, lists):
    per = {}
    for ids in lists[:20]:
        with _lib.kernel_timer() as kt:
            load(ids)
        for name, _grid, us in kt.records():
            per.setdefault(name.split("<")[0], []).append(us)
    torch.cuda.synchronize()
    return {k: round(statistics.median(v), 2) for k, v in per.items()}


def measure(workload, legs, extra):
    steps = {}
    for k, step in legs.items():
        window(step, 4)                                   # first visits, the capture, code objects
        steps[k] = max(5, min(400, int(WINDOW / window(step, 3, 4))))
    times = {k: [] for k in legs}
    at = {k: 7 for k in legs}
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
           "a_minus_c_ms": ms(med["a"] - med["c"]), "a_minus_c_range_ms": [ms(lo["a"] - hi["c"]), ms(hi["a"] - lo["c"])],
           "a_load_many_minus_c_ms": ms(med["a load_many"] - med["c"])}
    row.update(extra)
    row["peak_mem_mib"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(row), flush=True)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return json.dumps(row)


def graphed(net0, batch_of):
    """Leg (a) / (c): a stepper over a copy of ``net0``; ``batch_of(k)`` hands it step k's batch."""
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


lines = []
for B, Q in DTI_CASES:
    torch.manual_seed(0)
    ops.manual_seed(0, dev)
    rng = np.random.default_rng(B * 31 + Q)
    net0 = model.ArchitectureDTI().to(dev).train()
    n_lig, n_pairs = max(4 * B, 256), 16 * B
    ligs = [Data(m.x, m.edge_index, m.edge_attr) for m in (synth_molecule(rng) for _ in range(n_lig))]
    dd = DeviceDataset(ligs, dev)
    pro = Batch.from_data_list([synth_protein(rng, RES, RES) for _ in range(Q)]).to(dev)
    first, second = rng.integers(0, n_lig, n_pairs), rng.integers(0, Q, n_pairs)
    y = rng.standard_normal((n_pairs, 1)).astype(np.float32)
    y_dev = torch.from_numpy(y).to(dev)
    pairs = data.ResidentPairs(first, second, y, dev)
    lists = [rng.permutation(n_pairs)[:B] for _ in range(EPOCH)]
    make = lambda: pairs.dti_batch(dd, pro, B, phantom_rows=int(dd.ns.max()))          # noqa: E731
    ba, bm, probe = make(), make(), make()
    bm.load_many(lists)

    def fresh(k):
        ids = lists[k % EPOCH]
        return Fixed(mol=dd.collate(first[ids]), pro=pro, index=ops.pair_index(second[ids], B, Q), y=y_dev[torch.from_numpy(ids).to(dev)])
    fixed = fresh(0)
    legs = {"a": graphed(net0, lambda k: ba.load(lists[k % EPOCH], launch=False)),
            "a load_many": graphed(net0, lambda k: bm.load(step=k % EPOCH, launch=False)),
            "b": eager(net0, fresh), "c": graphed(net0, lambda k: fixed)}
    n_cap = ba.mol.capacity[0]
    real = float(np.mean([dd.ns[first[ids]].sum() for ids in lists]))
    extra = {"kernel_us_per_launch": kernel_us(probe.load, lists),
             "padding": {"N_cap": int(n_cap), "mean_real_nodes": round(real, 1), "phantom_node_share": round(1 - real / n_cap, 4),
                         "pair_slots": int(ba.index.P), "phantom_pair_slots": int(ba.index.P - B),
                         "phantom_slot_share": round(1 - B / ba.index.P, 4)}}
    lines.append(measure(f"default ArchitectureDTI train(), fwd+bwd+Adam, shuffled: B={B} pairs of {n_pairs} over {n_lig} ligands x {Q} "
                         f"resident {RES}-residue protein(s)", legs, extra))
    del legs, ba, bm, probe, fixed, dd, pairs, net0

for P, Q in DDI_CASES:
    torch.manual_seed(0)
    ops.manual_seed(0, dev)
    rng = np.random.default_rng(P * 7919 + Q)
    net0 = model.ArchitectureDDI().to(dev).train()
    drugs = Batch.from_data_list([synth_molecule(rng) for _ in range(Q)]).to(dev)
    n_pairs = 16 * P
    first, second = rng.integers(0, Q, n_pairs), rng.integers(0, Q, n_pairs)
    y = rng.standard_normal((n_pairs, 1)).astype(np.float32)
    y_dev = torch.from_numpy(y).to(dev)
    pairs = data.ResidentPairs(first, second, y, dev)
    lists = [rng.permutation(n_pairs)[:P] for _ in range(EPOCH)]
    ba, bm, probe = (pairs.ddi_batch(drugs, batch_size=P) for _ in range(3))
    bm.load_many(lists)

    def fresh(k):
        ids = lists[k % EPOCH]
        return Fixed(mol1=drugs, mol2=drugs, first=ops.pair_index(first[ids], P, Q, name="first", over="drugs"),
                     second=ops.pair_index(second[ids], P, Q, name="second", over="drugs"), y=y_dev[torch.from_numpy(ids).to(dev)])
    fixed = fresh(0)
    legs = {"a": graphed(net0, lambda k: ba.load(lists[k % EPOCH], launch=False)),
            "a load_many": graphed(net0, lambda k: bm.load(step=k % EPOCH, launch=False)),
            "b": eager(net0, fresh), "c": graphed(net0, lambda k: fixed)}
    extra = {"kernel_us_per_launch": kernel_us(probe.load, lists), "padding": {"pair_slots": P, "phantom_pair_slots": 0, "phantom_slot_share": 0.0}}
    lines.append(measure(f"default ArchitectureDDI train(), fwd+bwd+Adam, shuffled: P={P} pairs of {n_pairs} over {Q} resident drugs "
                         "(one Batch, both towers)", legs, extra))
    del legs, ba, bm, probe, fixed, pairs, net0

if _opts["--out"]:
    with open(_opts["--out"], "w") as f:
        f.write("\n".join(lines) + "\n")
