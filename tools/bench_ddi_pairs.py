"""Scoring the pairs of a drug-drug interaction set (the validation / test loops of src_2gi_ddi: both drugs of a pair are looked up in one
dictionary of molecule graphs, dataset.py:170-176): pairs / s of
  (a) model(mol1, mol2)            — both batches collated per chunk of pairs by DeviceDataset.collate (one launch each), both towers run
      on every copy; the model's graphed-call route is off (a pass never repeats a chunk)
  (b) enc = model.encode_drugs(all drugs) once, then model.score_pairs(enc, first, second) per chunk — no graph is collated per pair
on default ArchitectureDDI() in eval() under no_grad, Q synthetic molecules, P random pairs over them, chunks of C pairs.  One process, the
two legs alternate; timed with the host clock around a window that ends in a device synchronise, median of the rounds.  Also: the one-off
encode time, max |a - b| of the two outputs on one chunk, and the fusion ALONE at the chunk's shape — ops.pair_pool on the collated
(physically gathered) rows against ops.pair_pool_gather on the encoded rows, microseconds per call from glam_prof_* (separate, untimed calls).

usage: bench_ddi_pairs.py [--drugs Q] [--pairs P] [--chunk C[,C...]] [--rounds R]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glam_amd import _lib, model, ops
from glam_amd.data import Batch, DeviceDataset, synth_molecule

_opts = {"--drugs": "1024", "--pairs": "16384", "--chunk": "32,1024", "--rounds": "3"}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    if a not in _opts:
        sys.exit(__doc__)
    _opts[a] = _args.pop(0)
Q, P, ROUNDS = int(_opts["--drugs"]), int(_opts["--pairs"]), int(_opts["--rounds"])
CHUNKS = [int(c) for c in _opts["--chunk"].split(",")]
dev = torch.device("cuda")
torch.manual_seed(0)
net = model.ArchitectureDDI().to(dev).eval()
net.graphed_call = False
rng = np.random.default_rng(0)
drugs = [synth_molecule(rng) for _ in range(Q)]
first, second = rng.integers(0, Q, size=P), rng.integers(0, Q, size=P)
data = DeviceDataset(drugs, dev)
everything = Batch.from_data_list(drugs).to(dev)


def window(step, chunks):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for lo, hi in chunks:
        step(first[lo:hi], second[lo:hi])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fusion_us(call, names, reps=10):
    """Median over ``reps`` calls of the summed time of the kernels ``names`` of one call."""
    per_call = []
    for _ in range(reps):
        with _lib.kernel_timer() as kt:
            call()
            torch.cuda.synchronize()
        per_call.append(sum(us for name, _g, us in kt.records() if any(n in name for n in names)))
    return statistics.median(per_call)


with torch.no_grad():
    enc = net.encode_drugs(everything)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc = net.encode_drugs(everything)
    torch.cuda.synchronize()
    t_enc = time.perf_counter() - t0
    legs = {"a": lambda i1, i2: net(data.collate(i1), data.collate(i2)), "b": lambda i1, i2: net.score_pairs(enc, i1, i2)}
    for C in CHUNKS:
        chunks = [(lo, min(lo + C, P)) for lo in range(0, P, C)]
        pairs = chunks[-1][1]
        i1, i2 = first[:C], second[:C]
        diff = (legs["a"](i1, i2) - legs["b"](i1, i2)).abs().max().item()
        times = {k: [] for k in legs}
        for step in legs.values():
            window(step, chunks[:5] + chunks[-1:])               # warm-up of every shape of the window
        for _ in range(ROUNDS):
            for k, step in legs.items():                         # alternating: both legs see the same state of the machine
                times[k].append(window(step, chunks))
        # the fusion alone, at this chunk's shape: the rows of the last message step, gathered as a collated batch holds them
        m1, m2 = data.collate(i1), data.collate(i2)
        node_ptr = np.concatenate([[0], np.cumsum(data.ns)])
        rows_of = lambda ids: torch.from_numpy(np.concatenate([np.arange(node_ptr[q], node_ptr[q + 1]) for q in ids])).to(dev)   # noqa: E731
        g1, g2 = enc.rows1[-1].index_select(0, rows_of(i1)), enc.rows2[-1].index_select(0, rows_of(i2))
        sp1, sp2 = ops.segment_ptr(m1.batch, m1.num_graphs), ops.segment_ptr(m2.batch, m2.num_graphs)
        ix1, ix2 = ops.pair_index(i1, len(i1), Q), ops.pair_index(i2, len(i2), Q)
        ix1.on(dev), ix2.on(dev)
        same_max = torch.equal(ops.pair_pool(g1, g2, sp1, sp2)[:, 0], ops.pair_pool_gather(enc.rows1[-1], enc.rows2[-1], enc.sp, enc.sp, ix1, ix2)[:, 0])
        us_pool = fusion_us(lambda: ops.pair_pool(g1, g2, sp1, sp2), ("k_pair_max_partial", "k_pair_finish", "k_pair_pool_fwd"))
        us_gather = fusion_us(lambda: ops.pair_pool_gather(enc.rows1[-1], enc.rows2[-1], enc.sp, enc.sp, ix1, ix2), ("k_pair_gather",))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps({"workload": f"default ArchitectureDDI eval, {Q} drugs, {pairs} pairs in chunks of {C}, {ROUNDS} rounds",
                          "a_model_on_collated_chunks_pairs_per_s": pairs / med["a"], "b_score_pairs_pairs_per_s": pairs / med["b"],
                          "b_over_a_speedup": med["a"] / med["b"],
                          "a_ms_per_chunk": med["a"] / len(chunks) * 1e3, "b_ms_per_chunk": med["b"] / len(chunks) * 1e3,
                          "rounds_s": {k: [round(t, 4) for t in v] for k, v in times.items()},
                          "encode_drugs_ms_once": t_enc * 1e3, "max_abs_diff_a_b": diff,
                          "fusion_pair_pool_on_collated_rows_us": us_pool, "fusion_pair_pool_gather_us": us_gather,
                          "fusion_width": int(enc.rows1[-1].size(1)), "fusion_max_bit_equal": same_max}), flush=True)
