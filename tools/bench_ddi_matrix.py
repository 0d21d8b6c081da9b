"""The whole drug x drug table of a trained DDI model ("all partners of every drug"): Q x Q ordered pairs over Q drugs encoded once
(model.encode_drugs), scored by
  (a) model.score_pairs(enc, first, second) over all Q^2 pairs in chunks of C pairs — host index lists pushed through the listed-pairs
      call, the route before score_matrix; C = 1 024 and C = 65 536 (the larger chunk is the fair opponent: fewer, fuller launches)
  (b) model.score_matrix(enc) — one second-side-stationary fusion per step over the whole table, the head in bounded blocks
on default ArchitectureDDI() in eval() under no_grad, Q synthetic molecules of 12-28 atoms.  One process, the legs alternate; timed with
the host clock around a window that ends in a device synchronise, median of the rounds, spread = max - min of a leg's rounds.  Also: peak
device memory of (a) at the largest chunk and of (b) (torch's allocator, above what the encoding holds), max |a - b| of the outputs, the
mean lane fill of the plan's chunks (and of the panel's chunks over the same drugs), and the fusion ALONE on the rows of the last message
step — ops.pair_pool_gather on all Q^2 pairs, ops.pair_pool_panel on the drug rows (one drug per chunk: what the packed kernel must
beat), ops.pair_pool_grid — microseconds per call from glam_prof_* (separate, untimed calls; median and min - max of the repeats).

usage: bench_ddi_matrix.py [--drugs Q] [--chunk C[,C...]] [--rounds R]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glam_amd import _lib, model, ops
from glam_amd.data import Batch, synth_molecule

_opts = {"--drugs": "1024", "--chunk": "1024,65536", "--rounds": "3"}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    if a not in _opts:
        sys.exit(__doc__)
    _opts[a] = _args.pop(0)
Q, ROUNDS = int(_opts["--drugs"]), int(_opts["--rounds"])
CHUNKS = [int(c) for c in _opts["--chunk"].split(",")]
dev = torch.device("cuda")
torch.manual_seed(0)
net = model.ArchitectureDDI().to(dev).eval()
net.graphed_call = False
rng = np.random.default_rng(0)
everything = Batch.from_data_list([synth_molecule(rng) for _ in range(Q)]).to(dev)
first, second = np.repeat(np.arange(Q), Q), np.tile(np.arange(Q), Q)          # row-major: pair i * Q + j = (i, j)
P = Q * Q


def listed(C, keep=False):
    """Leg (a): every pair through score_pairs, C at a time.  ``keep``: the outputs as one [Q, Q, out_dim] table."""
    outs = []
    for lo in range(0, P, C):
        o = net.score_pairs(enc, first[lo:lo + C], second[lo:lo + C])
        if keep:
            outs.append(o)
    return torch.cat(outs).view(Q, Q, -1) if keep else None


def window(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def peak_mib(step):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def fusion_us(call, names, reps=7):
    """Over ``reps`` calls: the summed time of the kernels ``names`` of one call -> (median, min, max)."""
    per_call = []
    for _ in range(reps):
        with _lib.kernel_timer() as kt:
            call()
            torch.cuda.synchronize()
        per_call.append(sum(us for name, _g, us in kt.records() if any(n in name for n in names)))
    return [round(statistics.median(per_call), 1), round(min(per_call), 1), round(max(per_call), 1)]


with torch.no_grad():
    enc = net.encode_drugs(everything)
    table = net.score_matrix(enc)                                # the first matrix call: the one read-back, the sums, the plan
    plan = enc.grid(None)
    legs = {f"a: score_pairs, chunks of {C}": (lambda C=C: listed(C)) for C in CHUNKS}
    legs["b: score_matrix"] = lambda: net.score_matrix(enc)
    diff = (listed(CHUNKS[-1], keep=True) - table).abs().max().item()
    times = {k: [] for k in legs}
    for step in legs.values():
        step()                                                   # warm-up of every shape
    for _ in range(ROUNDS):
        for k, step in legs.items():                             # alternating: every leg sees the same state of the machine
            times[k].append(window(step))
    peaks = {k: round(peak_mib(step), 1) for k, step in list(legs.items())[-2:]}
    # the fusion alone, on the rows of the last message step
    x1, x2, sp = enc.rows1[-1], enc.rows2[-1], enc.sp
    ix1, ix2 = ops.pair_index(first, P, Q), ops.pair_index(second, P, Q)
    ix1.on(dev), ix2.on(dev)
    pplan = ops.panel_plan(enc.sizes_host, None)
    s1, s2 = enc.sum1[-1], enc.sum2[-1]
    g, ga = ops.pair_pool_gather(x1, x2, sp, sp, ix1, ix2, return_argmax=True)
    m, ma = ops.pair_pool_grid(x1, x2, sp, sp, plan, None, s1, s2, return_argmax=True)
    p, pa = ops.pair_pool_panel(x1, x2, sp, sp, pplan, s1, s2, return_argmax=True)
    same = {"grid_max_and_contacts_equal_gather": torch.equal(m[..., 0], g.view(Q, Q, 2)[..., 0]) and torch.equal(ma, ga.view(Q, Q, 2)),
            "grid_equals_panel_bit_for_bit": torch.equal(m, p) and torch.equal(ma, pa)}
    fusion = {"pair_pool_gather_all_pairs_us": fusion_us(lambda: ops.pair_pool_gather(x1, x2, sp, sp, ix1, ix2), ("k_pair_gather",)),
              "pair_pool_panel_on_drug_rows_us": fusion_us(lambda: ops.pair_pool_panel(x1, x2, sp, sp, pplan, s1, s2), ("k_pair_panel",)),
              "pair_pool_grid_us": fusion_us(lambda: ops.pair_pool_grid(x1, x2, sp, sp, plan, None, s1, s2), ("k_pair_grid",))}
    med = {k: statistics.median(v) for k, v in times.items()}
    b = "b: score_matrix"
    fair = f"a: score_pairs, chunks of {CHUNKS[-1]}"
    lo_a, hi_b = min(times[fair]), max(times[b])
    print(json.dumps({"workload": f"default ArchitectureDDI eval, {Q} drugs of {int(enc.sizes_host.min())}-{int(enc.sizes_host.max())} atoms "
                                  f"({enc.sp.N} rows), all {P} ordered pairs, {ROUNDS} rounds",
                      "ms_per_table": {k: round(v * 1e3, 2) for k, v in med.items()},
                      "rounds_ms": {k: [round(t * 1e3, 2) for t in v] for k, v in times.items()},
                      "spread_ms": {k: round((max(v) - min(v)) * 1e3, 2) for k, v in times.items()},
                      "pairs_per_s": {k: round(P / v) for k, v in med.items()},
                      "b_over_fair_a_speedup": round(med[fair] / med[b], 3),
                      "b_beats_fair_a_by_more_than_the_spread": bool(hi_b < lo_a),
                      "peak_MiB_above_the_encoding": peaks, "max_abs_diff_a_b": diff,
                      "fusion_width": int(x1.size(1)), "fusion_alone_us_median_min_max": fusion, **same,
                      "grid_chunks": plan.total_chunks, "grid_mean_lane_fill": round(plan.fill, 4),
                      "panel_chunks": pplan.total_chunks, "panel_mean_lane_fill": round(enc.sp.N / (64.0 * pplan.total_chunks), 4),
                      "head_row_drugs_per_block": net._matrix_block_rows(0, Q, Q)}), flush=True)
