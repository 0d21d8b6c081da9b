"""The head of a score table, listed against factored: head="rows" (the pair rows through lin_out0 / lin_out1: a [pairs, e_dim] hidden
matrix, in blocks for score_matrix) against head="factored" (ops.pair_head: the first layer as a row part + a column part + the fusion
columns' part, no pair rows and no hidden matrix) — the same run, the same encodings, default models in eval() under no_grad:
  leg 1  ArchitectureDDI.score_matrix over Q synthetic drugs of 12-28 atoms, the whole Q x Q table;
  leg 2  ArchitectureDTI.screen_panel of 1 024 and of 32 synthetic ligands against 15 proteins of 500 residues;
  leg 3  the head ALONE on the leg-1 table's operands (flat1, flat2 and the steps' fusions, computed once): the listed rows +
         lin_out0 + lin_out1 of model.py in blocks of _matrix_block_rows, against ops.pair_head.
One process, the two heads of a leg alternate; timed with the host clock around a window that ends in a device synchronise, median of the
rounds (min - max); peak device memory per leg and head from torch's allocator, above what was allocated before the call (the encoding).
Also max |rows - factored| of each leg's outputs, and the kernels of one factored head from glam_prof_*.

usage: bench_pair_head.py [--drugs Q] [--rounds R] [--out FILE]      (FILE: default profiles/pair_head_bench.txt)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from glam_amd import _lib, model, ops
from glam_amd.data import Batch, synth_molecule, synth_protein

_opts = {"--drugs": "1024", "--rounds": "3", "--out": os.path.join(ROOT, "profiles", "pair_head_bench.txt")}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    if a not in _opts:
        sys.exit(__doc__)
    _opts[a] = _args.pop(0)
Q, ROUNDS = int(_opts["--drugs"]), int(_opts["--rounds"])
HEADS = ("rows", "factored")
dev = torch.device("cuda")
rng = np.random.default_rng(0)


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


def leg(steps):
    """``steps``: head -> callable.  Warm-up of both, ROUNDS alternating rounds, then the peak of each."""
    for step in steps.values():
        step()
    times = {h: [] for h in steps}
    for _ in range(ROUNDS):
        for h, step in steps.items():                            # alternating: both heads see the same state of the machine
            times[h].append(window(step))
    ms = {h: [round(statistics.median(v) * 1e3, 3), round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for h, v in times.items()}
    r, f = times["rows"], times["factored"]
    return {"ms_median_min_max": ms, "peak_MiB_above_the_encoding": {h: round(peak_mib(step), 1) for h, step in steps.items()},
            "rows_over_factored": round(statistics.median(r) / statistics.median(f), 3),
            "factored_ahead_beyond_the_spread": bool(max(f) < min(r)), "rows_ahead_beyond_the_spread": bool(max(r) < min(f))}


result = {}
with torch.no_grad():
    # ---- leg 1: the DDI table
    torch.manual_seed(0)
    ddi = model.ArchitectureDDI().to(dev).eval()
    ddi.graphed_call = False
    enc = ddi.encode_drugs(Batch.from_data_list([synth_molecule(rng) for _ in range(Q)]).to(dev))
    tables = {h: ddi.score_matrix(enc, head=h) for h in HEADS}
    result[f"1: score_matrix, {Q} x {Q} drugs"] = dict(leg({h: (lambda h=h: ddi.score_matrix(enc, head=h)) for h in HEADS}),
                                                     max_abs_diff=(tables["rows"] - tables["factored"]).abs().max().item())
    # ---- leg 3 (on leg 1's operands): the head alone
    plan = enc.grid(None)
    fusion = [ops.pair_pool_grid(enc.rows1[s], enc.rows2[s], enc.sp, enc.sp, plan, None, enc.sum1[s], enc.sum2[s]) for s in range(ddi.message_steps)]
    o1, o2 = enc.flat1, enc.flat2
    per_block = ddi._matrix_block_rows(0, Q, Q)
    act = model._factored_head(ddi, "bench")

    def head_rows():
        with ops.weight_scope():
            return model._table_head_rows(ddi, o1, o2, fusion, Q, Q, per_block)          # the head of score_matrix(head="rows")

    def head_factored():
        return model._table_head_factored(ddi, act, o1, o2, fusion, Q, Q)
    result[f"3: the head alone, {Q} x {Q} pairs, e_dim 1024, F {2 * ddi.message_steps}"] = dict(
        leg({"rows": head_rows, "factored": head_factored}), max_abs_diff=(head_rows() - head_factored()).abs().max().item(),
        head_row_drugs_per_block=per_block)
    with _lib.kernel_timer() as kt:
        head_factored()
        torch.cuda.synchronize()
    result["kernels_of_one_factored_head_us"] = {n: round(us, 1) for n, _g, us in kt.records() if n.startswith("k_pair_head")}
    del tables, fusion, enc
    # ---- leg 2: the DTI panels
    torch.manual_seed(0)
    dti = model.ArchitectureDTI().to(dev).eval()
    dti.graphed_call = False
    penc = dti.encode_proteins(Batch.from_data_list([synth_protein(rng, 500, 500) for _ in range(15)]).to(dev))
    for L in (1024, 32):
        ligands = Batch.from_data_list([synth_molecule(rng) for _ in range(L)]).to(dev)
        panels = {h: dti.screen_panel(ligands, penc, head=h) for h in HEADS}
        result[f"2: screen_panel, {L} ligands x 15 proteins of 500 residues"] = dict(
            leg({h: (lambda h=h: dti.screen_panel(ligands, penc, head=h)) for h in HEADS}),
            max_abs_diff=(panels["rows"] - panels["factored"]).abs().max().item())

header = f"""tools/bench_pair_head.py --drugs {Q} --rounds {ROUNDS}, one MI355X, one process, the two heads of a leg alternating, {ROUNDS} rounds per leg
and head, [median, min, max] milliseconds of the host clock around a window that ends in a device synchronise.  Default ArchitectureDDI() /
ArchitectureDTI() (e_dim 1 024, three message steps: F = 6 fusion columns, hid 60) in eval() under no_grad, synthetic graphs, encoded once.
head="rows": the pair rows through lin_out0 / lin_out1 (score_matrix: in blocks of row drugs whose hidden matrix stays within 512 MiB;
screen_panel: in one piece).  head="factored": ops.pair_head (k_pair_head_side + k_pair_head).
Legs 1 and 2 time the WHOLE call (the ligand tower of screen_panel and the steps' fusions included); leg 3 the head alone on leg 1's operands.
Peak memory: torch's allocator, above what was allocated before the call (the encoding).
rows_over_factored = median / median;  *_ahead_beyond_the_spread: the slower head's fastest round is slower than the other's slowest.
"""
text = header + "\n" + json.dumps(result) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(_opts["--out"])), exist_ok=True)
with open(_opts["--out"], "w") as fh:
    fh.write(text)
print(json.dumps(result), flush=True)
