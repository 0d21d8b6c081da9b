"""The class table against the routes it replaces — called class, its log-probability and one selected log-probability for every entry of
a table, default models in eval() under no_grad, synthetic graphs, encoded once per leg:
  ddi86   ArchitectureDDI(out_dim=86) over the whole Q x Q table:  classify_matrix(classes=[1])  against  score_matrix(head="rows") +
          torch.log_softmax + max (three ATen launches over the [Q, Q, 86] logits);
  ddi8    the same at out_dim = 8, where score_matrix(head="factored") + the three ATen launches is a third route;
  dti2    ArchitectureDTI(out_dim=2), 1 024 ligands x 15 proteins of 500 residues:  classify_panel(classes=[1])  against  screen_panel
          (head="rows", and head="factored") + torch.log_softmax;
  each leg also times the head ALONE on the leg's operands (the flat matrices and the steps' fusions, computed once).
Every leg is a child process of its own under its own time limit (the parent never opens the device; a leg that fails or runs out of time
ends the run); in a leg the routes alternate, timed with the host clock around a window that ends in a device synchronise, median
(min - max) of the rounds; peak device memory per route from torch's allocator, above what was allocated before the call (the encoding).

usage: bench_pair_classes.py [--drugs Q] [--rounds R] [--limit SECONDS] [--out FILE]      (FILE: default profiles/pair_classes_bench.txt)"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_opts = {"--drugs": "1024", "--rounds": "5", "--limit": "240", "--out": os.path.join(ROOT, "profiles", "pair_classes_bench.txt"), "--leg": ""}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    if a not in _opts or not _args:
        sys.exit(__doc__)
    _opts[a] = _args.pop(0)
Q, ROUNDS, LIMIT = int(_opts["--drugs"]), int(_opts["--rounds"]), int(_opts["--limit"])
LEGS = ("ddi86", "ddi8", "dti2")


def run_leg(name):
    import numpy as np
    import torch

    from glam_amd import model, ops
    from glam_amd.data import Batch, synth_molecule, synth_protein

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
        """``steps``: route -> callable.  Warm-up of each, ROUNDS alternating rounds, then the peak of each."""
        for step in steps.values():
            step()
        times = {h: [] for h in steps}
        for _ in range(ROUNDS):
            for h, step in steps.items():                        # alternating: the routes see the same state of the machine
                times[h].append(window(step))
        med = {h: statistics.median(v) for h, v in times.items()}
        out = {"ms_median_min_max": {h: [round(med[h] * 1e3, 3), round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for h, v in times.items()},
               "peak_MiB_above_the_encoding": {h: round(peak_mib(step), 1) for h, step in steps.items()}}
        for h in steps:
            if h != "classes":
                out[f"{h}_over_classes"] = round(med[h] / med["classes"], 3)
                out[f"classes_ahead_of_{h}_beyond_the_spread"] = bool(max(times["classes"]) < min(times[h]))
                out[f"{h}_ahead_of_classes_beyond_the_spread"] = bool(max(times[h]) < min(times["classes"]))
        return out

    def from_logits(logits):
        """What the listed routes add to their logits: the three ATen launches."""
        lsm = torch.log_softmax(logits, -1)
        logp, cls = lsm.max(-1)
        return cls, logp, lsm[..., 1]

    def agreement(table, ref):
        cls, logp, sel1 = ref
        return {"cls_equal_share": round((table.cls.long() == cls).float().mean().item(), 6),
                "max_abs_diff_logp": (table.logp - logp).abs().max().item(), "max_abs_diff_sel": (table.sel[..., 0] - sel1).abs().max().item()}

    result = {}
    with torch.no_grad():
        torch.manual_seed(0)
        if name.startswith("ddi"):
            out_dim = int(name[3:])
            net = model.ArchitectureDDI(out_dim=out_dim).to(dev).eval()
            net.graphed_call = False
            enc = net.encode_drugs(Batch.from_data_list([synth_molecule(rng) for _ in range(Q)]).to(dev))
            steps = {"classes": lambda: net.classify_matrix(enc, classes=[1]),
                     "rows": lambda: from_logits(net.score_matrix(enc, head="rows"))}
            if out_dim <= ops.HEAD_MAX_OUT:
                steps["factored"] = lambda: from_logits(net.score_matrix(enc, head="factored"))
            result[f"{name}: the whole call, {Q} x {Q} drugs, out_dim {out_dim}"] = dict(leg(steps), **agreement(steps["classes"](), steps["rows"]()))
            # the head alone, on the table's operands
            plan = enc.grid(None)
            fusion = [ops.pair_pool_grid(enc.rows1[s], enc.rows2[s], enc.sp, enc.sp, plan, None, enc.sum1[s], enc.sum2[s])
                      for s in range(net.message_steps)]
            o1, o2, R, Cs = enc.flat1, enc.flat2, Q, Q
            per_block = net._matrix_block_rows(0, Q, Q)
        else:
            out_dim = 2
            net = model.ArchitectureDTI(out_dim=out_dim).to(dev).eval()
            net.graphed_call = False
            enc = net.encode_proteins(Batch.from_data_list([synth_protein(rng, 500, 500) for _ in range(15)]).to(dev))
            ligands = Batch.from_data_list([synth_molecule(rng) for _ in range(1024)]).to(dev)
            steps = {"classes": lambda: net.classify_panel(ligands, enc, classes=[1]),
                     "rows": lambda: from_logits(net.screen_panel(ligands, enc, head="rows")),
                     "factored": lambda: from_logits(net.screen_panel(ligands, enc, head="factored"))}
            result[f"{name}: the whole call, 1024 ligands x 15 proteins of 500 residues, out_dim 2"] = dict(
                leg(steps), **agreement(steps["classes"](), steps["rows"]()))
            plan = enc.panel(None)
            m = model._Tower(net, "mol", ligands)
            with ops.weight_scope():
                fusion, _, o1, o2 = net._panel_walk(m, ligands, enc, plan, False)
            R, Cs = 1024, 15
            per_block = R
        act = model._class_head(net, "bench")

        def head_rows():
            with ops.weight_scope():             # the head of score_matrix(head="rows"); the panel: one piece
                return from_logits(model._table_head_rows(net, o1, o2, fusion, R, Cs, per_block))
        heads = {"classes": lambda: model._table_head_classes(net, act, o1, o2, fusion, R, Cs, [1], False), "rows": head_rows}
        if out_dim <= ops.HEAD_MAX_OUT:
            heads["factored"] = lambda: from_logits(model._table_head_factored(net, act, o1, o2, fusion, R, Cs))
        result[f"{name}: the head alone, {R} x {Cs} pairs, e_dim 1024, F {2 * net.message_steps}, out_dim {out_dim}"] = leg(heads)
    print("LEG " + json.dumps(result), flush=True)


if _opts["--leg"]:
    run_leg(_opts["--leg"])
    sys.exit(0)

result = {}
for name in LEGS:
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--drugs", str(Q), "--rounds", str(ROUNDS)]
    try:
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        sys.exit(f"leg {name} ran past its limit of {LIMIT} s: nothing more is started")
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("LEG ")]
    if done.returncode != 0 or not lines:
        sys.exit(f"leg {name} ended with status {done.returncode}: nothing more is started\n{done.stderr[-2000:]}")
    result.update(json.loads(lines[-1][4:]))

header = f"""tools/bench_pair_classes.py --drugs {Q} --rounds {ROUNDS}, one MI355X, one process per leg, the routes of a leg alternating, {ROUNDS} rounds per
leg and route, [median, min, max] milliseconds of the host clock around a window that ends in a device synchronise.  Default models (e_dim
1 024, three message steps: F = 6 fusion columns, hid 60) with the leg's out_dim, in eval() under no_grad, synthetic graphs, encoded once.
classes: classify_matrix / classify_panel with classes=[1] (k_pair_head_classes_side + k_pair_head_classes): cls, logp and one selected
log-probability, no logits table.  rows / factored: score_matrix / screen_panel with that head, then torch.log_softmax, max and the column
of class 1 (out_dim 86 has no factored head).  "the whole call" includes the fusions (and the ligand tower of the panel); "the head alone"
runs on the same operands computed once.  Peak memory: torch's allocator, above what was allocated before the call (the encoding).
X_over_classes = median / median;  *_beyond_the_spread: the slower route's fastest round is slower than the other's slowest.
"""
text = header + "\n" + json.dumps(result) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(_opts["--out"])), exist_ok=True)
with open(_opts["--out"], "w") as fh:
    fh.write(text)
print(json.dumps(result), flush=True)
