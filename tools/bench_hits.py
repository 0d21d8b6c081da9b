"""Screening a ligand library against cached proteins down to the best K ligands per protein — three routes from the same
model.screen_panel(ligands, enc) per batch to the same K x Q hit lists:
  (a) every batch's scores copied to the host (one synchronising copy per batch), ONE numpy selection at the end — host memory grows
      with the library
  (b) a running selection on the device in ATen: torch.cat of the lists and the batch, torch.topk, gather of the ids — per batch
  (c) model.screen_top(batches, enc, k=K)              — the hit lists of csrc/hits.hip: two HIP launches per batch, no read-back
on default ArchitectureDTI() in eval() under no_grad, Q synthetic proteins of 500 residues encoded once, a library of steps x L synthetic
ligands in freshly shuffled resident batches (one window = one pass over the library: no ligand repeats inside it), L in {32, 1 024} x
Q in {1, 15}.  The three legs alternate inside one process; timed like tools/bench_panel.py (host clock around a window that starts with
empty lists and ends in a device synchronise — for (a) after the selection), median of the rounds and their spread (max - min).  Also:
whether the three routes select the same scores on one fixed pass, and the merge launches' own kernel time (k_hits_slab +
k_hits_finish) per batch from glam_prof_* (a separate, untimed pass).

usage: bench_hits.py [--L 32,1024] [--Q 1,15] [--k 100] [--steps N] [--rounds R] [--residues N] [--out FILE]"""
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

_opts = {"--L": "32,1024", "--Q": "1,15", "--k": "100", "--steps": "16", "--rounds": "3", "--residues": "500", "--out": ""}
_args = sys.argv[1:]
while _args:
    a = _args.pop(0)
    if a not in _opts:
        sys.exit(__doc__)
    _opts[a] = _args.pop(0)
LS, QS = [int(v) for v in _opts["--L"].split(",")], [int(v) for v in _opts["--Q"].split(",")]
K, STEPS, ROUNDS, RES = int(_opts["--k"]), int(_opts["--steps"]), int(_opts["--rounds"]), int(_opts["--residues"])
dev = torch.device("cuda")
torch.manual_seed(0)
net = model.ArchitectureDTI().to(dev).eval()
net.graphed_call = False
rng = np.random.default_rng(0)
proteins = [synth_protein(rng, RES, RES) for _ in range(max(QS))]
lines = []


def batches(loader):
    while True:                      # (every epoch is a fresh shuffle of the same library)
        yield from loader


def by_host(stream, enc):
    got = [net.screen_panel(mol, enc)[:, :, 0].cpu().numpy() for mol in stream]          # (one synchronising copy per batch)
    s = np.concatenate(got).T                                                            # [Q, N]
    k = min(K, s.shape[1])                                                               # (a window shorter than the lists)
    pick = np.argpartition(-s, k - 1, axis=1)[:, :k]
    best = np.take_along_axis(s, pick, 1)
    order = np.argsort(-best, axis=1, kind="stable")
    return np.take_along_axis(best, order, 1), np.take_along_axis(pick, order, 1)


def by_aten(stream, enc):
    ts = ti = None
    seen = 0
    for mol in stream:
        out = net.screen_panel(mol, enc)[:, :, 0].t()                                    # [Q, L]
        Q, L = out.shape
        if ts is None:
            ts = torch.full((Q, K), float("-inf"), device=dev)
            ti = torch.full((Q, K), -1, dtype=torch.int64, device=dev)
        ids = torch.arange(seen, seen + L, device=dev).expand(Q, L)
        cs, ci = torch.cat([ts, out], 1), torch.cat([ti, ids], 1)
        ts, pos = torch.topk(cs, K, dim=1)
        ti = ci.gather(1, pos)
        seen += L
    return ts, ti


def by_hit_list(stream, enc):
    return net.screen_top(stream, enc, k=K).result()


def window(leg, feed, enc, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    leg((next(feed) for _ in range(n)), enc)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


with torch.no_grad():
    for L in LS:
        library = [synth_molecule(rng) for _ in range(STEPS * L)]
        feed = batches(DataLoader(library, batch_size=L, shuffle=True, device=dev, resident=True))
        for Q in QS:
            enc = net.encode_proteins(Batch.from_data_list(proteins[:Q]).to(dev))
            legs = {"a: host copy + numpy": by_host, "b: ATen cat/topk/gather": by_aten, "c: screen_top": by_hit_list}
            fixed = [next(feed) for _ in range(STEPS)]                # one pass, the same batches for every route
            sa = by_host(fixed, enc)[0]
            sb = by_aten(fixed, enc)[0].cpu().numpy()
            sc = by_hit_list(fixed, enc)[0].cpu().numpy()
            times = {k: [] for k in legs}
            for leg in legs.values():
                window(leg, feed, enc, 3)                             # warm-up of every shape of the window
            for _ in range(ROUNDS):
                for k, leg in legs.items():                           # alternating: the legs see the same state of the box
                    times[k].append(window(leg, feed, enc, STEPS))
            with _lib.kernel_timer() as kt:
                by_hit_list(fixed, enc)
                torch.cuda.synchronize()
            rec = kt.records()
            merge = [r for r in rec if r[0] in ("k_hits_slab", "k_hits_finish")]
            assert len(merge) == 2 * STEPS, [r[0] for r in rec if "hits" in r[0]]
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            a, b, c = (med[k] for k in legs)
            lines.append(json.dumps({
                "workload": f"default ArchitectureDTI eval, K={K} of {STEPS} batches x L={L} ligands per window, Q={Q} proteins of {RES} "
                            f"residues, {ROUNDS} rounds",
                "a_ms_per_batch": a * 1e3, "b_ms_per_batch": b * 1e3, "c_ms_per_batch": c * 1e3,
                "a_scores_per_s": L * Q / a, "b_scores_per_s": L * Q / b, "c_scores_per_s": L * Q / c,
                "spread_ms": {k: v * 1e3 for k, v in spread.items()},
                "c_over_b_speedup": b / c, "c_beats_b_by_more_than_the_spread": bool(b - c > max(spread["b: ATen cat/topk/gather"], spread["c: screen_top"])),
                "c_over_a_speedup": a / c,
                "rounds_ms": {k: [round(t * 1e3, 4) for t in v] for k, v in times.items()},
                "same_scores_selected_a_c": bool(np.array_equal(sa, sc)), "same_scores_selected_b_c": bool(np.array_equal(sb, sc)),
                "merge_kernels_us_per_batch": sum(r[2] for r in merge) / STEPS,
                "merge_kernels_us_per_batch_last_half": sum(r[2] for r in merge[STEPS:]) / (STEPS / 2),
                "slab_us_first_batch": merge[0][2], "finish_us_first_batch": merge[1][2],
                "slab_us_last_batch": merge[-2][2], "finish_us_last_batch": merge[-1][2], "slab_grid": merge[-2][1],
                "all_glam_kernels_us_per_batch_leg_c": sum(r[2] for r in rec) / STEPS, "glam_launches_per_batch_leg_c": len(rec) / STEPS}))
            print(lines[-1], flush=True)
            del enc, fixed
        del feed, library
        torch.cuda.empty_cache()
if _opts["--out"]:
    os.makedirs(os.path.dirname(os.path.abspath(_opts["--out"])), exist_ok=True)
    with open(_opts["--out"], "w") as f:
        f.write("\n".join(lines) + "\n")
