"""A SHUFFLING training loop end to end (new batch composition every step: collation, host-to-device copy, CSR staging and
its validation sync, eager step): molecules/s at B = 1024 and B = 32.  ``--resident``: the same loop over a device-resident dataset
(``DataLoader(resident=True)``: one small copy and one launch per batch, index included).  ``--resident --graphed``: the same loop through one
fixed-capacity batch and ``GraphedTrainStep`` (``DataLoader(padded=True)``: one table copy and one graph launch per step),
with the padding overhead of an epoch (mean N_cap / N, E_cap / E).  ``--phantom-rows M`` (with ``--graphed``; ``M`` an integer or ``max`` = the
dataset's largest graph): the surplus rows in K phantom graphs of at most ``M`` nodes (``DataLoader(phantom_rows=M)``), with K
and the mean phantom graph size of the epoch."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from glam_amd import graphs, model, optim
from glam_amd.data import DataLoader, synth_molecule
resident = "--resident" in sys.argv[1:]
graphed = "--graphed" in sys.argv[1:]
if graphed and not resident:
    sys.exit("--graphed runs over the device-resident dataset: pass --resident too")
phantom_rows = sys.argv[sys.argv.index("--phantom-rows") + 1] if "--phantom-rows" in sys.argv[1:] else None
if phantom_rows is not None and not graphed:
    sys.exit("--phantom-rows shapes the padded batch of --graphed: pass --resident --graphed too")
dev = torch.device("cuda")
rng = np.random.default_rng(0)
mols = [synth_molecule(rng) for _ in range(8192)]
torch.manual_seed(0)
net = model.Architecture(mol_block="_NNConv", graph_norm="_PairNorm", graph_do="_None()", end_do="_None()", pre_act="ReLU", graph_act="ReLU",
                         flat_act="ReLU").to(dev)
opt = (optim.Adam(net.parameters(), lr=1e-3) if os.environ.get("GLAM_ADAM", "glam") == "glam"
           else torch.optim.Adam(net.parameters(), lr=1e-3, capturable=True, fused=True))
mse = lambda out, b: torch.nn.functional.mse_loss(out.view(-1), b.y.view(-1))      # noqa: E731
stepper = graphs.GraphedTrainStep(net, opt, graphs.padded_loss(mse)) if graphed else None
for B in (1024, 32):
    data = mols if B == 1024 else mols[:2048]
    m = None if phantom_rows is None else max(int(d.x.size(0)) for d in data) if phantom_rows == "max" else int(phantom_rows)
    loader = DataLoader(data, batch_size=B, shuffle=True, device=dev, resident=resident, padded=graphed, collate_in_step=graphed, phantom_rows=m)
    times = []
    for epoch in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        t_col = 0.0
        it = iter(loader)
        while True:
            c0 = time.perf_counter()
            b = next(it, None)
            t_col += time.perf_counter() - c0
            if b is None:
                break
            if graphed:
                stepper(b)
                pb = b
                continue
            opt.zero_grad(set_to_none=True)
            mse(net(b), b).backward()
            opt.step()
        torch.cuda.synchronize(); times.append((time.perf_counter() - t0, t_col))
    n = len(loader.dataset)
    if graphed:
        n_cap, e_cap = pb.capacity
        print(f"graphed B={B}: capacity N_cap={n_cap} E_cap={e_cap}; over the last epoch mean N_cap/N = {np.mean(n_cap / pb.totals[:, 0]):.3f}, "
              f"mean E_cap/E = {np.mean(e_cap / pb.totals[:, 1]):.3f}; graphs captured so far: {stepper.graphs()}", flush=True)
        K = pb.num_phantom_graphs
        print(f"graphed B={B}: phantom_rows={pb.phantom_rows} K={K} phantom graphs; over the last epoch mean phantom graph size = "
              f"{np.mean((n_cap - pb.totals[:, 0]) / K):.1f} nodes (largest {int((n_cap - pb.totals[:, 0]).max() + K - 1) // K})", flush=True)
    print(f"{'graphed' if graphed else 'resident' if resident else 'host'} loader B={B}: epoch {times[-1][0] * 1e3:.1f} ms for {n} molecules = {n / times[-1][0]:.0f} molecules/s "
          f"(collate + copy: {times[-1][1] * 1e3:.1f} ms of it)", flush=True)
