"""What the attention export costs: ``glam_amd.explain.explain`` on B synthetic molecules, default width, ``_TripletMessage`` with each of the
three readouts.  Three legs take turns in one process, each in device-synchronised windows of at least --window seconds after a warm-up:
  (a) forward   the eager eval forward alone (``model._eager_forward`` under no_grad: what explain() runs first)
  (b) explain   ``explain(model, batch)``: that forward + the export launches
  (c) op-by-op  the alpha of the three message steps the only way the package offered before: ``MessagePassing.propagate`` -> ``message`` ->
                ``layer.softmax`` on tensors pre-multiplied by the weights, the softmax's result kept (inputs captured once, outside the timing)
Then, through ``kernel_timer``, one explain() call's export kernels with the bytes they must move (from shapes) over the 8 TB/s HBM peak.
usage: bench_explain.py [--graphs 1024] [--window 0.5] [--windows 5]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from glam_amd import _lib, explain, layer, model
from glam_amd.data import synth_batch

ap = argparse.ArgumentParser()
ap.add_argument("--graphs", type=int, default=1024)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_explain.py measures on the GPU; there is no CPU path"
dev = torch.device("cuda")
HBM_PEAK = 8e12

b = synth_batch(args.graphs, seed=0).to(dev)
N, E, B = b.x.size(0), b.edge_index.size(1), args.graphs


def window(fn):
    """ms per call over a window of at least args.window seconds that ends in a device synchronise."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        for _ in range(10):
            fn()
        n += 10
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= args.window:
            return dt / n * 1e3


def op_by_op_leg(m, conv_inputs):
    """The three steps' alpha through propagate -> message -> layer.softmax, on pre-multiplied tensors."""
    conv = m.mol_conv.conv.conv
    kept = []
    real = layer.softmax

    def keeping(*a, **k):
        kept.append(real(*a, **k))
        return kept[-1]

    def leg():
        kept.clear()
        layer.softmax = keeping
        try:
            with torch.no_grad():
                for x, ei, ea in conv_inputs:
                    conv.propagate(ei, x=torch.matmul(x, conv.weight_node), edge_attr=torch.matmul(ea, conv.weight_edge))
        finally:
            layer.softmax = real
        return kept

    return leg


def export_bytes(name, De, ld):
    """Bytes the kernel must move, from shapes: De = padded edge-feature width, ld = padded row width of the readout's input."""
    if name.startswith("k_edge_attention_sent"):
        return (N + 1) * 4 + E * 4 + E * 16 + N * 16                       # colptr, eid_t, alpha rows; sent rows
    if name.startswith("k_edge_attention"):
        return (N + 1) * 4 + E * 8 + N * 16 + E * 16 + E * De * 4 + E * 16  # rowptr, src + eid, a_i, a_j, edge_attr; alpha rows
    if name.startswith("k_segment_softmax<1>"):
        return (B + 1) * 4 + N * 4 + N * 4
    return (B + 1) * 4 + N * ld * 4 + B * ld * 4 + N * 4                    # query form: the rows, the queries; the weights


print(f"B = {B} synthetic molecules: N = {N} atoms, E = {E} directed bonds; default width (hid_dim 60), _TripletMessage, 3 message steps")
print(f"ms per call: median of {args.windows} windows of >= {args.window} s per leg, the legs taking turns (spread = max - min)")
print(f"{'readout':14s} {'(a) forward':>12s} {'(b) explain':>12s} {'(b)-(a)':>9s} {'(c) op-by-op':>13s} {'spread a/b/c':>20s}")
for readout in ("GlobalPool5", "GlobalLAPool", "Set2Set"):
    torch.manual_seed(0)
    m = model.Architecture(mol_block="_TripletMessage", mol_readout=readout).to(dev).eval()
    conv_inputs = []
    h = m.mol_conv.conv.conv.register_forward_pre_hook(lambda mod, a: conv_inputs.append(a))
    with torch.no_grad():
        m._eager_forward(b)
    h.remove()

    def forward():
        with torch.no_grad():
            return m._eager_forward(b)

    legs = [forward, lambda: explain.explain(m, b), op_by_op_leg(m, conv_inputs)]
    # the two routes give the same weights (otherwise (c) is no baseline)
    ex, kept = legs[1](), legs[2]()
    for a_new, a_old in zip(ex.edge_attention, kept):
        assert (a_new - a_old.view(E, -1)).abs().max().item() < 1e-5
    for leg in legs:                 # warm-up of every shape
        for _ in range(20):
            leg()
    times = [[] for _ in legs]
    for _ in range(args.windows):
        for k, leg in enumerate(legs):
            times[k].append(window(leg))
    med = [statistics.median(t) for t in times]
    spread = "/".join(f"{max(t) - min(t):.3f}" for t in times)
    print(f"{readout:14s} {med[0]:12.3f} {med[1]:12.3f} {med[1] - med[0]:9.3f} {med[2]:13.3f} {spread:>20s}", flush=True)

    tm = m.mol_conv.conv.conv
    De_p, ld = layer._pad_de(tm.edge_channels), layer._ceil4(tm.node_channels)
    with _lib.kernel_timer() as kt:
        explain.explain(m, b)
    torch.cuda.synchronize()
    mine = [(n, g, us) for n, g, us in kt.records() if n.startswith(("k_edge_attention", "k_segment_softmax"))]
    for n, g, us in mine:
        by = export_bytes(n, De_p, ld)
        print(f"    {n:26s} grid {g:5d} {us:8.2f} us   {by / 1e6:7.2f} MB to move = {by / (us * 1e-6) / HBM_PEAK * 100:5.1f} % of the 8 TB/s HBM peak")
    print(f"    export kernels of one explain() call: {len(mine)} launches, {sum(us for _, _, us in mine):.1f} us in total", flush=True)
