"""Developer aid: the library's kernel launches of ONE full-model training step, in launch order (glam_prof_* labels and durations; ATen
launches are not listed: tools/bench_model.py --profile names those; the ATen normalisation ops of the step are counted at the end).
usage: kernel_sequence.py [batch] [preset]      (preset: relu, model_default, colnorm = a norm in every slot, DESIGN.md 4.12;
padded = relu on a fixed-capacity batch with the loss over output[:B], DESIGN.md 4.16: the collate launch leads the sequence and the ATen
ops of the output slice are counted at the end; padded_split = the same with phantom_rows = the dataset's largest graph)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from glam_amd import _lib, model, ops, optim, loss as glam_loss
ops.USE_TORCH_EXT = False      # the route a captured step takes
from glam_amd.data import DeviceDataset, synth_batch, synth_molecule

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
dev = torch.device("cuda")
torch.manual_seed(0)
PRESET = sys.argv[2] if len(sys.argv) > 2 else "relu"
if PRESET == "model_default":      # Architecture()'s keyword defaults in training mode: RReLU x 3, Dropout(0.2) twice
    net = model.Architecture(mol_block="_TripletMessage", message_steps=3).to(dev).train()
elif PRESET == "colnorm":          # _BatchNorm / batch-less _LayerNorm in the four norm slots (tests/test_gpu_colnorm.py's captured step)
    net = model.Architecture(pre_norm="_BatchNorm", graph_norm="_BatchNorm", flat_norm="_LayerNorm", end_norm="_BatchNorm", pre_act="ReLU",
                             graph_act="ReLU", flat_act="ReLU", graph_do="_None()", end_do="_None()", mol_block="_TripletMessage").to(dev)
else:
    net = model.Architecture(mol_block="_TripletMessage", message_steps=3, graph_do="_None()", end_do="_None()", pre_act="ReLU", graph_act="ReLU",
                             flat_act="ReLU").to(dev)
net.graphed_call = False      # (eager launches: every one carries its own events)
PADDED = PRESET in ("padded", "padded_split")
if PADDED:
    import numpy as np
    rng = np.random.default_rng(0)
    dd = DeviceDataset([synth_molecule(rng) for _ in range(2 * B)], dev)
    b = dd.padded(B, phantom_rows=int(dd.ns.max()) if PRESET == "padded_split" else None)
    b.load(rng.permutation(2 * B)[:B], launch=False)
else:
    b = synth_batch(B, seed=0).to(dev)
y = b.y.view(-1)
opt = optim.Adam(net.parameters(), lr=1e-3)
ONE = torch.ones((), device=dev)

def body():
    if PADDED:
        b.glam_reload()              # (the step's first launch: GraphedTrainStep calls the batch's reload hook)
    opt.zero_grad(set_to_none=True)
    loss = glam_loss.mse_loss(net(b)[:B].view(-1), y)      # (every preset's output has B rows but the padded ones': B + K)
    loss.backward(gradient=ONE)
    opt.step()

for _ in range(5):
    body()
torch.cuda.synchronize()
with _lib.kernel_timer(capacity=256) as kt:
    body()
torch.cuda.synchronize()
tot = 0.0
for i, (name, grid, us) in enumerate(kt.records()):
    tot += us
    print(f"{i:3d} {us:7.2f} us  grid {grid:6d}  {name}")
print(f"{i + 1} launches, {tot:.1f} us of kernels")

# the ATen normalisation / whole-tensor statistics ops the step still dispatches (none when every norm of the model is a library kernel)
import collections
from torch.utils._python_dispatch import TorchDispatchMode
NORM_OPS = ("batch_norm", "layer_norm", "aten.mean", "aten.std", "aten.var", "miopen")
if PADDED:                         # ... and what the slice output[:B] adds: forward a view, backward a zero fill and a copy into it
    NORM_OPS += ("slice", "aten.zeros", "aten.new_zeros", "aten.zero_", "aten.fill_", "aten.copy_")
seen = collections.Counter()
class Log(TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if any(k in str(func) for k in NORM_OPS):
            seen[str(func)] += 1
        return func(*args, **(kwargs or {}))
with Log():
    body()
torch.cuda.synchronize()
print("ATen normalisation ops in the step:" if not PADDED else "ATen normalisation, slice, fill and copy ops in the step:", dict(seen) if seen else "none")
