"""Ranger on the device (csrc/optim.hip `k_ranger` through glam_amd.optim.Ranger): the reference's trajectories
(tests/golden/ranger_*.npz), a default-shaped model with long rows and more tensors than one launch takes, capture, device learning
rates and ReduceLROnPlateau, parameters without a gradient, checkpoints exchanged with the reference's optimizer (restated below), and
training under GraphedTrainStep."""
import copy
import math

import numpy as np
import pytest
import torch

from glam_amd import model, ops, optim
from glam_amd.graphs import _gc_paused
from tests.conftest import assert_close
from tests.test_ranger_host import NAMES, load_case

pytestmark = pytest.mark.gpu

# fp32 against fp32: the reference (CPU) and the kernel round differently (row-mean order, fused loads); the difference grows by a few
# units of 2^-23 per step relative to the tensor's scale — the bound the float64 restatement meets in tests/test_ranger_host.py, doubled
TOL_PER_STEP = 4e-6
# Ranger's first steps (N_sma below the threshold) are momentum SGD at lr, not normalised: a default-initialised model on these
# synthetic batches has gradients up to 1e3 and diverges there under the reference's arithmetic as well (the restatement below gives
# the same losses).  The training tests scale the loss down — a power of two, so eager and captured stay bit-comparable; the
# rectified steps are scale-invariant
LOSS_SCALE = 2.0 ** -12


class RefRanger(torch.optim.Optimizer):
    """The reference's Ranger (src_1gp/ranger.py) restated: per tensor, a Python-int step count, ATen operations in the same order."""

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0, use_gc=True,
                 gc_conv_only=False, gc_loc=True):
        super().__init__(params, dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                                      weight_decay=weight_decay))
        self.alpha, self.k, self.N_sma_threshhold = alpha, k, N_sma_threshhold
        self.use_gc, self.gc_conv_only, self.gc_loc = use_gc, gc_conv_only, gc_loc

    def _centralise(self, x):
        if self.use_gc and x.dim() > (3 if self.gc_conv_only else 1):
            x.add_(-x.mean(dim=tuple(range(1, x.dim())), keepdim=True))
        return x

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st, g = self.state[p], p.grad
                if not st:
                    st.update(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p), slow_buffer=p.detach().clone())
                if self.gc_loc:
                    self._centralise(g)
                st["step"] += 1
                s, m, v = st["step"], st["exp_avg"], st["exp_avg_sq"]
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                m.mul_(b1).add_(g, alpha=1 - b1)
                b2t = b2 ** s
                n_max = 2 / (1 - b2) - 1
                n_sma = n_max - 2 * s * b2t / (1 - b2t)
                if n_sma > self.N_sma_threshhold:
                    step_size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** s)
                    G = m / v.sqrt().add_(group["eps"])
                else:
                    step_size = 1.0 / (1 - b1 ** s)
                    G = m
                if group["weight_decay"] != 0:
                    G.add_(p, alpha=group["weight_decay"])
                if not self.gc_loc:
                    G = self._centralise(G)
                p.add_(G, alpha=-step_size * group["lr"])
                if s % group["k"] == 0:
                    slow = st["slow_buffer"]
                    slow.add_(p - slow, alpha=self.alpha)
                    p.copy_(slow)


def _close(got, ref, steps, what):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    assert err <= TOL_PER_STEP * steps * scale, f"{what}: max|d|={err:.3e} > {TOL_PER_STEP * steps:.1e} * {scale:.3g}"


@pytest.mark.parametrize("name", NAMES)
def test_reproduces_the_reference_trajectory(device, name):
    c = load_case(name)
    hp = c["hp"]
    params = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(device)) for x in c["p0"]]
    opt = optim.Ranger(params, lr=c["lr"], alpha=hp["alpha"], k=int(hp["k"]), N_sma_threshhold=hp["N_sma_threshhold"], betas=hp["betas"],
                       eps=hp["eps"], weight_decay=hp["weight_decay"], use_gc=bool(hp["use_gc"]), gc_conv_only=bool(hp["gc_conv_only"]),
                       gc_loc=bool(hp["gc_loc"]))
    for s in range(1, c["steps"] + 1):
        for p, g in zip(params, c["gin"]):
            p.grad = torch.from_numpy(g[s - 1].copy()).to(device)
        opt.step()
        for i, p in enumerate(params):
            st = opt.state[p]
            _close(p, c["p"][i][s - 1], s, f"{name} step {s} tensor {i} p")
            _close(p.grad, c["grad"][i][s - 1], s, f"{name} step {s} tensor {i} p.grad")          # centralised in place (gc_loc)
            _close(st["exp_avg"], c["exp_avg"][i][s - 1], s, f"{name} step {s} tensor {i} exp_avg")   # G's aliasing (wd, gc_loc=False)
            _close(st["exp_avg_sq"], c["exp_avg_sq"][i][s - 1], s, f"{name} step {s} tensor {i} exp_avg_sq")
            _close(st["slow_buffer"], c["slow_buffer"][i][s - 1], s, f"{name} step {s} tensor {i} slow_buffer")
    assert float(opt.state[params[0]]["step"]) == c["steps"]


def test_default_model_long_rows_and_two_launches_against_the_restatement(device):
    """A default-shaped model's parameters (rows up to 1 024, a [1024, 300] weight), one 307 200-element row, an odd row of 5 003 and
    enough small tensors that the group needs two launches, 20 steps at k = 6: both branches of the rectification, three syncs."""
    torch.manual_seed(0)
    net = model.Architecture()
    base = [p.detach() for p in net.parameters()] + [torch.randn(1, 307200), torch.randn(1, 5003)]
    base += [torch.randn(3, 7 + i) for i in range(30)]
    assert len(base) > optim._lib.load().glam_ranger_max_tensors()
    mine = [torch.nn.Parameter(x.clone().to(device)) for x in base]
    ref = [torch.nn.Parameter(x.clone().to(device)) for x in base]
    o_mine, o_ref = optim.Ranger(mine, lr=1e-2, k=6), RefRanger(ref, lr=1e-2, k=6)
    gen = torch.Generator(device=device).manual_seed(1)
    for s in range(1, 21):
        for a, b in zip(mine, ref):
            g = torch.randn(a.shape, device=device, generator=gen) * 0.1 + 0.02
            a.grad, b.grad = g.clone(), g.clone()
        o_mine.step()
        o_ref.step()
    for i, (a, b) in enumerate(zip(mine, ref)):
        _close(a, b, 20, f"tensor {i} {tuple(a.shape)} p")
        _close(a.grad, b.grad, 20, f"tensor {i} p.grad")
        for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            _close(o_mine.state[a][key], o_ref.state[b][key], 20, f"tensor {i} {key}")


def _grads(shapes, steps, device, seed=3):
    gen = torch.Generator(device=device).manual_seed(seed)
    return [[torch.randn(s, device=device, generator=gen) * 0.1 for s in shapes] for _ in range(steps)]


def test_captured_steps_equal_eager_steps_bit_for_bit(device):
    k = 4
    steps = 2 * k + 8
    torch.manual_seed(1)
    shapes = [(60, 15), (60,), (1024, 300), (1, 1024), (1,), (5, 13)]
    base = [torch.randn(s) for s in shapes]
    grads = _grads(shapes, 1, device)[0]
    eager = [torch.nn.Parameter(x.clone().to(device)) for x in base]
    capt = [torch.nn.Parameter(x.clone().to(device)) for x in base]
    o_e, o_c = optim.Ranger(eager, lr=2.0 ** -7, k=k, weight_decay=1e-2), optim.Ranger(capt, lr=2.0 ** -7, k=k, weight_decay=1e-2)
    for p, g in zip(eager, grads):
        p.grad = g.clone()
    for p, g in zip(capt, grads):
        p.grad = g.clone()                   # static gradient buffers: the captured launch reads these addresses on every replay
    for _ in range(steps):
        o_e.step()
    o_c.step()                               # the first step builds the device state eagerly
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _gc_paused(), torch.cuda.graph(graph):          # (no collection of other tests' graphs during the capture)
        o_c.step()
    for _ in range(steps - 1):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, capt):
        assert torch.equal(a, b) and torch.equal(a.grad, b.grad)
        for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            assert torch.equal(o_e.state[a][key], o_c.state[b][key]), key
    assert float(o_c.state[capt[0]]["step"]) == steps


def test_device_learning_rate_and_reduce_lr_on_plateau(device):
    shapes = [(8, 12), (12,), (1, 300)]
    torch.manual_seed(2)
    base = [torch.randn(s) for s in shapes]
    grads = _grads(shapes, 14, device)
    runs = []
    for mode in ("float", "tensor", "plateau"):
        ps = [torch.nn.Parameter(x.clone().to(device)) for x in base]
        lr = torch.tensor(2.0 ** -6, device=device) if mode == "tensor" else 2.0 ** -6
        opt = optim.Ranger(ps, lr=lr, k=3)
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=0) if mode == "plateau" else None
        for s, gs in enumerate(grads):
            for p, g in zip(ps, gs):
                p.grad = g.clone()
            opt.step()
            if s % 4 == 3:
                if sched is not None:
                    sched.step(1.0)              # no improvement after the first call: lr / 2
                elif s > 3:
                    g0 = opt.param_groups[0]
                    g0["lr"] = g0["lr"] * 0.5 if torch.is_tensor(g0["lr"]) else g0["lr"] * 0.5
        runs.append([p.detach().clone() for p in ps])
        if mode == "plateau":
            assert opt.param_groups[0]["lr"] == 2.0 ** -8
    for a, b, c in zip(*runs):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_parameters_without_a_gradient_sit_the_step_out(device):
    torch.manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(6, 10, device=device)) for _ in range(3)]
    opt = optim.Ranger(ps, lr=1e-2, k=2)
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()
    before = [(p.detach().clone(), {k: opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq", "slow_buffer")}) for p in ps]
    ps[1].grad = None
    ps[0].grad, ps[2].grad = torch.randn_like(ps[0]), torch.randn_like(ps[2])
    opt.step()                                   # step 2: a Lookahead sync for the others
    p1, st1 = before[1]
    assert torch.equal(ps[1].detach(), p1)
    for key, val in st1.items():
        assert torch.equal(opt.state[ps[1]][key], val), key
    for i in (0, 2):
        assert not torch.equal(ps[i].detach(), before[i][0])
        assert torch.equal(ps[i].detach(), opt.state[ps[i]]["slow_buffer"])
    assert float(opt.state[ps[1]]["step"]) == 2          # one count per group
    for p in ps:
        p.grad = None
    snap = [p.detach().clone() for p in ps]
    opt.step()                                   # nobody has a gradient: nothing moves, the count stays
    assert all(torch.equal(p.detach(), q) for p, q in zip(ps, snap)) and float(opt.state[ps[0]]["step"]) == 2


@pytest.mark.parametrize("direction", ["glam_to_reference", "reference_to_glam"])
def test_checkpoints_move_between_this_optimizer_and_the_reference(device, direction):
    shapes = [(12, 20), (20,), (1, 3, 40)]
    torch.manual_seed(4)
    base = [torch.randn(s) for s in shapes]
    grads = _grads(shapes, 12, device)
    kw = dict(lr=1e-2, k=3, weight_decay=1e-3)

    def run(opt, ps, gs):
        for g_step in gs:
            for p, g in zip(ps, g_step):
                p.grad = g.clone()
            opt.step()

    first_cls, second_cls = (optim.Ranger, RefRanger) if direction == "glam_to_reference" else (RefRanger, optim.Ranger)
    ps = [torch.nn.Parameter(x.clone().to(device)) for x in base]
    first = first_cls(ps, **kw)
    run(first, ps, grads[:5])
    sd = first.state_dict()
    assert all(type(st["step"]) is int and st["step"] == 5 for st in sd["state"].values())
    sd = copy.deepcopy(sd)                                 # (as torch.save / torch.load would hand it over)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    second = second_cls(qs, **kw)
    second.load_state_dict(sd)
    run(first, ps, grads[5:])
    run(second, qs, grads[5:])
    for i, (a, b) in enumerate(zip(ps, qs)):
        _close(b, a, 12, f"{direction}: tensor {i}")
        for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            _close(second.state[b][key], first.state[a][key], 12, f"{direction}: tensor {i} {key}")
        assert int(float(second.state[b]["step"])) == 12


def test_graphed_train_step_follows_the_eager_trajectory_and_recaptures(device):
    """trainer.py:286-301 with Ranger: eager, one graph per batch and 16 steps per graph launch agree bit for bit over 24 steps at k = 6
    (rectification switch, four syncs), with ReduceLROnPlateau moving lr and k / N_sma_threshhold / alpha changed between epochs."""
    from glam_amd.data import DataLoader, synth_molecule
    from glam_amd.graphs import GraphedTrainStep
    rng = np.random.default_rng(4)
    mols = [synth_molecule(rng) for _ in range(24)]
    torch.manual_seed(6)
    net0 = model.Architecture(mol_block="_TripletMessage", message_steps=2, mol_readout="GlobalPool5", e_dim=64).to(device).train()
    loss_fn = lambda out, b: torch.nn.functional.mse_loss(out.view(-1), b.y.view(-1)) * LOSS_SCALE
    results = {}
    for mode in ("eager", "graph", "multi"):
        net = copy.deepcopy(net0)
        ops.manual_seed(77, device)
        opt = optim.Ranger(net.parameters(), lr=2.0 ** -9, k=6)
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=0)
        loader = DataLoader(mols, batch_size=8, device=device)
        stepper = GraphedTrainStep(net, opt, loss_fn)
        for epoch in range(10):
            if epoch == 5:
                opt.param_groups[0]["k"] = 4
                opt.N_sma_threshhold = 4
                opt.alpha = 0.25
            if mode == "multi":
                stepper.run(list(loader), steps_per_graph=16)
            else:
                for b in loader:
                    if mode == "graph":
                        stepper(b)
                    else:
                        opt.zero_grad(set_to_none=True)
                        loss_fn(net(b), b).backward()
                        opt.step()
            sched.step(1.0)
        assert float(opt.param_groups[0]["lr"]) == 2.0 ** -18
        results[mode] = [p.detach().clone() for p in net.parameters()]
    for a, b_, c in zip(results["eager"], results["graph"], results["multi"]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b_) and torch.equal(a, c)


def test_graphed_train_step_with_ranger_trains(device):
    from glam_amd.data import Batch, synth_molecule
    from glam_amd.graphs import GraphedTrainStep
    rng = np.random.default_rng(5)
    batch = Batch.from_data_list([synth_molecule(rng) for _ in range(32)]).to(device)
    torch.manual_seed(7)
    net = model.Architecture().to(device)
    opt = optim.Ranger(net.parameters(), lr=1e-3)              # the reference's defaults (lr 1e-3, k = 6)
    stepper = GraphedTrainStep(net, opt, lambda out, b: torch.nn.functional.mse_loss(out.view(-1), b.y.view(-1)) * LOSS_SCALE)
    losses = torch.stack([stepper(batch) for _ in range(48)]).cpu() / LOSS_SCALE
    assert torch.isfinite(losses).all(), losses
    assert stepper.graphs() == 1
    assert losses[-8:].mean() < 0.5 * losses[0], losses
