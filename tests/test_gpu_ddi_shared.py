"""GPU (MI355X): DDI training on drugs that are held once — ``glam_pair_pool_gather_train_fwd`` (csrc/pairgather.hip),
``glam_pair_pool_gather_bwd`` (csrc/pairgather_bwd.hip), ``ops.pair_pool_gather_shared`` and ``ArchitectureDDI.forward_shared`` on top.

What everything rests on: with every drug held ONCE on each side and a pair = two indices, the forward is bit for bit the inference
fusion (``ops.pair_pool_gather``), and the gradient of a drug's rows — on either side — is the sum of its copies' gradients in the batch of
physically gathered rows, taken in a fixed order, so two runs agree bit for bit.  The reference of every fusion case is the oracle's
``dot_and_global_pool`` on the gathered rows under autograd (which sums the copies), in fp32 and fp64.  ``forward_shared`` is then checked,
output and every parameter gradient, against the oracle's two-drug model on the expanded batches."""
import copy

import numpy as np
import pytest
import torch

import oracle.glam_oracle as O
from glam_amd import _lib, model, ops
from glam_amd._lib import GlamHipError
from glam_amd.data import Batch, synth_batch, synth_molecule
from tests.conftest import assert_close, assert_twin_parity

pytestmark = pytest.mark.gpu


def _batch(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))


def _ptr(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def _gathered(x, sizes, idx):
    off = _ptr(sizes)
    return torch.cat([x[off[q]:off[q + 1]] for q in idx]), _batch([sizes[q] for q in idx])


def _oracle_on_gathered(x1, x2, s1, s2, i1, i2, d_out, extra=None):
    """``run(dtype)`` for ``assert_twin_parity``: the oracle's fusion on physically gathered rows under autograd -> out, [d_x1, d_x2]
    (autograd sums the copies per drug).  ``extra(x1, x2) -> scalar``: a second use of the two matrices (held once)."""
    def run(dt):
        a, b = x1.to(dt).clone().requires_grad_(True), x2.to(dt).clone().requires_grad_(True)      # (clones: the inputs stay plain data)
        r1, b1 = _gathered(a, s1, i1)
        r2, b2 = _gathered(b, s2, i2)
        o = O.dot_and_global_pool(r1, r2, b1, b2, len(i1), 2)
        loss = (o * d_out.to(dt)).sum()
        if extra is not None:
            loss = loss + extra(a, b)
        return o.detach(), list(torch.autograd.grad(loss, [a, b]))
    return run


def _arg_of(out):
    return next(t for t in out.grad_fn.saved_tensors if t.dtype == torch.int32 and t.dim() == 2)


def _setup(s1, s2, D, P, device, seed, positive=False):
    torch.manual_seed(seed)
    x1, x2 = torch.randn(sum(s1), D), torch.randn(sum(s2), D)
    if positive:
        x1, x2 = x1.abs(), x2.abs()
    d_out = torch.randn(P, 2)
    sp1, sp2 = ops.SegmentPtr(_batch(s1).to(device), len(s1)), ops.SegmentPtr(_batch(s2).to(device), len(s2))
    return x1, x2, d_out, sp1, sp2


def _shared_grads(x1, x2, d_out, sp1, sp2, i1, i2, device, runs=2):
    a, b = x1.to(device).requires_grad_(True), x2.to(device).requires_grad_(True)
    out = ops.pair_pool_gather_shared(a, b, sp1, sp2, i1, i2)
    gs = [torch.autograd.grad(out, [a, b], d_out.to(device), retain_graph=True) for _ in range(runs)]
    return out, gs


# Nine drugs; tower 1 and tower 2 hold their own rows of each (the same Batch on both sides).  First-side segments of 1, 2, 33 and 70 rows,
# second-side segments of 1, 63, 64, 65 and 130 rows (one chunk of 64 lanes less one, exactly, plus one, and three chunks); drug 3 is
# first in three pairs, drug 5 second in three; pair 0 is drug 0 with itself; pairs 2 and 6 are the same pair; drug 8 is never referenced.
_SIZES = [1, 2, 33, 70, 63, 64, 65, 130, 7]
_FIRST = [0, 3, 2, 3, 1, 3, 2, 0, 1]
_SECOND = [0, 4, 5, 6, 7, 5, 5, 7, 4]


@pytest.mark.parametrize("D", [4, 15, 16, 60, 64, 92, 128])
def test_gather_shared_fusion_against_the_gathered_call(device, D):
    """16 lanes per row (4, 16, 60, 64), 32 (92, 128) and the dword form (15); with both indices, either one alone (the other side
    physically gathered) and neither."""
    P = len(_FIRST)
    x1, x2, d_out, sp, _ = _setup(_SIZES, _SIZES, D, P, device, D)
    g1, gb1 = _gathered(x1, _SIZES, _FIRST)
    g2, gb2 = _gathered(x2, _SIZES, _SECOND)
    gs1, gs2 = [_SIZES[q] for q in _FIRST], [_SIZES[q] for q in _SECOND]
    gsp1, gsp2 = ops.SegmentPtr(gb1.to(device), P), ops.SegmentPtr(gb2.to(device), P)
    ident = list(range(P))
    cases = {"both": (x1, x2, _SIZES, _SIZES, sp, sp, _FIRST, _SECOND, _FIRST, _SECOND),
             "idx1 only": (x1, g2, _SIZES, gs2, sp, gsp2, _FIRST, None, _FIRST, ident),
             "idx2 only": (g1, x2, gs1, _SIZES, gsp1, sp, None, np.asarray(_SECOND), ident, _SECOND),
             "neither": (g1, g2, gs1, gs2, gsp1, gsp2, None, None, ident, ident)}
    for what, (a, b, s1, s2, p1, p2, i1, i2, r1, r2) in cases.items():
        out, ((da, db), (da2, db2)) = _shared_grads(a, b, d_out, p1, p2, i1, i2, device)
        with torch.no_grad():
            ref, ref_arg = ops.pair_pool_gather(a.to(device), b.to(device), p1, p2, i1, i2, return_argmax=True)
        assert torch.equal(out.detach(), ref), f"{what}: forward differs from pair_pool_gather"
        assert torch.equal(_arg_of(out), ref_arg), f"{what}: argmax differs from pair_pool_gather"
        assert torch.equal(da, da2) and torch.equal(db, db2), f"{what}: a second backward differs from the first"
        for g, sizes, used, side in ((da, s1, r1, "x1"), (db, s2, r2, "x2")):
            off = _ptr(sizes)
            for q in set(range(len(sizes))) - set(used):
                assert g[off[q]:off[q + 1]].abs().max().item() == 0.0, f"{what}: unreferenced segment {q} of {side} must get zeros"
        assert_twin_parity(_oracle_on_gathered(a, b, s1, s2, r1, r2, d_out), out, [da, db], f"pair_pool_gather_shared D={D} {what}",
                           names=["x1", "x2"])


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("D", [60, 15])
def test_gather_shared_fusion_colliding_maxima(device, D, side):
    """Non-negative rows and one row of the shared drug scaled by 50: all five pairs have their maximum on THAT row, whose gradient is
    five fmaf terms in batch order on top of the common sum — once for a row of x1, once for a row of x2."""
    shared_sizes, partner_sizes, shared, partners = [6, 40], [3, 9, 1, 70, 5], [1] * 5, [0, 1, 2, 3, 1]
    s1, s2, i1, i2 = (shared_sizes, partner_sizes, shared, partners) if side == 1 else (partner_sizes, shared_sizes, partners, shared)
    x1, x2, d_out, sp1, sp2 = _setup(s1, s2, D, 5, device, 100 + D + side, positive=True)
    row = 6 + 17
    (x1 if side == 1 else x2)[row] *= 50
    out, ((d1, d2), (d1b, d2b)) = _shared_grads(x1, x2, d_out, sp1, sp2, i1, i2, device)
    assert _arg_of(out)[:, side - 1].tolist() == [row] * 5, "the case must put every pair's maximum on one row"
    assert torch.equal(d1, d1b) and torch.equal(d2, d2b)
    run = _oracle_on_gathered(x1, x2, s1, s2, i1, i2, d_out)
    assert_twin_parity(run, out, [d1, d2], f"colliding maxima D={D} side {side}", names=["x1", "x2"])
    got = (d1, d2)[side - 1]
    assert_twin_parity(lambda dt: (run(dt)[0], [run(dt)[1][side - 1][row]]), out, [got[row]], f"colliding maxima D={D} side {side}, the row",
                       names=["row"])
    assert got[:6].abs().max().item() == 0.0


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("D", [60, 92])
def test_gather_shared_fusion_many_pairs_on_one_drug(device, D, side):
    """70 pairs on one 40-row drug of one side (partners of 1-3 rows, identity on their side): its pair list is longer than a staged
    tile of 64."""
    many, one = [1 + (i % 3) for i in range(70)], [40]
    s1, s2, i1, i2 = (one, many, [0] * 70, None) if side == 1 else (many, one, None, [0] * 70)
    x1, x2, d_out, sp1, sp2 = _setup(s1, s2, D, 70, device, 200 + D + side)
    out, ((d1, d2), (d1b, d2b)) = _shared_grads(x1, x2, d_out, sp1, sp2, i1, i2, device)
    assert torch.equal(d1, d1b) and torch.equal(d2, d2b)
    ident = list(range(70))
    assert_twin_parity(_oracle_on_gathered(x1, x2, s1, s2, i1 or ident, i2 or ident, d_out), out, [d1, d2], f"many pairs D={D} side {side}",
                       names=["x1", "x2"])


@pytest.mark.parametrize("D", [60, 15])
def test_gather_shared_fusion_empty_segments(device, D):
    s1, s2, i1, i2 = [3, 0, 5], [0, 6, 4], [0, 1, 2, 2], [1, 1, 0, 2]          # pair 1: no first-side row; pair 2: no second-side row
    x1, x2, d_out, sp1, sp2 = _setup(s1, s2, D, 4, device, 3)
    out, ((d1, d2), _) = _shared_grads(x1, x2, d_out, sp1, sp2, i1, i2, device)
    arg = _arg_of(out)
    assert out[1:3].abs().max().item() == 0.0 and (arg[1:3] == -1).all() and (arg[0] >= 0).all() and (arg[3] >= 0).all()
    assert torch.isfinite(d1).all() and torch.isfinite(d2).all()
    live = [0, 3]
    run = _oracle_on_gathered(x1, x2, s1, s2, [i1[i] for i in live], [i2[i] for i in live], d_out[live])
    assert_twin_parity(run, out[live], [d1, d2], f"empty segments D={D}", names=["x1", "x2"])
    # no pair at all
    a, b = x1.to(device).requires_grad_(True), x2.to(device).requires_grad_(True)
    none = ops.pair_pool_gather_shared(a, b, sp1, sp2, [], [])
    assert none.shape == (0, 2)
    ga, gb = torch.autograd.grad(none.sum(), [a, b])
    assert ga.shape == a.shape and gb.shape == b.shape and ga.abs().max().item() == 0.0 and gb.abs().max().item() == 0.0


@pytest.mark.parametrize("D", [60, 15])
def test_gather_shared_fusion_with_identity(device, D):
    """The two matrices handed back through the node: their later gradients are added inside the ONE backward launch, at a 16-byte
    width and at a dword width; gradients of ``fusion + second use`` equal those of the ``with_identity=False`` graph."""
    s1, s2, i1, i2 = [5, 40, 2, 9], [70, 30, 4], [1, 0, 1, 1, 3], [1, 0, 1, 2, 1]
    x1, x2, d_out, sp1, sp2 = _setup(s1, s2, D, 5, device, 300 + D)
    w1, w2 = torch.randn_like(x1), torch.randn_like(x2)
    extra = lambda a, b: (a * a * w1.to(a)).sum() + (b * b * w2.to(b)).sum()      # noqa: E731
    got = []
    for with_identity in (True, False):
        a, b = x1.to(device).requires_grad_(True), x2.to(device).requires_grad_(True)
        if with_identity:
            out, a2, b2 = ops.pair_pool_gather_shared(a, b, sp1, sp2, i1, i2, with_identity=True)
            assert a2 is not a and b2 is not b, "both require grad: the add runs inside the launch for every width of the table"
        else:
            out, a2, b2 = ops.pair_pool_gather_shared(a, b, sp1, sp2, i1, i2), a, b
        loss = (out * d_out.to(device)).sum() + extra(a2, b2)
        with _lib.kernel_timer() as kt:
            gs = torch.autograd.grad(loss, [a, b])
        assert [r[0] for r in kt.records()].count("k_pair_gather_bwd") == 1, "one backward launch per fusion"
        got.append((out, gs))
    run = _oracle_on_gathered(x1, x2, s1, s2, i1, i2, d_out, extra)
    for (out, gs), what in zip(got, ("with_identity", "plain")):
        assert_twin_parity(run, out, list(gs), f"{what} D={D}", names=["x1", "x2"])
    assert torch.equal(got[0][0], got[1][0])
    # one side without a gradient: the plain triple, the matrices themselves
    a, b = x1.to(device).requires_grad_(True), x2.to(device)
    out, a2, b2 = ops.pair_pool_gather_shared(a, b, sp1, sp2, i1, i2, with_identity=True)
    assert a2 is a and b2 is b
    (ga,) = torch.autograd.grad((out * d_out.to(device)).sum() + extra(a2, b2), [a])
    assert_twin_parity(lambda dt: (run(dt)[0], run(dt)[1][:1]), out, [ga], f"one-sided D={D}", names=["x1"])
    # only the handed-back matrices are used: their gradients pass through
    a, b = x1.to(device).requires_grad_(True), x2.to(device).requires_grad_(True)
    _, a2, b2 = ops.pair_pool_gather_shared(a, b, sp1, sp2, i1, i2, with_identity=True)
    ga, gb = torch.autograd.grad((a2 * 2).sum() + (b2 * 3).sum(), [a, b])
    assert torch.equal(ga, torch.full_like(ga, 2)) and torch.equal(gb, torch.full_like(gb, 3))


@pytest.mark.parametrize("K,M,with_bias", [(300, 60, True), (300, 60, False), (60, 15, False), (60, 15, True), (320, 64, True)])
def test_matmul_tall_rows_do_not_depend_on_the_batch_length(device, K, M, with_bias):
    """The first n rows of a 256-row product are bit for bit the product of those n rows alone, below 64 rows, at 64 and above, at a width
    that is no multiple of 4 — and the short call's value and gradients are within the fp64-twin bound of ``a @ w + bias``."""
    torch.manual_seed(K + M)
    a, w, bias = torch.randn(256, K), torch.randn(K, M), torch.randn(M) if with_bias else None
    ad, wd, bd = a.to(device), w.to(device), None if bias is None else bias.to(device)
    with torch.no_grad():
        full = ops.matmul_tall(ad, wd, bd)
        for n in (1, 15, 16, 46, 60, 63, 64, 65, 120):
            part = ops.matmul_tall(ad[:n].contiguous(), wd, bd)
            assert part.shape == (n, M) and torch.equal(part, full[:n]), f"{n} rows alone differ from the same rows of 256"
    n = 46
    cot = torch.randn(n, M)
    leaves = [ad[:n].clone().requires_grad_(True), wd.clone().requires_grad_(True)] + ([bd.clone().requires_grad_(True)] if with_bias else [])
    out = ops.matmul_tall(*leaves)
    grads = torch.autograd.grad(out, leaves, cot.to(device))

    def run(dt):
        ls = [a[:n].to(dt).clone().requires_grad_(True), w.to(dt).clone().requires_grad_(True)] + ([bias.to(dt).clone().requires_grad_(True)] if with_bias else [])
        o = ls[0] @ ls[1] + (ls[2] if with_bias else 0)
        return o.detach(), list(torch.autograd.grad(o, ls, cot.to(dt)))
    assert_twin_parity(run, out, list(grads), f"matmul_tall {n} x {K} x {M}", names=["a", "w", "bias"][:len(leaves)])


# ---------------------------------------------------------------------------------------------
# ArchitectureDDI.forward_shared
# ---------------------------------------------------------------------------------------------
_ACTS = dict(pre_act="ReLU", graph_act="ReLU", flat_act="ReLU", end_act="ReLU")
_I1 = [0, 1, 2, 2, 0, 1]          # 6 pairs over 3 first-side ...
_I2 = [0, 1, 1, 0, 1, 1]          # ... and 2 second-side drugs


def _drugs(seed, n):
    rng = np.random.default_rng(seed)
    return [synth_molecule(rng) for _ in range(n)]


def _net(**kw):
    torch.manual_seed(12)
    return model.ArchitectureDDI(e_dim=64, message_steps=2, graph_do="_None()", end_do="_None()", **_ACTS, **kw).eval()


@pytest.mark.parametrize("mol_block,norm,alpha", [("_NNConv", "_None", 4), ("_TripletMessage", "_PairNorm", 4),
                                                  ("_TripletMessageLight", "_LayerNorm", 4), ("_NNConv", "_None", 1)])
def test_forward_shared_vs_oracle_on_the_expanded_batches(device, monkeypatch, mol_block, norm, alpha):
    """Output and every parameter gradient of ``forward_shared(drugs1, drugs2, first, second)`` against the oracle's two-drug model on the
    batches of ``drugs1[first]`` / ``drugs2[second]`` collated one per pair (autograd on its state dict), once in ``eval()`` and once in
    ``train()`` (nothing here is stochastic: the two runs are equal); every step's fusion maximum is bit-equal to that of ``model(B1, B2)``."""
    d1, d2 = _drugs(3, 3), _drugs(5, 2)
    B1, B2 = Batch.from_data_list([d1[q] for q in _I1]), Batch.from_data_list([d2[q] for q in _I2])
    net = _net(mol_block=mol_block, graph_norm=norm, hid_dim_alpha=alpha)
    names = [n for n, _ in net.named_parameters()]
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    torch.manual_seed(1)
    cot = torch.randn(6, 1)

    def run(dt):
        sd = {k: (v.to(dt).requires_grad_(True) if k in names else v.to(dt)) for k, v in sd0.items()}
        cast = lambda b: type(b)(b.x.to(dt), b.edge_index, b.edge_attr.to(dt), batch=b.batch)      # noqa: E731
        out = O.architecture_ddi(sd, cast(B1), cast(B2), 6, message_steps=2, mol_block=mol_block, graph_norm=norm, **_ACTS)
        return out.detach(), list(torch.autograd.grad(out, [sd[n] for n in names], cot.to(dt), allow_unused=True))

    net = net.to(device)
    net.graphed_call = False
    seen = {"model": [], "shared": []}

    def spy(name, key):
        inner = getattr(model, name)

        def f(*a, **k):
            r = inner(*a, **k)
            seen[key].append(r[0].detach().clone())
            return r
        monkeypatch.setattr(model, name, f)
    spy("dot_and_global_pool2", "model")
    spy("dot_and_global_pool2_gather_shared", "shared")
    m1, m2 = Batch.from_data_list(d1).to(device), Batch.from_data_list(d2).to(device)
    results = []
    for training in (False, True):
        net.train(training)
        out = net.forward_shared(m1, m2, _I1, _I2)
        results.append((out.detach(), torch.autograd.grad(out, list(net.parameters()), cot.to(device), allow_unused=True)))
    net.eval()
    with torch.no_grad():
        net(B1.to(device), B2.to(device))
    (out, grads), (out_t, grads_t) = results
    assert out.shape == (6, 1) and torch.equal(out, out_t)
    for n, a, b in zip(names, grads, grads_t):
        assert (a is None and b is None) or torch.equal(a, b), f"eval() and train() differ in d_{n}"
    o64, g64 = run(torch.float64)
    for n, a, r in zip(names, grads, g64):
        assert (a is None) == (r is None), f"{n}: a gradient on one side only"
    assert_twin_parity(run, out, list(grads), f"forward_shared {mol_block}/{norm}/alpha={alpha}", names=names)
    assert len(seen["shared"]) == 4 and len(seen["model"]) == 2
    for s in range(2):           # (the exact comparison of the maxima is the next test's)
        assert_close(seen["shared"][s], seen["model"][s], 1e-5, f"step {s}: fusion")


def _fusion_maxima(device, monkeypatch, d1, d2, i1, i2, **kw):
    """Every step's fusion output of ``forward_shared`` on the distinct drugs and of ``model(B1, B2)`` on the expanded batches (the
    monkeypatch spy of the test above), both in ``eval()`` under ``no_grad``."""
    net = _net(**kw).to(device)
    net.graphed_call = False
    seen = {"dot_and_global_pool2": [], "dot_and_global_pool2_gather_shared": []}
    for name in seen:
        def f(*a, _inner=getattr(model, name), _into=seen[name], **k):
            r = _inner(*a, **k)
            _into.append(r[0].detach().clone())
            return r
        monkeypatch.setattr(model, name, f)
    with torch.no_grad():
        net.forward_shared(Batch.from_data_list(d1).to(device), Batch.from_data_list(d2).to(device), i1, i2)
        net(Batch.from_data_list([d1[q] for q in i1]).to(device), Batch.from_data_list([d2[q] for q in i2]).to(device))
    shared, full = seen["dot_and_global_pool2_gather_shared"], seen["dot_and_global_pool2"]
    assert len(shared) == len(full) == 2
    return shared, full


@pytest.mark.parametrize("mol_block,norm,alpha", [("_NNConv", "_None", 4), ("_TripletMessage", "_PairNorm", 4),
                                                  ("_TripletMessageLight", "_LayerNorm", 4), ("_NNConv", "_None", 1)])
def test_forward_shared_fusion_max_is_that_of_model(device, monkeypatch, mol_block, norm, alpha):
    """6 pairs over 3 + 2 drugs: every step's fusion maximum ``torch.equal`` to that of ``model(B1, B2)``.

    3 drugs are 60 rows and 2 drugs 46, the expanded batches 120 and 138: the towers' rows must not depend on the length of the batch around
    them.  ``_NNConv``'s relation product (``ops.matmul_tall``, ``[N, 300] x [300, 60]`` and at hid = 15 ``[N, 60] x [60, 15]``) therefore
    runs its HIP forward kernel below 64 rows and at odd widths too (``_MatmulTallRows``), not a library GEMM that picks its kernel — and
    its roundings — by the row count."""
    shared, full = _fusion_maxima(device, monkeypatch, _drugs(3, 3), _drugs(5, 2), _I1, _I2, mol_block=mol_block, graph_norm=norm,
                                  hid_dim_alpha=alpha)
    for s in range(2):
        assert torch.equal(shared[s][:, 0], full[s][:, 0]), f"step {s}: the fusion max differs from model(B1, B2)"


@pytest.mark.parametrize("alpha", [4, 1])
def test_forward_shared_fusion_max_is_that_of_model_from_64_rows(device, monkeypatch, alpha):
    """``_NNConv`` with 9 pairs over 6 + 6 drugs (132 and 116 rows, on the other side of the 64-row line of ``ops.matmul_tall``): every
    step's fusion maximum is ``torch.equal`` to that of ``model(B1, B2)`` here too."""
    i1, i2 = [0, 3, 2, 3, 1, 3, 2, 5, 4], [0, 4, 5, 1, 2, 5, 5, 2, 3]
    shared, full = _fusion_maxima(device, monkeypatch, _drugs(3, 6), _drugs(5, 6), i1, i2, mol_block="_NNConv", hid_dim_alpha=alpha)
    for s in range(2):
        assert torch.equal(shared[s][:, 0], full[s][:, 0]), f"step {s}: the fusion max differs from model(B1, B2)"


def test_forward_shared_default_stochastic_configuration_trains(device):
    """The reference's defaults (RReLU, Dropout(0.2)) in ``train()``: noise is drawn once per distinct drug — it runs, every parameter gets
    a finite gradient and each tower gets one that is not zero.  Both sides read the SAME Batch here."""
    torch.manual_seed(2)
    net = model.ArchitectureDDI().to(device).train()
    ops.manual_seed(4, device)
    drugs = synth_batch(4, seed=3).to(device)
    out = net.forward_shared(drugs, drugs, [0, 1, 2, 3, 3, 0], [1, 1, 0, 2, 3, 0])
    assert out.shape == (6, 1)
    out.sum().backward()
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    for mod in ("mol1_lin0", "mol1_conv", "mol1_flat", "mol2_lin0", "mol2_conv", "mol2_flat"):
        assert max(p.grad.abs().max().item() for p in getattr(net, mod).parameters()) > 0, f"{mod} got no gradient"


class _SharedStep(torch.nn.Module):
    """What a trainer wraps around ``forward_shared`` for ``GraphedTrainStep`` (which calls ``model(batch)``)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, batch):
        return self.net.forward_shared(batch.mol1, batch.mol2, batch.first, batch.second)


class _PairBatch:
    def __init__(self, mol1, mol2, first, second, y):
        self.mol1, self.mol2, self.first, self.second, self.y = mol1, mol2, first, second, y


def test_forward_shared_is_captured_by_graphed_train_step(device):
    """Two batches, four visits under ``GraphedTrainStep`` (eager, captured, replayed, replayed) in the default training configuration
    follow the eager trajectory — one batch with ``PairIndex``es kept across the steps, one with the default indices the model keeps."""
    from glam_amd.graphs import GraphedTrainStep
    torch.manual_seed(7)
    net0 = model.ArchitectureDDI(e_dim=64, message_steps=2).to(device).train()
    a, b, c = synth_batch(3, seed=21).to(device), synth_batch(2, seed=22).to(device), synth_batch(4, seed=23).to(device)
    torch.manual_seed(8)
    batches = [_PairBatch(a, b, ops.pair_index(_I1, 6, 3, name="first", over="drugs"), ops.pair_index(_I2, 6, 2, name="second", over="drugs"),
                          torch.randn(6, device=device)),
               _PairBatch(c, c, None, None, torch.randn(4, device=device))]
    loss_fn = lambda out, bt: torch.nn.functional.mse_loss(out.view(-1), bt.y.view(-1))      # noqa: E731
    results = []
    for graphed in (False, True):
        step = _SharedStep(copy.deepcopy(net0))
        opt = torch.optim.Adam(step.parameters(), lr=1e-3, capturable=True)
        stepper = GraphedTrainStep(step, opt, loss_fn)
        ops.manual_seed(5, device)
        losses = []
        for _visit in range(4):
            for bt in batches:
                if graphed:
                    losses.append(float(stepper(bt)))
                else:
                    opt.zero_grad(set_to_none=True)
                    loss = loss_fn(step(bt), bt)
                    loss.backward()
                    opt.step()
                    losses.append(float(loss.detach()))
        if graphed:
            assert stepper.graphs() == 2
        results.append((losses, [p.detach().clone() for p in step.parameters()]))
    (l_e, p_e), (l_g, p_g) = results
    assert np.allclose(l_e, l_g, rtol=1e-5, atol=1e-6), (l_e, l_g)
    for got, ref in zip(p_g, p_e):
        assert_close(got, ref, 1e-5, "parameter")


def test_capturing_an_index_without_device_copies_is_refused(device):
    """The device copies of an index and of its by-drug lists come from an eager first visit: a capture cannot make them."""
    torch.manual_seed(3)
    from glam_amd.graphs import _gc_paused
    x1, x2 = torch.randn(12, 60, device=device), torch.randn(9, 60, device=device)
    sp1, sp2 = ops.SegmentPtr(_batch([5, 7]).to(device), 2), ops.SegmentPtr(_batch([4, 5]).to(device), 2)
    kept1, kept2 = ops.pair_index([0, 1, 1], 3, 2, name="idx1", over="segments of x1"), ops.pair_index([1, 1, 0], 3, 2, name="idx2", over="segments of x2")
    with torch.no_grad():
        eager = ops.pair_pool_gather_shared(x1, x2, sp1, sp2, kept1, kept2)          # the eager first visit makes the copies
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with _gc_paused(), torch.cuda.graph(graph):
            with pytest.raises(GlamHipError, match="keep ONE PairIndex across the steps"):
                ops.pair_pool_gather_shared(x1, x2, sp1, sp2, [0, 1, 1], [1, 1, 0])      # fresh indices: no copy on the device yet
            captured = ops.pair_pool_gather_shared(x1, x2, sp1, sp2, kept1, kept2)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, eager)


def test_forward_shared_refusals_come_before_any_launch(device):
    m1, m2 = synth_batch(3, seed=3).to(device), synth_batch(2, seed=5).to(device)
    gsn, ln, bn, net = (_net(graph_norm="_GraphSizeNorm").to(device), _net(flat_norm="_LayerNorm").to(device),
                        _net(graph_norm="_BatchNorm").to(device), _net().to(device))
    odd = _net().to(device)
    odd.mol2_flat.norm = ln.mol2_flat.norm                                        # the SECOND tower alone
    with _lib.kernel_timer() as kt:
        with pytest.raises(GlamHipError, match="mol1_conv's norm _GraphSizeNorm"):
            gsn.forward_shared(m1, m2, _I1, _I2)
        with pytest.raises(GlamHipError, match="mol1_flat's norm _LayerNorm"):
            ln.forward_shared(m1, m2, _I1, _I2)
        with pytest.raises(GlamHipError, match="mol2_flat's norm _LayerNorm"):
            odd.forward_shared(m1, m2, _I1, _I2)
        with pytest.raises(GlamHipError, match="mol1_conv's norm _BatchNorm"):
            bn.train().forward_shared(m1, m2, _I1, _I2)
        for bad1, bad2 in ((_I1, [0, 1, 1]), (_I1, _I2 + [0]), ([0, 1, 3, 2, 0, 1], _I2), (_I1, [0, 1, 2, 0, 1, 1]), (_I1, None), (None, _I2),
                           (None, None)):          # wrong lengths, out of range, identity with Q != P
            with pytest.raises(IndexError):
                net.forward_shared(m1, m2, bad1, bad2)
        with pytest.raises(GlamHipError, match="read-back"):
            net.forward_shared(m1, m2, torch.tensor(_I1, device=device), _I2)
        with pytest.raises(GlamHipError, match="read-back"):
            net.forward_shared(m1, m2, _I1, torch.tensor(_I2, device=device))
    assert kt.records() == [], "a refusal launched something"
    with torch.no_grad():
        assert bn.eval().forward_shared(m1, m2, _I1, _I2).shape == (6, 1)            # running statistics are per row: accepted
        assert net.forward_shared(m1, m2, _I1, _I2).shape == (6, 1)
        assert net.forward_shared(m1, m1).shape == (3, 1)                            # identity on both sides of one Batch
