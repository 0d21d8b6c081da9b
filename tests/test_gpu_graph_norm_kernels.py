"""GPU (MI355X): every dispatch form of the graph-norm kernels (csrc/norm.hip: PairNorm, mode 0, and the graph LayerNorm statistics,
mode 1) against the oracle evaluated in fp64 and fp32 on the CPU, GRAPH BY GRAPH (tests/graph_norm_cases.py).

Each direction has three kernel forms and a fused norm + Dropout form:

  wave per graph, float4   k_graph_norm_fwd_v4 / _bwd_v4 <MODE, false>    D % 4 == 0, D <= 64, N / B < 64, 16-byte-aligned tensors
  block per graph          k_graph_norm_fwd_block / _bwd_block <MODE>     D % 4 == 0, D <= 64, N / B >= 64, 16-byte-aligned tensors
  generic, lane / channel  k_graph_norm_fwd / _bwd <MODE>                 any other D <= 256, and any unaligned tensor
  norm + Dropout           k_graph_norm_fwd_v4 / _bwd_v4 <MODE, true>     glam_graph_norm_drop_fwd / _bwd, the wave form's shapes

The form follows the AVERAGE graph size, so the wave form meets graphs of hundreds of rows (and the phantom graph of a padded resident
batch) and the block form meets 1-row and empty graphs: the size lists hold both.  Every test reads the launched kernel names from
``kernel_timer`` — a case that quietly takes another route fails — runs its op twice and asserts bit-equal results (the kernels reduce
in a fixed order), and holds every graph to the fp64-twin bound of its own rows.  tests/test_graph_norm_host.py shows on the CPU that an
independent fp32 evaluation of the same inputs stays within half that bound."""
import pytest
import torch

from glam_amd import _lib, ops
from glam_amd._lib import GlamHipError, kernel_timer
from tests import graph_norm_cases as C

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
MAX_BLOCKS = 2048                   # common.h: kMaxBlocks, the grid cap behind the grid-stride loops


def _kernel(direction, form, mode, drop=False):
    """The name ``kernel_timer`` records for a launch: the first argument of the launch macro as written in norm.hip (without the
    parentheses that guard a template argument list's comma)."""
    if form == "wave":
        return f"k_graph_norm_{direction}_v4<{mode}, {'true' if drop else 'false'}>"
    if form == "block":
        return f"k_graph_norm_{direction}_block<{mode}>"
    return f"k_graph_norm_{direction}<{mode}>"


def _unaligned(t):
    """A contiguous view of ``t``'s values at a 4-byte storage offset of a real allocation (16-byte alignment broken, in bounds;
    differentiable: the gradient arrives at ``t``)."""
    flat = torch.cat([t.new_zeros(1), t.reshape(-1)])
    u = flat[1:].view(t.shape)
    assert u.data_ptr() % 16 != 0
    return u


def _norm_launches(kt):
    return [(n, g) for n, g, _ in kt.records() if "k_graph_norm" in n]


def _run_ops(device, setting, sizes, x, cot, cot_id=None, wrap=None):
    """``ops.pair_norm`` / ``ops.graph_standardize`` forward and backward on the device -> ``(y, dx, [(kernel name, grid)])``."""
    kind, scale, eps = setting
    sp = ops.SegmentPtr(C.batch_of(sizes).to(device), len(sizes))
    xd = x.to(device).requires_grad_(True)
    xin = wrap(xd) if wrap else xd
    identity = cot_id is not None
    with kernel_timer() as kt:
        if kind == "pair":
            out = ops.pair_norm(xin, sp, scale=scale, eps=eps, with_identity=identity)
        else:
            out = ops.graph_standardize(xin, sp, eps=eps, with_identity=identity)
        if identity:
            y, x_id = out
            loss = (y * cot.to(device)).sum() + (x_id * cot_id.to(device)).sum()
        else:
            y, loss = out, (out * cot.to(device)).sum()
        (dx,) = torch.autograd.grad(loss, [xd])
    return y.detach().cpu(), dx.cpu(), _norm_launches(kt)


def _check_case(device, sizes_name, D, setting, form, identity=False, wrap=None, grid=None):
    """Parity per graph, the kernel form, bit-reproducibility, and the exact rows: a 1-row graph under PairNorm (``inv_cnt = 1``, so
    ``x' = x - x = 0``: output 0, gradient 0 or exactly the addend) and a graph of all-zero rows (output 0 in both modes)."""
    assert (sizes_name, D) in C.ALL_CASES, "a new case goes through tests/test_graph_norm_host.py first: add it to graph_norm_cases"
    sizes = C.SIZE_LISTS[sizes_name]
    x, cot, cot_id = C.inputs(sizes_name, D)
    ref = C.reference(sizes_name, D, setting, identity)
    what =f"{sizes_name} D={D} {C.setting_id(setting)} {form}" + (" identity" if identity else "")
    runs = [_run_ops(device, setting, sizes, x, cot, cot_id if identity else None, wrap) for _ in range(2)]
    (y, dx, launches), (y2, dx2, _) = runs
    mode = C.MODE[setting[0]]
    assert [n for n, _ in launches] == [_kernel("fwd", form, mode), _kernel("bwd", form, mode)], f"{what}: launched {launches}"
    if grid is not None:
        assert [g for _, g in launches] == [grid, grid], f"{what}: grids {launches}"
    assert torch.equal(y, y2) and torch.equal(dx, dx2), f"{what}: two runs differ"
    C.assert_per_graph_parity(y, ref[F64][0], ref[F32][0], sizes, what + " out")
    C.assert_per_graph_parity(dx, ref[F64][1], ref[F32][1], sizes, what + " grad.x")
    batch = C.batch_of(sizes)
    one = torch.tensor(sizes)[batch] == 1
    if setting[0] == "pair" and one.any():
        assert (y[one] == 0).all(), f"{what}: 1-row graphs must come out exactly 0"
        assert torch.equal(dx[one], cot_id[one] if identity else torch.zeros_like(dx[one])), f"{what}: gradient rows of 1-row graphs"
    if sizes_name.startswith("ZERO"):
        assert (x[batch == 1] == 0).all() and (y[batch == 1] == 0).all(), f"{what}: the all-zero graph must come out exactly 0"
    return y, dx


# ---------------------------------------------------------------------------------------------
# parity through the ops, form by form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("D", [4, 60, 64])
def test_wave_form(device, D, setting):
    """``k_graph_norm_fwd_v4 / _bwd_v4<MODE, false>`` on WAVE (N // B = 34): empty graphs at both ends and inside, 1 to 8 rows, exactly
    one register pass (32), 33, two passes (64), 65, a partial fourth pass (97) and a 600-row graph.  D = 4 leaves one float4 lane of
    16 active, D = 60 leaves lane 15 idle.  ``scale = 2.5`` reaches the backward's ``a^3 / scale^2``."""
    _check_case(device, "WAVE", D, setting, "wave")


@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("D", [4, 60, 64])
@pytest.mark.parametrize("sizes_name", ["BLOCK", "PHANTOM"])
def test_block_form(device, sizes_name, D, setting):
    """``k_graph_norm_fwd_block / _bwd_block<MODE>``: BLOCK (N // B = 153) holds empty and 1-row graphs, fewer rows than the 16 row
    groups (2, 15), 16, 17, and the edges of ``block_colsum``'s 64-row unroll (48, 49, 63, 64, 65, 113), up to 1 000 rows; PHANTOM is a
    padded resident batch: ten 20-row molecules and one 6 000-row phantom graph."""
    _check_case(device, sizes_name, D, setting, "block")


@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("sizes_name,D", [(n, D) for n in ("WAVE", "BLOCK") for D in (45, 65, 92, 256)] + [("PHANTOM", 92)])
def test_generic_form(device, sizes_name, D, setting):
    """``k_graph_norm_fwd / _bwd<MODE>`` (a lane per channel, up to four 64-channel chunks) at whatever the average graph size: D = 45
    (chunk 0 only), 65 (a single lane in chunk 1), 92 (the padded width of hid_dim_alpha = 6), 256 (all four chunks full)."""
    _check_case(device, sizes_name, D, setting, "generic")


@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("sizes_name,D,form", [("WAVE", 60, "wave"), ("BLOCK", 60, "block"), ("WAVE", 92, "generic"), ("BLOCK", 92, "generic")])
def test_identity_path_adds_the_second_gradient_in_the_store(device, sizes_name, D, form, setting):
    """``with_identity=True`` under the cotangent ``<y, cot1> + <x, cot2>``: ``glam_graph_norm_bwd_add`` in all three forms (the
    ``addend`` argument of ``_bwd_v4<MODE, false>``, ``_bwd_block`` and the generic ``_bwd``) — a single backward launch.  The
    reference is the oracle's norm plus the identity; a 1-row PairNorm graph's gradient is exactly the addend."""
    _check_case(device, sizes_name, D, setting, form, identity=True)


@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("sizes_name,D,form", [("ZERO_WAVE", 60, "wave"), ("ZERO_WAVE", 45, "generic"), ("ZERO_BLOCK", 60, "block")])
def test_a_graph_of_all_zero_rows(device, sizes_name, D, form, setting):
    """A graph whose rows are all 0 (40 rows; 300 in the block form's batch): zero variance, so ``a = scale / sqrt(eps)``; the output
    is exactly 0 in both modes, the gradient ``a (g - gbar)`` stays within the graph's bound.  A 1-row graph sits beside it."""
    _check_case(device, sizes_name, D, setting, form)


@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("sizes_name,D,form", [("STRIDE_WAVE", 8, "wave"), ("STRIDE_WAVE", 6, "generic"), ("STRIDE_BLOCK", 4, "block")])
def test_grid_stride_loops_wrap(device, sizes_name, D, form, setting):
    """9 000 graphs of 1, 2, 3, 1, ... rows (more than 2 048 blocks x 4 waves) through ``_v4`` (D = 8) and the generic kernels (D = 6),
    2 100 graphs of 64 rows (more than 2 048 blocks) through ``_block`` (D = 4): the recorded grid is the cap and the graphs behind
    the first sweep are normalised like the rest (parity per graph)."""
    _check_case(device, sizes_name, D, setting, form, grid=MAX_BLOCKS)


@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
def test_unaligned_views_take_the_generic_kernels(device, setting):
    """A contiguous view at a 4-byte storage offset (D = 60, graphs of 5, 40 and 300 rows: block-form shapes): ``ld4`` / ``st4`` need
    16-byte-aligned rows, so ``glam_graph_norm_fwd`` (unaligned ``x``) and ``glam_graph_norm_bwd`` (the saved unaligned ``x``) must take
    ``k_graph_norm_fwd / _bwd<MODE>``; the aligned tensor of the same values takes the block form and agrees within the bound."""
    _check_case(device, "UNALIGNED", 60, setting, "generic", wrap=_unaligned)
    _check_case(device, "UNALIGNED", 60, setting, "block")


@pytest.mark.parametrize("mode", [0, 1])
def test_unaligned_gradient_and_addend_at_the_c_abi(device, mode):
    """``glam_graph_norm_bwd`` / ``_bwd_add`` with an unaligned ``gy``, ``dx`` or ``addend`` (each alone; everything else aligned): the
    generic ``k_graph_norm_bwd<MODE>`` (``scale = 2.5``), and the very bits it gives when an unaligned ``x`` forces it; with everything
    aligned the same call takes ``k_graph_norm_bwd_block<MODE>``."""
    lib, P = _lib.load(), _lib.ptr
    sizes, D = C.UNALIGNED, 60
    x, cot, cot_id = (t.to(device) for t in C.inputs("UNALIGNED", D))
    N, B = x.size(0), len(sizes)
    sp = ops.SegmentPtr(C.batch_of(sizes).to(device), B)

    def bwd(xx, gy, add, dx):
        with kernel_timer() as kt:
            if add is None:
                rc = lib.glam_graph_norm_bwd(P(xx), P(gy), P(sp.ptr), N, B, D, mode, 2.5, 1e-3, P(dx), _lib.stream())
            else:
                rc = lib.glam_graph_norm_bwd_add(P(xx), P(gy), P(sp.ptr), N, B, D, mode, 2.5, 1e-3, P(add), P(dx), _lib.stream())
        assert rc == 0, lib.glam_last_error()
        return [n for n, _ in _norm_launches(kt)]

    base, base_add = torch.empty_like(x), torch.empty_like(x)
    assert bwd(_unaligned(x), cot, None, base) == [_kernel("bwd", "generic", mode)]
    assert bwd(_unaligned(x), cot, cot_id, base_add) == [_kernel("bwd", "generic", mode)]
    for which in ("gy", "dx", "addend"):
        dx = _unaligned(torch.empty_like(x)) if which == "dx" else torch.empty_like(x)
        names = bwd(x, _unaligned(cot) if which == "gy" else cot, None if which != "addend" else _unaligned(cot_id), dx)
        assert names == [_kernel("bwd", "generic", mode)], f"unaligned {which}: launched {names}"
        assert torch.equal(dx, base_add if which == "addend" else base), f"unaligned {which}"
    dx = torch.empty_like(x)
    assert bwd(x, cot, cot_id, dx) == [_kernel("bwd", "block", mode)]


# ---------------------------------------------------------------------------------------------
# norm + Dropout at the C ABI: k_graph_norm_fwd_v4 / _bwd_v4 <MODE, true>
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("setting", C.SETTINGS, ids=C.setting_id)
@pytest.mark.parametrize("D", [4, 60, 64])
def test_norm_dropout_c_abi(device, D, setting, p):
    """``glam_graph_norm_drop_fwd`` / ``_bwd`` (``k_graph_norm_fwd_v4 / _bwd_v4<MODE, true>``, both modes) on WAVE.

    Forward: ``y`` is bit-equal to ``glam_graph_norm_fwd``; ``y_drop`` is exactly ``y * fl(1 / (1 - p))`` or 0, the same whether ``y``
    is stored or null; the keep rate over the n non-zero elements is within 5 sqrt(p (1 - p) / n) of 1 - p; a second call on the advanced
    stream draws another mask.  Backward with the recorded ``eff``, for ``gy`` in {null, tensor} x ``addend`` in {null, tensor}: the mask
    m is recovered from the forward outputs, the reference is the oracle's autograd under the cotangent ``gy + gy_drop * m / (1 - p)``
    plus the addend, per graph.  Where ``y = 0`` the mask cannot be read off — only in 1-row PairNorm graphs, whose gradient is 0 (or
    the addend) whatever the mask."""
    lib, P = _lib.load(), _lib.ptr
    kind, scale, eps = setting
    mode = C.MODE[kind]
    sizes = C.WAVE
    x, cot, cot_id = C.inputs("WAVE", D)
    batch = C.batch_of(sizes)
    N, B = x.size(0), len(sizes)
    sp = ops.SegmentPtr(batch.to(device), B)
    xd = x.to(device)
    what = f"norm+dropout D={D} {C.setting_id(setting)} p={p}"
    assert lib.glam_graph_norm_drop_supported(N, B, D) == 1

    y_plain = torch.full_like(xd, float("nan"))
    assert lib.glam_graph_norm_fwd(P(xd), P(sp.ptr), N, B, D, mode, scale, eps, P(y_plain), _lib.stream()) == 0, lib.glam_last_error()

    def fwd(seed, want_y):
        st = ops.manual_seed(seed) if seed is not None else ops.rng_state(device)
        eff = torch.full((2,), -1, dtype=torch.int64, device=device)
        y = torch.full_like(xd, float("nan")) if want_y else None
        yd = torch.full_like(xd, float("nan"))
        with kernel_timer() as kt:
            rc = lib.glam_graph_norm_drop_fwd(P(xd), P(sp.ptr), N, B, D, mode, scale, eps, p, P(st), P(eff), P(y), P(yd), _lib.stream())
        assert rc == 0, lib.glam_last_error()
        assert [n for n, _ in _norm_launches(kt)] == [_kernel("fwd", "wave", mode, drop=True)], what
        return y, yd, eff

    y, yd, eff = fwd(77, True)
    _, yd_null, eff_null = fwd(77, False)
    _, yd_next, eff_next = fwd(None, False)                      # not reseeded: the launch before advanced the stream
    assert torch.equal(y, y_plain), f"{what}: y differs from glam_graph_norm_fwd"
    assert torch.equal(yd, yd_null) and torch.equal(eff, eff_null), f"{what}: y_drop depends on whether y is stored"
    inv = torch.ones((), dtype=F32) / (1 - torch.tensor(p, dtype=F32))          # fl(1 / (1 - p)), as drop_scale_w computes it
    kept = y * inv.to(device)
    assert ((yd == kept) | (yd == 0)).all(), f"{what}: y_drop is neither y / (1 - p) nor 0 somewhere"
    live = y != 0
    n = int(live.sum())
    rate = float((yd[live] != 0).float().mean())
    assert abs(rate - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, f"{what}: keep rate {rate:.4f} over {n} elements"
    assert eff.tolist() == [77, 0] and eff_next[0].item() == 77 and eff_next[1].item() > 0, (eff.tolist(), eff_next.tolist())
    assert not torch.equal((yd_next != 0)[live], (yd != 0)[live]), f"{what}: the advanced stream drew the same mask"
    assert ((yd_next == kept) | (yd_next == 0)).all()

    one = (torch.tensor(sizes)[batch] == 1)
    dead = ~live.cpu()
    if mode == 0:
        assert (dead.all(dim=1) == one).all() and not dead[~one].any(), f"{what}: zeros outside the 1-row graphs"
    else:
        assert not dead.any(), f"{what}: an exact zero in the output"
    m = (yd != 0).cpu().double()
    gyd, gy_t, add_t = cot.to(device), cot_id.to(device), cot.flip(0).contiguous().to(device)
    for gy in (None, gy_t):
        for add in (None, add_t):
            outs = []
            for _ in range(2):
                dx = torch.full_like(xd, float("nan"))
                with kernel_timer() as kt:
                    rc = lib.glam_graph_norm_drop_bwd(P(xd), P(gy), P(gyd), P(sp.ptr), N, B, D, mode, scale, eps, p, P(eff), P(add), P(dx),
                                                      _lib.stream())
                assert rc == 0, lib.glam_last_error()
                assert [k for k, _ in _norm_launches(kt)] == [_kernel("bwd", "wave", mode, drop=True)], what
                outs.append(dx.cpu())
            w = f"{what} gy={'null' if gy is None else 'set'} addend={'null' if add is None else 'set'} grad.x"
            assert torch.equal(outs[0], outs[1]), f"{w}: two runs differ"
            c = cot.double() * m / (1 - p) + (0 if gy is None else cot_id.double())
            refs = {dt: C.run_oracle(setting, sizes, x, c, dt)[1] + (0 if add is None else add_t.cpu().to(dt)) for dt in (F64, F32)}
            C.assert_per_graph_parity(outs[0], refs[F64], refs[F32], sizes, w)
            if mode == 0:
                assert torch.equal(outs[0][one], add_t.cpu()[one] if add is not None else torch.zeros_like(outs[0][one])), w


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_library_usable(device):
    """D = 257 (GLAM_E_UNSUPPORTED), mode = 2 (GLAM_E_INVALID), rows that do not equal ``sp.N``: a ``GlamHipError`` or status code
    before any launch, and the next valid call succeeds."""
    lib, P = _lib.load(), _lib.ptr
    sizes = [3, 0, 5]
    sp = ops.SegmentPtr(C.batch_of(sizes).to(device), len(sizes))
    x = torch.randn(8, 12, device=device)
    with kernel_timer() as kt:
        with pytest.raises(GlamHipError, match="D=257"):
            ops.pair_norm(torch.randn(8, 257, device=device), sp)
        with pytest.raises(GlamHipError, match="D=257"):
            ops.graph_standardize(torch.randn(8, 257, device=device), sp)
        with pytest.raises(GlamHipError, match="rows"):
            ops.pair_norm(torch.randn(9, 12, device=device), sp)
        y = torch.empty_like(x)
        assert lib.glam_graph_norm_fwd(P(x), P(sp.ptr), 8, 3, 12, 2, 1.0, 1e-5, P(y), _lib.stream()) == _lib.GLAM_E_INVALID
        assert lib.glam_graph_norm_bwd(P(x), P(x), P(sp.ptr), 8, 3, 12, 2, 1.0, 1e-5, P(y), _lib.stream()) == _lib.GLAM_E_INVALID
        assert lib.glam_graph_norm_bwd(P(x), P(x), P(sp.ptr), 8, 3, 257, 0, 1.0, 1e-5, P(y), _lib.stream()) == _lib.GLAM_E_UNSUPPORTED
    assert _norm_launches(kt) == []
    xr = x.clone().requires_grad_(True)
    out = ops.pair_norm(xr, sp)
    (g,) = torch.autograd.grad(out.square().sum(), [xr])
    ref = C.oracle_fn(("pair", 1.0, 1e-5), C.batch_of(sizes), len(sizes))(x.cpu().double())
    assert (out.detach().cpu().double() - ref).abs().max() <= 1e-5 and torch.isfinite(g).all()
