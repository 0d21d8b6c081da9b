"""Shared by tests/test_triplet_cases_host.py (CPU) and tests/test_gpu_triplet_kernels.py (GPU): the graphs on which the fused
gather / softmax / scatter kernels of ``TripletMessage`` can go wrong, seeded inputs for them, and a plain restatement of the
aggregate (``aggregate_ref``) evaluated in fp64 and fp32.  Plain torch; imports no HIP and nothing of ``glam_amd``.

Why these graphs: the general kernels (csrc/triplet_kernels.h) walk the CSR segment of a node ``CH`` edges at a time (4 at
``ITER == 1``, 2 otherwise), clamp the slots past the segment's end to its last edge and mask them; the backward by target changes
its formula once a segment is longer than one chunk.  ``degree_ladder`` therefore puts one node on each side of every such edge —
0, 1, CH - 1, CH, CH + 1, 2 CH, 2 CH + 1, 63 / 64 / 65, 130 — and adds what a molecular batch never holds: directed edges, self-loops,
a duplicated edge, isolated nodes at both ends of the node range.  ``ell_mix`` builds the three edge lists on which the layer's
forward and its two backward launches are picked from DIFFERENT kernel families (in-degree <= 4 vs out-degree <= 4)."""
import types

import torch
import torch.nn.functional as F

import oracle.glam_oracle as O

LADDER = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 130, 0, 1]


def degree_ladder(in_degrees=LADDER, seed=0, directed=True, flip=False):
    """One graph in which node ``i < len(in_degrees)`` has exactly ``in_degrees[i]`` incoming edges; behind them filler nodes of
    in-degree 2 (so that the widest segment can draw distinct sources and N is odd: no multiple of 16, 32 or 64) and one last node
    without any edge.  Node 0 must be requested with in-degree 0: it and the last node are isolated (neither source nor target).
    Sources are drawn at random without repetition inside a segment and never equal the target, except for what is put in on purpose:

    * ``loop_only``: the first node of in-degree 1 — its only incoming edge is a self-loop;
    * ``loop_in``: the first node of in-degree >= 5 (more than one chunk at either ``CH``) — one of its incoming edges is a self-loop;
    * ``dup``: the first node of in-degree >= 7 — two of its incoming edges come from the same source ``dup_src``.

    The edge order is shuffled.  ``directed=False`` appends the mirror image of every edge (an undirected graph: in- and out-degree
    agree, each at least the requested value).  ``flip=True`` swaps the rows of ``edge_index``: the same ladder on the OUT-degrees,
    which is what the backward by source walks.  Returns a namespace ``edge_index[2, E]`` int64, ``N``, ``loop_only``, ``loop_in``,
    ``dup``, ``dup_src``, ``isolated`` (node ids as they stand in ``edge_index`` after ``flip``) and ``ladder``."""
    deg = list(in_degrees)
    assert deg[0] == 0 and 1 in deg and max(deg) >= 7, "the ladder needs in-degrees 0 (first), 1 and >= 7"
    g = torch.Generator().manual_seed(seed)
    n_fill = max(0, max(deg) + 8 - len(deg))
    n_fill += (len(deg) + n_fill + 1) % 2 == 0                 # N odd
    N = len(deg) + n_fill + 1
    deg = deg + [2] * n_fill + [0]
    loop_only = deg.index(1)
    loop_in = next(i for i, d in enumerate(deg) if d >= 5)
    dup = next(i for i, d in enumerate(deg) if d >= 7)
    src, dst = [], []
    dup_src = None
    for n, d in enumerate(deg):
        if d == 0:
            continue
        cand = torch.tensor([j for j in range(1, N - 1) if j != n])       # nodes 0 and N - 1 stay isolated
        s = cand[torch.randperm(cand.numel(), generator=g)[:d]].tolist()
        assert len(s) == d
        if n == loop_only:
            s = [n]
        if n == loop_in:
            s[int(torch.randint(0, d, (1,), generator=g))] = n
        if n == dup:
            a, b = (0, d - 1) if n != loop_in else [k for k in range(d) if s[k] != n][:2]
            s[b] = s[a]                                                    # first and last edge of the segment as drawn
            dup_src = s[a]
        src += s
        dst += [n] * d
    ei = torch.tensor([src, dst], dtype=torch.long)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    if not directed:
        ei = torch.cat([ei, ei.flip(0)], 1)
    if flip:
        ei = ei.flip(0)
    return types.SimpleNamespace(edge_index=ei.contiguous(), N=N, loop_only=loop_only, loop_in=loop_in, dup=dup, dup_src=dup_src,
                                 isolated=(0, N - 1), ladder=list(in_degrees))


def degrees(edge_index, N):
    """``(in_degree[N], out_degree[N])`` of an edge list."""
    return torch.bincount(edge_index[1], minlength=N), torch.bincount(edge_index[0], minlength=N)


def stride_graph(N, hub, seed=0, hub_degree=130):
    """``N`` nodes of in-degree ``n % 4`` (0..3: inside one chunk) with sources drawn within 64 ids of the target, and ``hub_degree``
    incoming edges at node ``hub`` — for the grid-stride cases, where ``hub`` lies in the part of the node range that a block reaches
    only on its second trip."""
    g = torch.Generator().manual_seed(seed)
    d = torch.arange(N) % 4
    d[hub] = hub_degree
    dst = torch.repeat_interleave(torch.arange(N), d)
    off = torch.randint(1, 64, (dst.numel(),), generator=g)
    src = (dst + off) % N
    ei = torch.stack([src, dst])
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


def ring_lattice(N, seed=0):
    """Every node bonded to its neighbours at distance 1 and 2 around a ring: in- and out-degree exactly 4 at any ``N``, one-hot bond
    rows of width 4 — the molecular form (warp-specialised kernels) at sizes beyond their grid caps.  ``(edge_index, edge_attr, N)``."""
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(N)
    b = torch.cat([torch.stack([n, (n + 1) % N]), torch.stack([n, (n + 2) % N])], 1)
    kind = torch.randint(0, 4, (b.size(1),), generator=g)
    ei = torch.cat([b, b.flip(0)], 1)
    ea = F.one_hot(torch.cat([kind, kind]), 4).float()
    perm = torch.randperm(ei.size(1), generator=g)
    return ei[:, perm].contiguous(), ea[perm].contiguous(), N


def molecules(seed=0, sizes=(5, 9, 14, 20, 7, 11, 17, 6, 23, 12, 8, 15)):
    """A batch of molecule-like graphs, as ``glam_amd.data.synth_batch`` collates them: every bond in both directions, at most 4 bonds
    per atom (at least one atom with exactly 4), one-hot bond rows of width 4 shared by the two directions of a bond.  Returns
    ``(edge_index[2, E], edge_attr[E, 4], N)``."""
    g = torch.Generator().manual_seed(seed)
    bonds, off = [], 0
    for n in sizes:
        d = [0] * n
        adj = set()
        for k in range(1, n):
            free = [j for j in range(k) if d[j] < 3]
            j = free[int(torch.randint(0, len(free), (1,), generator=g))]
            adj.add((j, k)); d[j] += 1; d[k] += 1
        for _ in range(2):                                  # ring closures: up to 4 bonds per atom
            free = [j for j in range(n) if d[j] < 4]
            pairs = [(a, b) for a in free for b in free if a < b and (a, b) not in adj]
            if pairs:
                a, b = pairs[int(torch.randint(0, len(pairs), (1,), generator=g))]
                adj.add((a, b)); d[a] += 1; d[b] += 1
        bonds += [(a + off, b + off) for a, b in sorted(adj)]
        off += n
    b = torch.tensor(bonds, dtype=torch.long).t()
    kind = torch.randint(0, 4, (b.size(1),), generator=g)
    ei = torch.cat([b, b.flip(0)], 1)
    ea = F.one_hot(torch.cat([kind, kind]), 4).float()
    assert int(degrees(ei, off)[0].max()) == 4
    return ei.contiguous(), ea, off


def ell_mix(kind, seed=0, sizes=None):
    """The three edge lists on which ``TripletMessage`` mixes its kernel families (forward by ``in-degree <= 4``, backward by source by
    ``out-degree <= 4``), each with one-hot bond rows of width 4.  Returns ``(edge_index, edge_attr, N)``.

    * ``"a"``: a plain symmetric molecule batch (both hold; the mix comes from asking for ``d_edge_attr``);
    * ``"b"``: directed edges added until exactly one atom has 5 outgoing edges; every in-degree stays <= 4;
    * ``"c"``: the mirror image — exactly one atom has 5 incoming edges; every out-degree stays <= 4."""
    ei, ea, N = molecules(seed) if sizes is None else molecules(seed, sizes)
    if kind == "a":
        return ei, ea, N
    assert kind in ("b", "c")
    g = torch.Generator().manual_seed(seed + 1)
    din = degrees(ei, N)[0]
    hub = int(torch.argmax(din))                               # an atom with 4 bonds: one directed edge more makes 5
    nbrs = set(ei[1][ei[0] == hub].tolist()) | {hub}
    free = [v for v in range(N) if din[v] <= 3 and v not in nbrs]
    other = free[int(torch.randint(0, len(free), (1,), generator=g))]
    extra = torch.tensor([[hub], [other]])                     # hub -> other: out-degree 5 at hub, in-degree <= 4 at other
    if kind == "c":
        extra = extra.flip(0)
    ei = torch.cat([ei, extra], 1)
    ea = torch.cat([ea, F.one_hot(torch.randint(0, 4, (1,), generator=g), 4).float()])
    perm = torch.randperm(ei.size(1), generator=g)
    return ei[:, perm].contiguous(), ea[perm].contiguous(), N


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def aggregate_ref(xw, a_ij, edge_attr, w_edge, M, edge_index, H, Cp, slope, emul):
    """The formula above ``glam_triplet_fwd`` in include/glam_hip.h, in the dtype of its inputs (differentiable):

        logit[e, h] = leaky_relu(a_ij[dst, h] + sum_k edge_attr[e, k] M[k, h] + a_ij[src, 4 + h], slope)
        alpha       = segment softmax of logit over the incoming edges of dst (max-shifted, +1e-16: ``O.segment_softmax``)
        emul = 1:   aggr[n, h, :] = sum_e alpha[e, h] (sum_k edge_attr[e, k] w_edge[k, h, :]) xw[src, h, :]
        emul = 0:   aggr[n, h, :] = sum_e alpha[e, h] xw[src, h, :]

    ``xw[N, H*Cp]``, ``a_ij[N, 8]``, ``edge_attr[E, De]``, ``w_edge[De, H*Cp]`` (``None`` at ``emul = 0``), ``M[De, 4]``.  A node
    without incoming edges gets a zero row."""
    src, dst = edge_index[0], edge_index[1]
    N = xw.size(0)
    logit = a_ij[:, :H].index_select(0, dst) + (edge_attr @ M)[:, :H] + a_ij[:, 4:4 + H].index_select(0, src)
    alpha = O.segment_softmax(F.leaky_relu(logit, slope), dst, N)
    msg = alpha.unsqueeze(-1) * xw.index_select(0, src).view(-1, H, Cp)
    if emul:
        msg = msg * (edge_attr @ w_edge).view(-1, H, Cp)
    return O.scatter(msg, dst, N, "sum").reshape(N, H * Cp)


def layer_ref(x, edge_index, edge_attr, weight_node, weight_edge, weight_triplet_att, weight_scale=None, bias=None, heads=3,
              slope=0.2):
    """``O.triplet_message`` — ``O.triplet_message_light`` when ``weight_edge`` is ``None``."""
    if weight_edge is None:
        return O.triplet_message_light(x, edge_index, edge_attr, weight_node, weight_triplet_att, bias, slope)
    return O.triplet_message(x, edge_index, edge_attr, weight_node, weight_edge, weight_triplet_att, weight_scale, bias, heads, slope)


def staged_operands(x, edge_attr, weight_node, weight_edge, weight_triplet_att, H):
    """``(xw, a_ij, w_edge, M)`` of ``aggregate_ref`` from a TripletMessage's parameters, mapped as ``TripletMessage._staged_weights()``
    maps them (unpadded): ``a_ij = x @ Wa`` with ``Wa`` from the node thirds of ``weight_triplet_att`` through ``weight_node``, ``M``
    from its edge third through ``weight_edge``.  The light layer (``weight_edge is None``, ``att[1, 2C + De]``, one head): the edge
    part of ``att`` IS ``M``'s first column."""
    C = weight_node.size(0)
    att = weight_triplet_att[0]
    if weight_edge is None:
        De = att.numel() - 2 * C
        Wa = weight_node @ torch.stack([att[:C], att[C + De:]], dim=-1)                 # [C, 2]
        a_ij = F.pad((x @ Wa).unsqueeze(-1), (0, 3)).reshape(-1, 8)
        return x @ weight_node, a_ij, None, F.pad(att[C:C + De].unsqueeze(-1), (0, 3))
    De = weight_edge.size(0)
    Wn = weight_node.view(C, H, C)
    a_i = torch.einsum("nc,chk,hk->nh", x, Wn, att[:, :C])
    a_j = torch.einsum("nc,chk,hk->nh", x, Wn, att[:, 2 * C:])
    M = torch.einsum("dhk,hk->dh", weight_edge.view(De, H, C), att[:, C:2 * C])
    return x @ weight_node, torch.cat([F.pad(a_i, (0, 4 - H)), F.pad(a_j, (0, 4 - H))], 1), weight_edge, F.pad(M, (0, 4 - H))


def aggregate_inputs(edge_index, N, H, Cp, De, emul, seed, kind="normal", pad_from=None):
    """Seeded fp32 CPU operands of ``aggregate_ref`` / ``ops.triplet_aggregate`` and a cotangent, as a dict.  ``kind``:

    * ``"normal"``: unit normal everything (logits of order 1);
    * ``"ties"``: ``M = 0`` and ``a_ij = 0`` — every logit is 0, alpha is exactly 1 / in-degree;
    * ``"wide"``: ``a_ij`` scaled by 25 — the bulk of the logits spans about +-60 and the tail passes 88.7, where ``exp`` leaves fp32
      (a softmax without its max shift gives inf / nan there; with it every term is <= 1);

    The head columns ``H..3`` of ``a_ij`` and ``M`` are zero, as the layer's staging pads them.  ``pad_from``: columns
    ``pad_from..Cp-1`` of every head of ``xw`` and ``w_edge`` are zero (a width the layer pads to a multiple of four)."""
    g = torch.Generator().manual_seed(seed)
    E = edge_index.size(1)
    xw = torch.randn(N, H, Cp, generator=g)
    a_ij = torch.randn(N, 2, 4, generator=g)
    ea = torch.randn(E, De, generator=g)
    we = torch.randn(De, H, Cp, generator=g) if emul else None
    M = torch.randn(De, 4, generator=g) * 0.5
    cot = torch.randn(N, H * Cp, generator=g)
    a_ij[:, :, H:] = 0
    M[:, H:] = 0
    if kind == "ties":
        a_ij.zero_(); M.zero_()
    elif kind == "wide":
        a_ij *= 25.0
    else:
        assert kind == "normal"
    if pad_from is not None:
        xw[:, :, pad_from:] = 0
        if emul:
            we[:, :, pad_from:] = 0
    return dict(xw=xw.reshape(N, H * Cp), a_ij=a_ij.reshape(N, 8), edge_attr=ea, w_edge=we.reshape(De, H * Cp) if emul else None, M=M,
                cot=cot)


AGG_NAMES = ("xw", "a_ij", "edge_attr", "w_edge", "M")


def run_aggregate_ref(inp, edge_index, H, Cp, slope, emul, dtype, fn=aggregate_ref, want_dea=True):
    """``(aggr, [d_xw, d_a_ij, d_edge_attr, d_w_edge, d_M])`` of ``fn`` (default: ``aggregate_ref``) with autograd on the CPU in
    ``dtype``, under the cotangent ``inp["cot"]``; ``d_w_edge`` is ``None`` at ``emul = 0``, ``d_edge_attr`` without ``want_dea``."""
    ts = {n: (inp[n].to(dtype).requires_grad_(n != "edge_attr" or want_dea) if inp[n] is not None else None) for n in AGG_NAMES}
    out = fn(ts["xw"], ts["a_ij"], ts["edge_attr"], ts["w_edge"], ts["M"], edge_index, H, Cp, slope, emul)
    leaves = [ts[n] for n in AGG_NAMES if ts[n] is not None and ts[n].requires_grad]
    gs = iter(torch.autograd.grad((out * inp["cot"].to(dtype)).sum(), leaves, allow_unused=True))
    grads = [(next(gs) if (ts[n] is not None and ts[n].requires_grad) else None) for n in AGG_NAMES]
    grads = [torch.zeros_like(ts[n]) if (g is None and ts[n] is not None and ts[n].requires_grad) else g for g, n in zip(grads, AGG_NAMES)]
    return out.detach(), grads
