"""``glam_pair_list_load`` (csrc/pairlist.hip) and the host table builders of the resident pair batches (``glam_amd.data``), restated in
numpy from their definitions — the oracle of the kernel on the GPU and of the builders on the host — with the case list both test files
walk and the WRONG restatements the comparison must catch (the style of ``tests/index_cases.py``).

The kernel, per present side: ``idx[i] = col[ids[i]]`` for ``i < B`` and ``pad`` behind; ``order`` = the stable argsort of ``idx``; ``ptr`` =
``[0] + cumsum(bincount(idx, minlength=Q))``; and ``y_out[i] = y[ids[i]]``.  Restated here slot by slot and segment by segment (no argsort,
no bincount): the comparison against ``ops.PairsByProtein`` in the host tests is then one between two independent derivations."""
import numpy as np

WRONG = ("unstable", "stale_phantom", "open_ptr", "pad_ignored", "ghost_run", "y_by_slot")


def pair_list_restated(ids, col, B, P, Q, pad, wrong=None, previous=None):
    """``(idx, order, ptr)`` int32 of one side.  ``ids``: the step's pair ids (``None`` = identity); ``previous``: the ``idx`` the load before
    left (what a builder that skips the phantom slots would keep).  ``wrong``: one of ``WRONG`` (``y_by_slot`` concerns ``labels_restated``)."""
    col = np.asarray(col)
    ids = np.arange(B) if ids is None else np.asarray(ids)
    idx = np.empty(P, dtype=np.int32)
    for i in range(P):
        if i < B:
            idx[i] = col[ids[i]]
        elif wrong == "stale_phantom":
            idx[i] = pad if previous is None else previous[i]
        elif wrong == "pad_ignored":
            idx[i] = col[0]
        else:
            idx[i] = pad
    order, ptr = [], [0]
    for q in range(Q):
        run = [i for i in range(P) if idx[i] == q]               # ascending i: the stable order
        if wrong == "unstable":
            run = run[::-1]
        if wrong == "ghost_run" and not run:
            run = [0]                                            # an unreferenced segment handed a pair
        order += run
        ptr.append(len(order))
    if wrong == "ghost_run":
        order = order[:P] + [0] * max(0, P - len(order))
    if wrong == "open_ptr":
        ptr[Q] = 0                                               # the closing entry never written
    return idx, np.asarray(order, dtype=np.int32), np.asarray(ptr, dtype=np.int32)


def labels_restated(ids, y, B, wrong=None):
    """``y_out [B, r]``: the label rows of the step's pairs, in slot order."""
    ids = np.arange(B) if ids is None else np.asarray(ids)
    if wrong == "y_by_slot":
        return np.stack([y[i] for i in range(B)]) if B else y[:0]
    return np.stack([y[ids[i]] for i in range(B)]) if B else y[:0]


def reference_lists(idx, Q):
    """What the issue names as the truth: numpy's stable argsort and the cumulative bincount."""
    return (np.argsort(idx, kind="stable").astype(np.int32),
            np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=Q))]).astype(np.int32))


def cases():
    """The smallest cases at which one wave per segment over rounds of 64 keys — or any tiled alternative — can go wrong.  Each: ``name``,
    ``P``, ``B``, ``Q``, ``pad``, ``col`` int32 ``[Np]`` (the resident pair column), ``y`` float32 ``[Np, 3]`` and ``loads``: two or more
    DIFFERENT id vectors of length ``B`` for one object, so that residue shows."""
    g = np.random.default_rng(29)
    out = []

    def add(name, P, B, Q, pad=0, col=None, loads=None, Np=None):
        Np = Np or max(2 * P, 8)
        col = g.integers(0, Q, Np).astype(np.int32) if col is None else np.asarray(col, dtype=np.int32)
        Np = col.shape[0]
        loads = loads or [g.permutation(Np)[:B] for _ in range(2)]
        y = g.standard_normal((Np, 3)).astype(np.float32)
        out.append(dict(name=name, P=P, B=B, Q=Q, pad=pad, col=col, y=y, loads=[np.asarray(l, dtype=np.int64) for l in loads]))

    add("one pair", 1, 1, 1)
    add("one full round", 64, 64, 3)
    add("a second key round", 65, 65, 3)
    add("one segment owns every pair, five rounds", 300, 300, 1)
    add("padding slots, Q beyond a block of waves, most segments empty", 130, 100, 700, pad=3)
    rev = np.arange(257)[::-1]
    add("every run of length 1, descending input", 257, 257, 257, col=rev, loads=[np.arange(257), g.permutation(257)])
    add("keys all Q - 1: the closing entry", 70, 70, 5, col=np.concatenate([np.full(70, 4), g.integers(0, 5, 70)]),
        loads=[np.arange(70), 70 + g.permutation(70)])
    add("repeated pair ids within one load", 40, 40, 6, loads=[g.integers(0, 10, 40), g.integers(5, 20, 40)])
    add("padding behind a short load, pad = Q - 1", 96, 33, 4, pad=3)
    return out


# ---------------------------------------------------------------------------------------------
# the host table builders of glam_amd.data, restated
# ---------------------------------------------------------------------------------------------
def dti_table_restated(pair_ids, first, ns, es):
    """``[4 * (B + 1) + B]``: the ligand slot table — ids (one entry of padding), then the exclusive node / edge / y offsets of the slots,
    each closed by its total (no y rows: zeros) — and the pair ids behind it; with the node and edge totals."""
    pair_ids = [int(p) for p in pair_ids]
    B = len(pair_ids)
    table = np.zeros((4, B + 1), dtype=np.int64)
    n = e = 0
    for i, p in enumerate(pair_ids):
        lig = int(first[p])
        table[0, i] = lig
        table[1, i], table[2, i] = n, e
        n, e = n + int(ns[lig]), e + int(es[lig])
    table[1, B], table[2, B] = n, e
    return np.concatenate([table.reshape(-1), np.asarray(pair_ids, dtype=np.int64)]).astype(np.int32), n, e


def ddi_table_restated(pair_ids):
    return np.asarray([int(p) for p in pair_ids], dtype=np.int32)
