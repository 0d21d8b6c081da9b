"""The phantom tail of a fixed-capacity batch, restated in numpy from its definition — the oracle of
``glam_collate_padded`` for everything behind the real rows."""
import numpy as np


def phantom_layout(N, E, N_cap, E_cap):
    """A batch with ``N`` real nodes and ``E`` real edges in tensors of ``N_cap`` / ``E_cap`` rows: phantom node ``p`` (id ``N + p``, ``P = N_cap
    - N`` of them) owns a contiguous run of ``q + (p < rem)`` self-loops, ``q, rem = divmod(E_cap - E, P)``.  Returns a dict of int64 arrays:
    ``starts`` / ``lens`` [P]; ``rowptr`` = entries ``[N, N_cap]`` of rowptr and colptr (closed by ``E_cap``); ``src`` / ``eid`` = entries
    ``[E, E_cap)`` of src = dst and eid = eid_t; ``edge_index`` [2, E_pad]; ``ell_nodes`` / ``ell_edges`` [P, 4] (the run in order, -1 in the free
    slots; ``None`` where a run is longer than 4)."""
    P, E_pad = N_cap - N, E_cap - E
    assert P >= 1 and E_pad >= 0
    q, rem = divmod(E_pad, P)
    p = np.arange(P, dtype=np.int64)
    lens = q + (p < rem)
    starts = E + p * q + np.minimum(p, rem)
    owner = np.repeat(N + p, lens)
    out = {"starts": starts, "lens": lens, "rowptr": np.concatenate([starts, [E_cap]]), "src": owner, "eid": np.arange(E, E_cap, dtype=np.int64),
           "edge_index": np.stack([owner, owner]), "ell_nodes": None, "ell_edges": None}
    if int(lens.max()) <= 4:
        k = np.arange(4, dtype=np.int64)[None, :]
        used = k < lens[:, None]
        out["ell_nodes"] = np.where(used, (N + p)[:, None], -1)
        out["ell_edges"] = np.where(used, starts[:, None] + k, -1)
    return out


def stable_grouping(keys, other, num_nodes):
    """Brute force: ``(rowptr, other sorted, eid)`` of the edges grouped by ``keys``, stable inside every group."""
    eid = np.argsort(keys, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=num_nodes))])
    return rowptr, other[eid], eid
