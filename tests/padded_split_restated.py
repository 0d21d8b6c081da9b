"""The phantom tail of a fixed-capacity batch whose surplus nodes are cut into ``K`` bounded phantom graphs, restated in
numpy from its definition — the oracle of ``glam_collate_padded_split`` for everything behind the real rows.  The edge runs are per node,
so the edge, CSR and ELL tails are those of ``tests.padded_restated.phantom_layout``; what the cut adds is ``batch`` and ``ptr``."""
import numpy as np

from tests.padded_restated import phantom_layout


def split_layout(N, E, N_cap, E_cap, B, K):
    """``phantom_layout(N, E, N_cap, E_cap)`` plus, for ``K`` phantom graphs behind ``B`` real ones (``s, r = divmod(N_cap - N, K)``):
    ``counts`` [K] = ``s + (j < r)``, the nodes of phantom graph ``j``; ``ptr`` [K + 1] = entries ``[B, B + K]`` of the batch's ``ptr``
    (``N + j s + min(j, r)``, closed by ``N_cap``); ``batch`` [P] = entries ``[N, N_cap)`` of the batch vector, built by repetition rather
    than by the closed form the kernel evaluates."""
    P = N_cap - N
    assert 1 <= K <= P
    out = phantom_layout(N, E, N_cap, E_cap)
    s, r = divmod(P, K)
    j = np.arange(K + 1, dtype=np.int64)
    out["counts"] = s + (j[:K] < r)
    out["ptr"] = N + j * s + np.minimum(j, r)
    out["batch"] = np.repeat(B + j[:K], out["counts"])
    return out
