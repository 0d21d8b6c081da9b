"""The factored pair head (``ops.pair_head``, csrc/pairhead.hip) restated in torch (a helper, not a test module): over a table the first
linear layer of the head separates into a row part, a column part and the fusion columns' part,

    out[i, j, o] = b1[o] + sum_e w1[o, e] * act(A[i, e] + B[j, e] + sum_k Wf[e, k] * f[i, j, k])
    A = flat_a @ W0[:, :hid].T + b0,   B = flat_b @ W0[:, hid:2 hid].T,   Wf = W0[:, 2 hid:]

in whatever precision the inputs come in — and the listed head it must equal, ``lin_out1(lin_out0(cat rows))`` of the oracle's
``linear_block`` assembly on the ``R * Cs`` pair rows.  ``WRONG``: four restatements someone could have written instead; the host test
shows that the comparison sees each of them."""
import torch

import oracle.glam_oracle as O

WRONG = ("act_before_b", "no_fusion", "wf_from_hid", "b0_twice")
ACTS = {"none": ("_None", 0.0), "relu": ("ReLU", 0.0), "leaky": ("LeakyReLU", 0.01)}       # op name -> (the oracle's name, its slope)


def act_fn(h, act, slope):
    if act == "none":
        return h
    if act == "relu":
        return torch.relu(h)
    assert act == "leaky", act
    return torch.where(h > 0, h, h * slope)


def factored(flat_a, flat_b, f, W0, b0, w1, b1, act="none", slope=0.0, wrong=None):
    """``[R, Cs, out_dim]`` in the inputs' dtype; ``f`` ``[R, Cs, F]`` or ``None``."""
    R, Cs, hid = flat_a.size(0), flat_b.size(0), flat_a.size(1)
    F = 0 if f is None else f.size(2)
    assert W0.size(1) == 2 * hid + F
    A = flat_a @ W0[:, :hid].T + b0                                           # [R, e_dim]
    B = flat_b @ W0[:, hid:2 * hid].T                                         # [Cs, e_dim]
    if wrong == "b0_twice":
        B = B + b0
    Wf = W0[:, hid:hid + F] if wrong == "wf_from_hid" else W0[:, 2 * hid:]
    fus = 0 if (F == 0 or wrong == "no_fusion") else f @ Wf.T                 # [R, Cs, e_dim]
    if wrong == "act_before_b":
        h = act_fn(A[:, None, :] + fus, act, slope) + B[None, :, :]
    else:
        h = act_fn(A[:, None, :] + B[None, :, :] + fus, act, slope)
    return h @ w1.T + b1


def pair_rows(flat_a, flat_b, f):
    """The ``R * Cs`` input rows of the listed head, row-major: row ``i * Cs + j`` = ``cat[flat_a[i], flat_b[j], f[i, j]]``."""
    R, Cs = flat_a.size(0), flat_b.size(0)
    parts = [flat_a.repeat_interleave(Cs, 0), flat_b.repeat(R, 1)] + ([] if f is None else [f.reshape(R * Cs, -1)])
    return torch.cat(parts, dim=-1)


def listed(flat_a, flat_b, f, W0, b0, w1, b1, act="none"):
    """The head as the models assemble it, out of the oracle's ``linear_block``: ``lin_out1(lin_out0(rows))`` -> ``[R, Cs, out_dim]``.
    ``act``: a key of ``ACTS`` (the oracle's LeakyReLU has the slope 0.01)."""
    sd = {"lin_out0.linear.weight": W0, "lin_out0.linear.bias": b0, "lin_out1.linear.weight": w1, "lin_out1.linear.bias": b1}
    hidden = O.linear_block(sd, "lin_out0.", pair_rows(flat_a, flat_b, f), ACTS[act][0])
    return O.linear_block(sd, "lin_out1.", hidden, "_None").view(flat_a.size(0), flat_b.size(0), -1)


def inputs(R, Cs, hid, e_dim, F, out_dim, seed=0, dtype=torch.float64):
    """``(flat_a, flat_b, f, W0, b0, w1, b1)`` on the CPU, drawn once per shape from ``seed``; weights at the scale of ``torch.nn.Linear``'s
    initialisation, so that the hidden values straddle zero (both branches of the activation are taken)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)       # noqa: E731
    K = 2 * hid + F
    t = (rnd(R, hid), rnd(Cs, hid), rnd(R, Cs, F) if F else None, rnd(e_dim, K) / K ** 0.5, rnd(e_dim) / K ** 0.5,
         rnd(out_dim, e_dim) / e_dim ** 0.5, rnd(out_dim) / e_dim ** 0.5)
    return tuple(None if x is None else x.to(dtype) for x in t)
