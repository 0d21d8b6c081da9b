"""The backward of the panel fusion (csrc/pairpanel_bwd.hip, ``glam_pair_pool_panel_bwd``) restated in numpy, IN THE KERNEL'S ORDER, and the
pieces the CPU and GPU tests of it share: the forward it differentiates, the expanded pair list, the autograd twin on that list, and six
WRONG variants of the restatement that the twin bound must catch.

    ligand l, rows a:   S_l = 0, + w[l, j] * prosum[sel[j]] for j ascending;  d_mol[a] = S_l, then fma(g[l, j, 0], pro[arg[l, j, 1]], .)
                        for the j whose maximum sits on row a, j ascending, + add_mol[a] last
    protein q, rows b:  S_q = 0, + w[l, j] * molsum[l] for the pairs (l, j) with sel[j] == q in ascending l * Qs + j;  d_pro[b] = S_q, then
                        fma(g[l, j, 0], mol[arg[l, j, 0]], .) for those of them whose maximum sits on row b, same order, + add_pro[b] last
    w[l, j] = g[l, j, 1] / (n_l * n_q), the product taken in the working precision; an empty ligand or protein (arg = -1) adds nothing.

A product ``w * sum`` is rounded before it is added (the kernel stages it through LDS); the max terms are fused multiply-adds."""
import numpy as np
import torch

WRONG = ("ignores_duplicates", "garbage_to_unselected", "scales_by_n_l_only", "max_term_on_every_row", "swaps_argmax_columns",
         "counts_empty_segments")


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(list(sizes), dtype=torch.long))


def by_protein(sel, Q):
    """``(order, ptr)``: the stable argsort of ``sel`` and the offsets of the proteins' runs — what ``PanelPlan.by_protein`` must hold."""
    sel = np.asarray(sel, dtype=np.int64)
    order = np.array(sorted(range(len(sel)), key=lambda j: sel[j]), dtype=np.int64)        # (Python's sort is stable)
    ptr = np.zeros(Q + 1, dtype=np.int64)
    for q in sel:
        ptr[q + 1:] += 1
    return order, ptr


def panel_fwd(mol, pro, ms, ps, sel):
    """``out [L, Qs, 2]`` (fp64), ``arg [L, Qs, 2]`` (rows of ``mol`` / ``pro``; -1 for an empty side) of the panel, pair by pair; ties go
    to the smallest flattened index, as in the kernels."""
    mol, pro = np.asarray(mol, dtype=np.float64), np.asarray(pro, dtype=np.float64)
    mp, pp = ptr_of(ms), ptr_of(ps)
    L, Qs = len(ms), len(sel)
    out, arg = np.zeros((L, Qs, 2)), np.full((L, Qs, 2), -1, dtype=np.int64)
    for l in range(L):
        for j, q in enumerate(sel):
            if ms[l] == 0 or ps[q] == 0:
                continue
            S = mol[mp[l]:mp[l + 1]] @ pro[pp[q]:pp[q + 1]].T
            k = int(np.argmax(S))
            out[l, j] = S.max(), S.mean()
            arg[l, j] = mp[l] + k // ps[q], pp[q] + k % ps[q]
    return out, arg


def _fma(a, x, acc, dt):
    if dt == np.float64:
        return a * x + acc
    return (np.float64(a) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)      # (a * x is exact in fp64)


def panel_bwd(mol, pro, ms, ps, sel, arg, g, add_mol=None, add_pro=None, dtype=np.float32, wrong=None):
    """``(d_mol, d_pro)`` in ``dtype``, every sum in the kernel's order.  ``wrong``: one of ``WRONG`` — the same code with one mistake."""
    assert wrong is None or wrong in WRONG
    dt = np.dtype(dtype).type
    mol, pro, g = np.asarray(mol, dtype=dt), np.asarray(pro, dtype=dt), np.asarray(g, dtype=dt)
    arg = np.asarray(arg, dtype=np.int64)
    if wrong == "swaps_argmax_columns":
        arg = arg[..., ::-1]
    mp, pp = ptr_of(ms), ptr_of(ps)
    L, Qs, Q, D = len(ms), len(sel), len(ps), mol.shape[1]
    molsum = np.stack([mol[mp[l]:mp[l + 1]].sum(0, dtype=dt) for l in range(L)]) if L else np.zeros((0, D), dt)
    prosum = np.stack([pro[pp[q]:pp[q + 1]].sum(0, dtype=dt) for q in range(Q)]) if Q else np.zeros((0, D), dt)
    order, qptr = by_protein(sel, Q)
    first_use = [j for j in range(Qs) if sel[j] not in list(sel[:j])]
    d_mol, d_pro = np.zeros_like(mol), np.zeros_like(pro)

    def w(l, j):
        nl, nq = ms[l], ps[sel[j]]
        if wrong == "counts_empty_segments":
            nl, nq = max(nl, 1), max(nq, 1)
        if nl <= 0 or nq <= 0:
            return None
        return g[l, j, 1] / (dt(nl) if wrong == "scales_by_n_l_only" else dt(nl) * dt(nq))

    def role(own_rows, own_col, pairs, partner_sum, partner_rows, out):
        r0, r1 = own_rows
        if r1 <= r0:
            return
        S = np.zeros(D, dt)
        for l, j in pairs:
            wt = w(l, j)
            if wt is not None:
                S = S + (wt * partner_sum(l, j)).astype(dt)
        rows = np.tile(S, (r1 - r0, 1))
        for l, j in pairs:
            own, oth = arg[l, j, own_col], arg[l, j, 1 - own_col]
            if wrong == "counts_empty_segments" and own < 0:
                own, oth = r0, 0                                           # an empty pair treated as one with a maximum
            if own < 0 or oth < 0 or oth >= partner_rows.shape[0]:
                continue
            hit = range(r0, r1) if wrong == "max_term_on_every_row" else ([own] if r0 <= own < r1 else [])
            for r in hit:
                rows[r - r0] = _fma(g[l, j, 0], partner_rows[oth], rows[r - r0], dt)
        out[r0:r1] = rows

    for l in range(L):
        js = first_use if wrong == "ignores_duplicates" else range(Qs)
        role((mp[l], mp[l + 1]), 0, [(l, j) for j in js], lambda l, j: prosum[sel[j]], pro, d_mol)
    for q in range(Q):
        js = [int(j) for j in order[qptr[q]:qptr[q + 1]]]
        if wrong == "ignores_duplicates":
            js = js[:1]
        role((pp[q], pp[q + 1]), 1, [(l, j) for l in range(L) for j in js], lambda l, j: molsum[l], mol, d_pro)
        if wrong == "garbage_to_unselected" and not js:
            d_pro[pp[q]:pp[q + 1]] = 1.0
    if add_mol is not None:
        d_mol = d_mol + np.asarray(add_mol, dtype=dt)
    if add_pro is not None:
        d_pro = d_pro + np.asarray(add_pro, dtype=dt)
    return d_mol, d_pro


def expanded(ms, ps, sel, skip_empty=False):
    """The expanded pair list of the table, ligand-major: ``(pairs, mol_rows, mol_batch, pro_rows, pro_batch)`` — pair ``i`` of ``pairs``
    is ``(l, j)``, ``mol_rows`` / ``pro_rows`` gather the physically replicated rows.  ``skip_empty``: without the pairs that have an empty
    side (the reference's loop has no value for them; they contribute nothing)."""
    mp, pp = ptr_of(ms), ptr_of(ps)
    pairs = [(l, j) for l in range(len(ms)) for j in range(len(sel)) if not (skip_empty and (ms[l] == 0 or ps[sel[j]] == 0))]
    mol_rows = np.concatenate([np.arange(mp[l], mp[l + 1]) for l, _ in pairs] + [np.zeros(0, dtype=np.int64)])
    pro_rows = np.concatenate([np.arange(pp[sel[j]], pp[sel[j] + 1]) for _, j in pairs] + [np.zeros(0, dtype=np.int64)])
    return (pairs, torch.from_numpy(mol_rows), batch_of([ms[l] for l, _ in pairs]), torch.from_numpy(pro_rows),
            batch_of([ps[sel[j]] for _, j in pairs]))


def twin_on_expanded(fusion, mol, pro, ms, ps, sel, d_out, extra=None, skip_empty=False):
    """``run(dtype)`` for ``assert_twin_parity``: ``fusion(mol_rows, pro_rows, mol_batch, pro_batch, P, 2)`` (the oracle's
    ``dot_and_global_pool``) on the expanded pair list under autograd -> ``out [L, Qs, 2]``, ``[d_mol, d_pro]`` with the copies' gradients
    summed per row.  ``extra(mol, pro) -> scalar``: a second use of the two matrices (held once)."""
    pairs, mrows, mb, prows, pb = expanded(ms, ps, sel, skip_empty)
    L, Qs = len(ms), len(sel)

    def run(dt):
        m, p = mol.detach().to(dt).clone().requires_grad_(True), pro.detach().to(dt).clone().requires_grad_(True)
        out = torch.zeros(L, Qs, 2, dtype=dt)
        loss = m.sum() * 0 + p.sum() * 0
        if pairs:
            o = fusion(m[mrows], p[prows], mb, pb, len(pairs), 2)
            at = torch.tensor(pairs)
            loss = loss + (o * d_out.to(dt)[at[:, 0], at[:, 1]]).sum()
            out[at[:, 0], at[:, 1]] = o.detach()
        if extra is not None:
            loss = loss + extra(m, p)
        gm, gp = torch.autograd.grad(loss, [m, p])
        return out, [gm, gp]
    return run
