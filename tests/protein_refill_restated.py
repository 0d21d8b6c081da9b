"""The host arithmetic of one load of ``glam_amd.data.ResidentDTIRefillBatch`` restated in plain Python (lists, ``sorted``, ``index``):
which proteins take the batch's slots, in which order, which slot a pair's protein sits in, and the table that one copy carries.  No
numpy tricks, no GPU: tests/test_protein_refill_host.py pins ``data.protein_slot_ids`` / ``data.dti_refill_tables`` to this, and
tests/test_gpu_protein_refill.py takes its slots and keys from here."""


def slots_and_keys(second_of_pairs, ns, slots):
    """``(slot ids, keys, U)``: the sorted distinct proteins ``u`` of the pairs, then the smallest proteins by ``(ns, id)`` that are not in
    ``u`` until ``slots`` are taken; ``keys[i]`` = the position of pair ``i``'s protein in ``u``.  ``ValueError`` for ``U > slots``."""
    second = [int(s) for s in second_of_pairs]
    u = sorted(set(second))
    if len(u) > slots:
        raise ValueError(f"{len(u)} distinct proteins, {slots} slots")
    by_size = sorted(range(len(ns)), key=lambda i: (int(ns[i]), i))
    fill = [i for i in by_size if i not in u][:slots - len(u)]
    return u + fill, [u.index(s) for s in second], len(u)


def offsets(ids, counts):
    """The exclusive offsets of the slots' rows, closed by their total."""
    out, run = [0], 0
    for i in ids:
        run += int(counts[i])
        out.append(run)
    return out


def refill_table(pair_ids, first, second, lig_ns, lig_es, pro_ns, pro_es, slots, phantoms):
    """The int table of one load: ligand ids (one entry of padding) and their node / edge / y offsets, the pair ids, the protein slot ids
    (one entry of padding) and their node / edge / y offsets, the ``B`` keys, ``phantoms`` zeros."""
    pair_ids = [int(i) for i in pair_ids]
    B = len(pair_ids)
    lig = [int(first[i]) for i in pair_ids]
    slot_ids, keys, _U = slots_and_keys([second[i] for i in pair_ids], pro_ns, slots)
    table = lig + [0] + offsets(lig, lig_ns) + offsets(lig, lig_es) + [0] * (B + 1)
    table += pair_ids
    table += slot_ids + [0] + offsets(slot_ids, pro_ns) + offsets(slot_ids, pro_es) + [0] * (slots + 1)
    return table + keys + [0] * phantoms
