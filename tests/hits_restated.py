"""The hit lists' total order and the expected lists after a stream of updates, restated with ``numpy.lexsort`` (a helper, not a test
module): better score first (larger with ``largest``, smaller without; ``-0.0 == +0.0``), equal scores by ascending id, NaN scores after
every number (among themselves by ascending id).  Selection involves no rounding: everything compared against this is compared bit for
bit (``bits`` / ``same``)."""
import numpy as np

NAN_BITS = 0x7FC00000          # an unfilled slot's score


def order(scores, ids, largest):
    """The permutation that sorts the candidates best first."""
    scores, ids = np.asarray(scores, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    nan = np.isnan(scores)
    s = np.where(nan, np.float32(0), scores)
    return np.lexsort((ids, -s if largest else s, nan))


def top(updates, k, largest):
    """``updates``: a list of ``(scores [L, Qs] float32, ids [L] or None)`` in stream order -> ``(scores [Qs, k] float32, ids [Qs, k]
    int32, counts [Qs] int64)`` after all of them; ``None`` ids are positions in the stream.  Padded with NaN / -1."""
    offered, all_s, all_i = 0, [], []
    for s, i in updates:
        s = np.asarray(s, dtype=np.float32)
        all_s.append(s)
        all_i.append(np.arange(offered, offered + s.shape[0], dtype=np.int64) if i is None else np.asarray(i, dtype=np.int64))
        offered += s.shape[0]
    s, i = np.concatenate(all_s, 0), np.concatenate(all_i)
    Qs = s.shape[1]
    out_s = np.full((Qs, k), NAN_BITS, dtype=np.uint32).view(np.float32)
    out_i = np.full((Qs, k), -1, dtype=np.int32)
    for j in range(Qs):
        best = order(s[:, j], i, largest)[:k]
        out_s[j, :best.size], out_i[j, :best.size] = s[best, j], i[best]
    return out_s, out_i, np.full(Qs, min(k, s.shape[0]), dtype=np.int64)


def bits(a):
    """float32 (numpy array or tensor) -> its uint32 image, for exact comparison (NaN == NaN, -0.0 != +0.0)."""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, expected):
    """Whether ``got`` — ``HitList.result()``, device tensors — is ``expected`` — ``top()`` — bit for bit."""
    (gs, gi, gc), (es, ei, ec) = got, expected
    return (np.array_equal(bits(gs), bits(es)) and np.array_equal(gi.cpu().numpy(), ei) and gi.cpu().numpy().dtype == np.int32
            and np.array_equal(gc.cpu().numpy(), ec))


def special_scores(n, rng):
    """``n`` float32 scores drawn from +-0, +-inf, NaN (quiet, negative, with a payload), denormals and a few normals — many ties."""
    pool = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC01234, 0x00000001, 0x80000001,
                     0x007FFFFF, 0x807FFFFF, 0x3F800000, 0xBF800000, 0x3F800001, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32)
    return pool[rng.integers(0, pool.size, n)].view(np.float32)
