"""A host twin of the device-side random stream (glam_amd/csrc/rng.h) and of the noise the training-mode kernels draw from it.

The stream is the public Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written here from
the published algorithm: ten rounds of

    (c0, c1, c2, c3) <- (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0)),    M0 = D2511F53, M1 = CD9E8D57

with the key bumped by (9E3779B9, BB67AE85) after every round.  Key = the 64-bit seed, counter = (element-quad index, launch offset).

ONE rule holds in every kernel: element ``i`` of the tensor as stored (flat index, padded width) draws word ``i % 4`` of ``philox4(i / 4)``,
whatever thread computes it.  The RReLU slope comes from the word's high 16 bits, the Dropout decision from its low 16 bits; every forward
records the ``(seed, offset)`` it used in ``eff`` and leaves ``offset + 1`` behind.  So the host regenerates, bit for bit, the slope and the
mask of every element of every launch, and a training-mode operation becomes an ordinary deterministic function with an fp64 reference.

numpy only; no device.  ``slopes`` is bit-exact to the kernels' ``fmaf(hi - lo, (w >> 16) / 65536, lo)``: its 65 536-entry table is built
in integer arithmetic and rounded ONCE to fp32 (an fma rounds once; the difference ``hi - lo`` is the fp32 one).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counter ``(c0, c1, c2, c3)`` under the key ``(k0, k1)``: four uint32 arrays (vectorised over the counter)."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _MASK32 for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(seed, offset, n):
    """uint32[n]: the word of flat element ``i`` of a launch that recorded ``eff == (seed, offset)``."""
    seed, offset, n = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(n)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    v = philox4x32_10(q & _MASK32, q >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(v, axis=1).reshape(-1)[:n]


def keep_mask(w, p):
    """bool: the elements Dropout(p) keeps — ``(w & 0xffff) / 65536 >= float32(p)``, exact (both sides are exact in fp64)."""
    return (np.asarray(w, dtype=np.uint32) & np.uint32(0xFFFF)).astype(np.float64) / 65536.0 >= np.float64(np.float32(p))


def _dyadic(x):
    """``(m, e)`` with ``x == m * 2**e`` exactly for a finite float."""
    num, den = float(x).as_integer_ratio()
    return num, -(den.bit_length() - 1)


def _round_f32(m, e):
    """``m * 2**e`` (m >= 0 an int) rounded once, to nearest even, to fp32."""
    if m == 0:
        return np.float32(0.0)
    top = m.bit_length() - 1 + e                        # 2^top <= value < 2^(top + 1)
    q = max(top, -126) - 23                             # the quantum of fp32 at this magnitude (subnormals: 2^-149)
    sh = q - e
    if sh <= 0:
        n = m << -sh
    else:
        n, rem, half = m >> sh, m & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and (n & 1)):
            n += 1
    return np.float32(np.ldexp(float(n), q))            # n <= 2^24: exact


_TABLES: dict = {}


def slope_table(lo, hi):
    """fp32[65536]: ``fmaf(hi - lo, h / 65536, lo)`` for every high half ``h``, all operands fp32, each entry rounded once."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    key = (lo32.tobytes(), hi32.tobytes())
    if key not in _TABLES:
        d32 = np.float32(hi32 - lo32)                    # one IEEE fp32 subtraction, as the kernel's
        assert d32 >= 0 and lo32 > 0, "RReLU needs 0 < lower <= upper"
        dm, de = _dyadic(d32)
        lm, le = _dyadic(lo32)
        e = min(de - 16, le)
        a, b = dm << (de - 16 - e), lm << (le - e)
        _TABLES[key] = np.array([_round_f32(a * h + b, e) for h in range(65536)], dtype=np.float32)
    return _TABLES[key]


def slopes(w, lo, hi):
    """fp32: the RReLU slope of every word, bit-exact to the device's."""
    return slope_table(lo, hi)[np.asarray(w, dtype=np.uint32) >> np.uint32(16)]


def drop_scale32(p):
    """The fp32 factor the kernels multiply kept elements by: ``1.f / (1.f - p)``."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def rrelu(pre, sign_from, slope):
    """fp64 RReLU under known noise: ``pre`` where ``sign_from > 0``, else ``pre * slope`` (at 0 the slope side: torch's convention)."""
    pre = np.asarray(pre, dtype=np.float64)
    return np.where(np.asarray(sign_from) > 0, pre, pre * np.asarray(slope, dtype=np.float64))


def dropout(v, mask, p):
    """fp64 Dropout under a known mask: ``v / (1 - p)`` where kept, 0 elsewhere (p as the fp32 value the kernel receives)."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(mask, v / (1.0 - np.float64(np.float32(p))), 0.0)
