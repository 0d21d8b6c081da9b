"""The host twin of the device stream (tests/philox_twin.py) against published answers, exact fractions and the statistics the training
noise must have.  tests/test_gpu_training_noise.py pins the device to this twin bit for bit, so what is shown here carries over."""
from fractions import Fraction

import numpy as np
import pytest

from tests import philox_twin as pt

# Known answers of Philox4x32-10 (the Random123 distribution's known-answer file): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = pt.philox4x32_10(*ctr, *key)
    assert tuple(int(g[0]) for g in got) == want


def test_philox_is_vectorised_over_the_counter():
    c = np.array([0, 0xFFFFFFFF, 0x243F6A88], dtype=np.uint64)
    got = pt.philox4x32_10(c, [0, 0xFFFFFFFF, 0x85A308D3], [0, 0xFFFFFFFF, 0x13198A2E], [0, 0xFFFFFFFF, 0x03707344], 0, 0)
    assert tuple(int(g[0]) for g in got) == KAT[0][2]
    assert all(g.dtype == np.uint32 and g.shape == (3,) for g in got)


def test_words_follow_the_element_rule():
    """Element i draws word i % 4 of philox4(i / 4); counter = (q lo, q hi, offset lo, offset hi), key = (seed lo, seed hi)."""
    seed, off = 0x9E3779B97F4A7C15, 2 ** 32 + 5
    w = pt.words(seed, off, 23)
    assert w.dtype == np.uint32 and w.shape == (23,)
    for i in (0, 1, 5, 22):
        v = pt.philox4x32_10(i // 4, 0, off & 0xFFFFFFFF, off >> 32, seed & 0xFFFFFFFF, seed >> 32)
        assert int(w[i]) == int(v[i % 4][0])
    assert np.array_equal(pt.words(seed, off, 8), w[:8]) and pt.words(seed, off, 0).shape == (0,)
    # both halves of the offset and of the seed reach the words
    for s2, o2 in ((seed, 5), (seed, off + 1), (seed & 0xFFFFFFFF, off), (seed ^ 1, off)):
        assert (pt.words(s2, o2, 64) != pt.words(seed, off, 64)).mean() > 0.9
    # the known answers through `words`: counter (0, 0, 0, 0) is quad 0 of offset 0 under seed 0
    assert tuple(int(x) for x in pt.words(0, 0, 4)) == KAT[0][2]
    assert tuple(int(x) for x in pt.words(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 4)) != KAT[1][2]      # (quad 0, not quad 2^64 - 1)


def _nearest_f32(fr):
    """An exact fraction rounded to nearest-even fp32 by search among the neighbours of its fp64 image."""
    c = np.float32(float(fr))
    cand = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    dist = [abs(Fraction(float(x)) - fr) for x in cand]
    best = min(dist)
    win = [x for x, d in zip(cand, dist) if d == best]
    if len(win) > 1:                                     # a tie: the even mantissa
        win = [x for x in win if (int(np.float32(x).view(np.uint32)) & 1) == 0]
    return np.float32(win[0])


@pytest.mark.parametrize("lo,hi", [(1 / 8, 1 / 3), (0.01, 0.7), (0.3, 0.3)])
def test_slope_table_equals_the_exact_fraction(lo, hi):
    """fmaf(hi - lo, h / 65536, lo) with fp32 operands, rounded once, on all 65 536 high halves."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    d = Fraction(float(np.float32(hi32 - lo32)))
    want = np.array([_nearest_f32(d * h / 65536 + Fraction(float(lo32))) for h in range(65536)], dtype=np.float32)
    got = pt.slope_table(lo, hi)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == lo32 and got.max() <= hi32 and np.all(np.diff(got) >= 0)
    w = np.array([0x0000FFFF, 0xFFFF0000, 0x80001234], dtype=np.uint32)
    assert np.array_equal(pt.slopes(w, lo, hi), got[[0, 65535, 0x8000]])


def test_keep_mask_threshold():
    lowhalf = np.arange(65536, dtype=np.uint32) | np.uint32(0xABCD0000)       # the high half never matters
    for p in (0.2, 0.5, 0.0):
        k = pt.keep_mask(lowhalf, p)
        want = np.array([Fraction(int(h), 65536) >= Fraction(float(np.float32(p))) for h in range(65536)])
        assert np.array_equal(k, want)
    assert pt.keep_mask(lowhalf, 0.0).all()
    # float32(0.2) = 0.2 + 2.98e-9 > 13107 / 65536 = 0.19999695: half 13107 is dropped, 13108 kept
    k = pt.keep_mask(lowhalf, 0.2)
    assert not k[13107] and k[13108] and k.sum() == 65536 - 13108
    # p = 0.5 is exact: the element AT the threshold is kept (>=)
    k = pt.keep_mask(lowhalf, 0.5)
    assert k[32768] and not k[32767] and k.sum() == 32768


def test_fp64_helpers():
    pre = np.array([-2.0, 0.0, 3.0, -1.0])
    sl = np.array([0.25, 0.25, 0.25, 0.5], dtype=np.float32)
    out = pt.rrelu(pre, pre, sl)
    assert out.dtype == np.float64 and np.array_equal(out, [-0.5, 0.0, 3.0, -0.5])
    d = pt.dropout(out, np.array([True, True, False, True]), 0.5)
    assert np.array_equal(d, [-1.0, 0.0, 0.0, -1.0])
    assert pt.drop_scale32(0.2).dtype == np.float32 and pt.drop_scale32(0.0) == 1.0


def _corr(a, b):
    return float(np.corrcoef(np.stack([a, b]))[0, 1])


def test_noise_statistics_of_the_twin():
    """What test_rrelu_and_dropout_device_stream_statistics asks of the device (tests/test_gpu_parity.py), asked of the twin, with that
    test's bounds: n = 2^20 slopes ~ U(lo, hi) have sigma(mean) = 0.06 / 1024 = 6e-5 (bound 3e-4), chi^2 over 16 bins has 15 degrees of
    freedom (P(chi^2 > 50) ~ 1e-5), correlations of independent samples have sigma 1 / 1024 (bound 5e-3), and the keep rate has
    sigma <= 0.5 / 1024 (bound 2e-3)."""
    n, lo, hi = 1 << 20, 1 / 8, 1 / 3
    w = pt.words(1234, 0, n)
    a = pt.slopes(w, lo, hi).astype(np.float64)
    assert a.min() >= lo and a.max() <= hi
    assert abs(a.mean() - (lo + hi) / 2) < 3e-4
    assert abs(a.var(ddof=1) - (hi - lo) ** 2 / 12) < 3e-5
    hist = np.histogram(a, bins=16, range=(lo, hi))[0]
    assert ((hist - n / 16) ** 2 / (n / 16)).sum() < 50
    assert abs(_corr(a[:-1], a[1:])) < 5e-3                               # neighbours are independent
    for p in (0.2, 0.5):
        assert abs(pt.keep_mask(w, p).mean() - (1 - p)) < 2e-3
    # the two halves of one word: the slope says nothing about the mask
    low = (w & np.uint32(0xFFFF)).astype(np.float64)
    assert abs(_corr(a, low)) < 5e-3
    assert abs(_corr(a, pt.keep_mask(w, 0.2).astype(np.float64))) < 5e-3
    # consecutive launches (offsets o and o + 1) draw independent numbers
    w1 = pt.words(1234, 1, n)
    a1 = pt.slopes(w1, lo, hi).astype(np.float64)
    assert (w1 != w).mean() > 0.99
    assert abs(_corr(a, a1)) < 5e-3
    assert abs(_corr(low, (w1 & np.uint32(0xFFFF)).astype(np.float64))) < 5e-3
    k0, k1 = pt.keep_mask(w, 0.2), pt.keep_mask(w1, 0.2)
    assert abs((k0 & k1).mean() - 0.64) < 2e-3                            # P(both keep) = 0.8^2
