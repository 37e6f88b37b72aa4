"""The kernels' shared-divisor quotient (device_core.inc div_y / div3): y = RN(1/d) once,
then q0 = RN(n*y), q = RN(q0 - RN(d*q0 - n)*y) per numerator, claimed bit-identical to the IEEE
division n / d (Markstein's correction; the reference divides component by component, tuple.rs:95-98,
light.rs:60-61).  fma is emulated exactly with rational arithmetic (Fraction -> float rounds to
nearest, ties to even), so this checks the claim on the CPU for the magnitudes the renders use.

The area-light path's integer quotient (render_levels.inc small_div: an f32 estimate and two integer corrections) is
restated in numpy float32 and tried over the whole domain of its two call sites, every level up to 1024."""
import math
import random
from fractions import Fraction as F

import numpy as np
import pytest


def fma(a, b, c):
    if a == 0.0 or b == 0.0:  # signed-zero semantics of a*b + c with an exact zero product
        return (a * b) + c
    r = F(a) * F(b) + F(c)
    if r == 0:
        return 0.0  # exact zero sum of non-zero terms is +0 in round-to-nearest
    return float(r)


def div_y(n, d, y):
    q0 = n * y
    return fma(-fma(d, q0, -n), y, q0)


def same(a, b):
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)


@pytest.mark.parametrize("seed", range(4))
def test_div_y_matches_ieee_division(seed):
    rnd = random.Random(seed)
    for _ in range(6000):
        d = math.ldexp(rnd.random() + 0.5, rnd.randint(-40, 40))  # positive divisors (norms, distances)
        n = math.ldexp(rnd.random() * 2.0 - 1.0, rnd.randint(-45, 45))
        y = 1.0 / d
        assert same(div_y(n, d, y), n / d), (n, d)


def test_div_y_signed_zeros_and_unit_vectors():
    rnd = random.Random(7)
    for n in (0.0, -0.0):
        for d in (1.0, 3.0, 0.1, 1e30):
            assert same(div_y(n, d, 1.0 / d), n / d)
    for _ in range(4000):  # normalize(v): every component over |v|
        v = [rnd.uniform(-10, 10) for _ in range(3)]
        m = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        y = 1.0 / m
        for c in v:
            assert same(div_y(c, m, y), c / m)


def test_area_cell_offsets():
    """(col + u) / level for every level up to RR_MAX_AREA_LEVEL (1024, rray.h), u with 32 random bits
    (jitter_value), including the extreme cells (col 0 with u = 0, col level-1 with u just below 1).
    Markstein's theorem covers every level (y = RN(1/level), q0 faithful, the residual exact in one fma);
    the samples check the implementation of it."""
    rnd = random.Random(11)
    for level in range(1, 1025):
        y = 1.0 / level
        cases = [(0, 0.0), (level - 1, (2**32 - 1) / 4294967296.0)]
        cases += [(rnd.randrange(level), rnd.getrandbits(32) * (1.0 / 4294967296.0))
                  for _ in range(40 if level <= 64 else 8)]
        for col, u in cases:
            n = col + u
            assert same(div_y(n, float(level), y), n / level), (level, col, u)


def small_div(n, d):
    """render_levels.inc small_div, statement by statement, on uint32 arrays n and a divisor d: rd = 1.0f / (float)d,
    q = (uint32)((float)n * rd) (conversions round to nearest even and truncate, as numpy's do), then the two
    corrections in wrapping 32-bit arithmetic."""
    n = np.asarray(n, np.uint32)
    d32 = np.uint32(d)
    rd = np.float32(1.0) / np.float32(d)
    q = (n.astype(np.float32) * rd).astype(np.uint32)
    q = np.where(q * d32 > n, q - np.uint32(1), q)
    q = np.where((q + np.uint32(1)) * d32 <= n, q + np.uint32(1), q)
    return q


def test_small_div_pairs_over_events():
    """area_shadow_block's h = small_div(j, level^2): pair j of nh <= 256 events.  Every level 1..RR_MAX_AREA_LEVEL, n
    around every multiple h d, h <= 256 (-1, 0, +1, the middle, d - 1): 1.3 million cases up to n = 2^28 + 2^20, far past
    the 2^24 where (float)n stops being exact; the quotient stays at or below 256."""
    cases = 0
    h = np.arange(257, dtype=np.int64)
    for level in range(1, 1025):
        d = level * level
        n = np.concatenate([h * d - 1, h * d, h * d + 1, h * d + d // 2, h * d + d - 1])
        n = np.unique(n[n >= 0])
        bad = np.flatnonzero(small_div(n, d) != n // d)
        assert len(bad) == 0, (level, int(n[bad[0]]))
        cases += len(n)
    assert cases > 1_000_000


def test_small_div_rows_of_cells():
    """row = small_div(s, level) for the cell s < level^2: every s for levels up to 64, and above that s around every
    multiple of level (-1, 0, +1, the middle, level - 1)."""
    for level in range(1, 1025):
        if level <= 64:
            s = np.arange(level * level, dtype=np.int64)
        else:
            r = np.arange(level, dtype=np.int64) * level
            s = np.concatenate([r - 1, r, r + 1, r + level // 2, r + level - 1])
            s = np.unique(s[(s >= 0) & (s < level * level)])
        bad = np.flatnonzero(small_div(s, level) != s // level)
        assert len(bad) == 0, (level, int(s[bad[0]]))


def test_small_div_restatement_can_fail():
    """the restatement is no tautology: past its precondition (quotients of 2^22 and more) the f32 estimate is off by
    more than the two corrections mend"""
    n = np.arange(2**32 - 4096, 2**32 - 1, dtype=np.int64)
    assert (small_div(n, 3) != n // 3).any()
