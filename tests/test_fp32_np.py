"""fp32_np.fma32 against exact rational arithmetic rounded to fp32 once, on random triples and on constructed ties."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_np as fp  # noqa: E402

F = np.float32


def _round32(x):
    """The float32 nearest the Fraction x, ties to even; +-inf past the largest finite."""
    if x == 0:
        return F(0.0)
    sign, x = (-1.0 if x < 0 else 1.0), abs(x)
    e = max(x.numerator.bit_length() - x.denominator.bit_length() - 24, -149)   # 2^23 <= x / 2^e < 2^24 within one step
    while x / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while e > -149 and x / Fraction(2) ** e < 2 ** 23:
        e -= 1
    q = x / Fraction(2) ** e
    m = q.numerator // q.denominator
    rem = q - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    if m * Fraction(2) ** e >= Fraction(2) ** 128:
        return F(sign * np.inf)
    return F(sign * float(m) * 2.0 ** e) if e >= -126 else F(sign * np.ldexp(float(m), e))


def _exact(a, b, c):
    return np.array([_round32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F)


def _same(x, y):
    return np.array_equal(np.asarray(x, F).view(np.uint32), np.asarray(y, F).view(np.uint32))


def test_round32_is_numpys_on_doubles():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(2000) * 10.0 ** rng.uniform(-44, 38, 2000)
    assert _same([_round32(Fraction(float(x))) for x in v], v.astype(F))


def test_random_triples():
    rng = np.random.default_rng(1)
    n = 4000
    a, b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n) for _ in range(2))
    a, b = a.astype(F), b.astype(F)
    # a third with c near -a b (cancellation), a third far smaller than a b (a sticky tail), a third unrelated
    ab = a.astype(np.float64) * b.astype(np.float64)
    c = np.where(np.arange(n) % 3 == 0, -ab * (1.0 + rng.uniform(-1e-6, 1e-6, n)),
                 np.where(np.arange(n) % 3 == 1, ab * 2.0 ** rng.uniform(-70, -20, n), rng.standard_normal(n))).astype(F)
    assert _same(fp.fma32(a, b, c), _exact(a, b, c))


def _ties(rng, n):
    """a b an odd integer in [2^24, 2^25), scaled by a power of two: exactly an fp32 midpoint.  c: a tail far below the
    fp64 sum's last bit, of either sign, or zero."""
    A = (rng.integers(2 ** 24 // 3 + 1, 2 ** 25 // 3, n) | 1).astype(np.int64)
    assert np.all((3 * A >= 2 ** 24) & (3 * A < 2 ** 25) & (3 * A % 2 == 1))
    sa, sc = 2.0 ** rng.integers(-30, 30, n), 2.0 ** rng.integers(-70, -36, n)
    a = (A * sa).astype(F)
    b = np.full(n, 3.0, F) * np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(F)
    c = (np.abs(a.astype(np.float64)) * sc * rng.choice([-1.0, 0.0, 1.0], n)).astype(F)
    return a, b, c


def test_constructed_ties():
    a, b, c = _ties(np.random.default_rng(2), 3000)
    want = _exact(a, b, c)
    assert _same(fp.fma32(a, b, c), want)
    old = fp.fma32_double_rounding(a, b, c)
    wrong = old.view(np.uint32) != want.view(np.uint32)
    print(f"ties: the double rounding is wrong on {wrong.sum()} of {len(a)}")
    assert wrong.sum() > 500 and np.all(c[wrong] != 0.0)
    # one by hand: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24, the midpoint above 1 + 2^-11; 2^-80 more decides it upward
    x = F(1.0 + 2.0 ** -12)
    got, twice = fp.fma32(x, x, F(2.0 ** -80)), fp.fma32_double_rounding(x, x, F(2.0 ** -80))
    assert float(got) == 1.0 + 2.0 ** -11 + 2.0 ** -23 and float(twice) == 1.0 + 2.0 ** -11
    assert float(fp.fma32(x, x, F(-2.0 ** -80))) == 1.0 + 2.0 ** -11 == float(fp.fma32(x, x, F(0.0)))


def test_specials_and_shapes():
    inf, nan = F(np.inf), F(np.nan)
    assert fp.fma32(inf, F(1.0), F(1.0)) == inf and fp.fma32(F(3e38), F(10.0), F(0.0)) == inf
    assert np.isnan(fp.fma32(inf, F(0.0), F(1.0))) and np.isnan(fp.fma32(inf, F(1.0), -inf)) and np.isnan(fp.fma32(nan, F(1.0), F(1.0)))
    assert fp.fma32(F(1e30), F(1e30), -inf) == -inf
    tiny = F(2.0 ** -149)
    assert fp.fma32(tiny, F(0.5), F(0.0)) == 0.0 and fp.fma32(tiny, F(0.75), F(0.0)) == tiny     # ties to even; above the tie
    assert fp.fma32(np.ones((3, 1), F), np.ones(4, F), F(1.0)).shape == (3, 4) and fp.fma32(F(1.0), F(1.0), F(1.0)).shape == ()


def test_ulp_steps():
    x = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -149, 3.4028235e38, np.inf, np.nan], F)
    up, down = fp.ulp_steps(x, 1), fp.ulp_steps(x, -1)
    assert float(up[2]) == 1.0 + 2.0 ** -23 and float(down[2]) == 1.0 - 2.0 ** -24 and float(up[3]) == -(1.0 - 2.0 ** -24)
    assert float(up[0]) == 2.0 ** -149 == float(up[1]) and float(down[4]) == 0.0 and float(down[0]) == -2.0 ** -149
    assert np.isinf(up[5]) and np.isinf(up[6]) and np.isnan(up[7])
    v = np.random.default_rng(3).standard_normal(1000).astype(F)
    for k in (-6, -1, 0, 1, 6):
        assert np.array_equal(fp.ulp_distance(v, fp.ulp_steps(v, k)), np.full(1000, k))
