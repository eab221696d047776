"""fp32 arithmetic for the numpy twins of the device chains: what numpy's float32 does not give exactly.

numpy rounds every float32 operation to nearest, as the device's __f*_rn intrinsics do, but it has no fused multiply-add.
fma32() is one, rounded once.  fma32_double_rounding() is what the twins used before: the sum taken in fp64 and rounded
again, which differs from the fused operation where the fp64 sum lands on an fp32 midpoint that the exact sum is not on
(tests/test_fp32_np.py constructs such triples).  ulp_steps() moves float32 values by whole ulps, for the envelopes the twins
put around the device's library calls.
"""
import numpy as np

F = np.float32


def fma32_double_rounding(a, b, c):
    """a b + c in fp64, then rounded to fp32: two roundings.  Kept for tests/test_fp32_np.py and the sensitivity test."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def fma32(a, b, c):
    """fma(a, b, c) on float32 arrays (broadcast), correctly rounded once.  The product of two fp32 is exact in fp64
    (48 bits); the sum with c is taken by a TwoSum, and where its error term is not zero and the fp64 sum's last mantissa
    bit is even the sum is stepped one fp64 ulp toward the error: round-to-odd.  A value rounded to odd at 53 bits rounds to
    nearest at 24 bits as the exact value does (53 >= 24 + 2).  Infinities and NaN pass through as IEEE has them."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        s = np.array(s, np.float64, ndmin=1)
        err = np.broadcast_to(err, s.shape)
        move = np.isfinite(err) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)   # (err is NaN where s is not finite)
        if move.any():
            s = np.where(move, np.nextafter(s, np.copysign(np.inf, err)), s)
        out = s.astype(F)
    return out.reshape(np.broadcast(a, b, c).shape)


def ulp_steps(x, k):
    """The float32 k ulps from x (k an integer, either sign), by the ordered integer view; NaN and infinities stay."""
    x = np.asarray(x, F)
    i = x.view(np.int32).astype(np.int64)
    o = np.where(i < 0, -(i & 0x7FFFFFFF), i) + int(k)                # monotone in x; +-0 share 0
    o = np.clip(o, -0x7F800000, 0x7F800000)
    back = np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F)
    return np.where(np.isfinite(x), back, x).astype(F)


def ulp_distance(x, y):
    """y - x in float32 ulps (int64), by the ordered integer view; meaningful where both are finite."""
    def key(v):
        i = np.asarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return key(y) - key(x)
