"""BN254 G1 in Python integers, and the scalar / point cases of the per-point multiplication and the SRS update tests
(tests/test_gpu_g1_mul.py, tests/test_gpu_srs_update.py, tests/test_srs_update_host.py).  No library of the project is
used here: coordinates cross as uint64 limbs in Montgomery form (x * 2^256 mod q), as the boundary defines them."""
import random

import numpy as np

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = 1 << 256
MASK64 = (1 << 64) - 1


def limbs(x: int, words: int = 4) -> list:
    return [(x >> (64 * i)) & MASK64 for i in range(words)]


def unlimbs(a) -> int:
    return sum(int(v) << (64 * i) for i, v in enumerate(a))


def fr_mont(x: int) -> np.ndarray:
    return np.array(limbs(x % R * MONT % R), np.uint64)


def fr_raw_limbs(x: int) -> np.ndarray:
    """x AS IT IS in the limbs (no reduction, no Montgomery factor): for non-canonical inputs"""
    return np.array(limbs(x), np.uint64)


def fq_mont(x: int) -> list:
    return limbs(x % Q * MONT % Q)


def fq_unmont(a) -> int:
    return unlimbs(a) * pow(MONT, -1, Q) % Q


def affine_to_np(p) -> np.ndarray:
    """(x, y) or None (identity -> (0,0))"""
    if p is None:
        return np.zeros(8, np.uint64)
    return np.array(fq_mont(p[0]) + fq_mont(p[1]), np.uint64)


def np_to_affine(a):
    a = np.asarray(a).reshape(8)
    if not a.any():
        return None
    return fq_unmont(a[:4]), fq_unmont(a[4:])


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % Q == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, Q) % Q
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, Q) % Q
    x = (lam * lam - p[0] - q[0]) % Q
    return x, (lam * (p[0] - x) - p[1]) % Q


def neg(p):
    return None if p is None else (p[0], (Q - p[1]) % Q)


# Jacobian inside the ladder (one inversion per product instead of one per step)
def _jdbl(p):
    x, y, z = p
    if z == 0:
        return p
    a = x * x % Q
    b = y * y % Q
    c = b * b % Q
    d = 2 * ((x + b) * (x + b) - a - c) % Q
    e = 3 * a % Q
    x3 = (e * e - 2 * d) % Q
    return x3, (e * (d - x3) - 8 * c) % Q, 2 * y * z % Q


def _jadd_affine(p, q):
    x1, y1, z1 = p
    if z1 == 0:
        return q[0], q[1], 1
    z2 = z1 * z1 % Q
    u2 = q[0] * z2 % Q
    s2 = q[1] * z1 * z2 % Q
    if u2 == x1:
        if s2 == y1:
            return _jdbl(p)
        return 0, 1, 0
    h = (u2 - x1) % Q
    r = (s2 - y1) % Q
    h2 = h * h % Q
    h3 = h * h2 % Q
    v = x1 * h2 % Q
    x3 = (r * r - h3 - 2 * v) % Q
    return x3, (r * (v - x3) - y1 * h3) % Q, z1 * h % Q


def mul(p, k: int):
    """k * p, p = (x, y) or None"""
    k %= R
    if p is None or k == 0:
        return None
    acc = (0, 1, 0)
    for bit in bin(k)[2:]:
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd_affine(acc, p)
    if acc[2] == 0:
        return None
    zi = pow(acc[2], -1, Q)
    return acc[0] * zi * zi % Q, acc[1] * zi * zi * zi % Q


G = (1, 2)


def mul_each_ref(points, scalars) -> np.ndarray:
    """points: list of (x, y) / None, scalars: list of ints -> uint64[n, 8]"""
    out = np.zeros((len(points), 8), np.uint64)
    for i, (p, k) in enumerate(zip(points, scalars)):
        out[i] = affine_to_np(mul(p, k))
    return out


def points_np(points) -> np.ndarray:
    return np.array([affine_to_np(p) for p in points], np.uint64).reshape(-1, 8)


def scalars_np(scalars) -> np.ndarray:
    return np.array([fr_mont(k) for k in scalars], np.uint64).reshape(-1, 4)


def digits(s: int, w: int):
    """the recoding of csrc/g1_mul_digits.h restated: (windows, top, [d_(windows-1) .. d_0]), s = top 2^(w windows) + sum d_j 2^(w j)"""
    windows = (255 + w - 1) // w
    half = 1 << (w - 1)
    t = s + sum(half << (w * j) for j in range(windows))
    assert t < 1 << 256
    ds = [((t >> (w * j)) & ((1 << w) - 1)) - half for j in range(windows)]
    return windows, t >> (w * windows), ds[::-1]


def edge_scalars(w: int) -> list:
    """what the issue lists: 0 .. 2^w + 1, r - j for j = 1 .. 2^w + 1, 2^253, (r -+ 1)/2, the all-maximum-digit and
    all-minimum-digit patterns of the recoding (as far up as they stay below r), and seeded random values"""
    half = 1 << (w - 1)
    out = list(range(0, (1 << w) + 2)) + [R - j for j in range(1, (1 << w) + 2)]
    out += [1 << 253, (R - 1) // 2, (R + 1) // 2]
    windows = (255 + w - 1) // w
    for d in (half - 1, -half):
        # digit d in the windows 0 .. m-1, then (d < 0) a one above them so that the value is positive
        m = windows
        while True:
            v = sum(d << (w * j) for j in range(m)) + ((1 << (w * m)) if d < 0 else 0)
            if 0 < v < R:
                break
            m -= 1
        _, top, ds = digits(v, w)
        assert ds[len(ds) - m:] == [d] * m and m >= windows - 3, (w, d, m)
        out.append(v)
    rng = random.Random(15)
    out += [rng.randrange(R) for _ in range(24)]
    return out
