"""The three scans of csrc/poly.hip restated on Python integers: the running product of the permutation and lookup
arguments, the evaluation of a polynomial and the division by X - z of the GWC openings.  Nothing of the library or of
the oracle is used: values are canonical integers in [0, r), the converters below go to and from the library's
uint64[n, 4] arrays (little-endian limbs of value * 2^256 mod r).

tests/test_poly_ref_host.py holds the oracle's three functions against this file, so that the oracle can judge the sizes
at which Python integers are too slow."""
import functools

import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
_MONT = (1 << 256) % R
_MONT_INV = pow(_MONT, -1, R)


# ---- the operations
@functools.lru_cache(maxsize=1 << 17)
def _inv(d: int) -> int:
    """(remembered: the cases of one test share their denominators)"""
    return pow(d, -1, R)


def grand_product(num, den, z0):
    """z[0] = z0, z[i+1] = z[i] * num[i] / den[i], n values; a zero denominator makes its ratio 0 (halo2's BatchInvert
    leaves zeros alone).  num[n-1] and den[n-1] are not used."""
    z = [z0 % R]
    for i in range(len(num) - 1):
        ratio = num[i] * _inv(den[i] % R) % R if den[i] % R else 0
        z.append(z[-1] * ratio % R)
    return z


def eval_poly(a, x):
    """a[0] + a[1] x + ... by Horner's rule"""
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % R
    return acc


def kate_division(a, z):
    """The quotient of a(X) by X - z, n values: q[n-1] = 0, q[i] = a[i+1] + z q[i+1] (the remainder a(z) is dropped)."""
    n = len(a)
    q = [0] * n
    for i in range(n - 2, -1, -1):
        q[i] = (a[i + 1] + z * q[i + 1]) % R
    return q


# ---- converters
def _rows(a) -> list:
    """the stored integers of a uint64[n, 4] (or [4]) array"""
    a = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4)
    raw = a.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(a.shape[0])]


def _array(stored) -> np.ndarray:
    raw = b"".join(v.to_bytes(32, "little") for v in stored)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def to_ints(a) -> list:
    """Montgomery array -> canonical integers"""
    return [v * _MONT_INV % R for v in _rows(a)]


def to_int(a) -> int:
    return to_ints(a)[0]


def from_ints(vals) -> np.ndarray:
    """canonical integers -> Montgomery array uint64[n, 4]"""
    return _array([v % R * _MONT % R for v in vals])


def from_int(v: int) -> np.ndarray:
    return from_ints([v])[0]


def stored(vals) -> np.ndarray:
    """uint64[n, 4] whose STORED limbs are the given integers (each below r): stored(r - 1) is the largest bit pattern a
    kernel can meet, the element -(2^-256)."""
    assert all(0 <= v < R for v in vals)
    return _array(vals)


# ---- case families, shared by the host and the GPU tests (Montgomery arrays; `fill(seed, n)` draws n random elements)
def strip_rows(n: int, lane: int = 341):
    """(first, last) row of lane `lane`'s strip in the 1024-lane forms: a strip is ceil(n / 1024) rows"""
    strip = (n + 1023) // 1024
    first = lane * strip
    assert first + strip <= n
    return first, first + strip - 1


def zero_places(n: int) -> list:
    """the rows at which the single-zero grand-product cases put their zero (n > 1024)"""
    return sorted({0, 1, 255, 256, *strip_rows(n), n - 2, n - 1})


def gp_zero_free(fill, n: int, all_families: bool):
    """-> {name: (num, den, z0)} without a zero anywhere"""
    num, den, z0 = fill(1, n), fill(2, n), fill(3, 1)[0]
    out = {"random": (num, den, z0)}
    if all_families:
        top = stored([R - 1])
        out["stored r - 1 everywhere"] = (np.tile(top, (n, 1)), np.tile(top, (n, 1)), top[0])
        out["z0 = 1"] = (num, den, from_int(1))
    return out


def gp_degenerate(fill, n: int):
    """-> {name: (num, den, z0, rows that are not zero)}: two zeros in one block or strip, every denominator zero, z0 = 0"""
    num, den, z0 = fill(1, n), fill(2, n), fill(3, 1)[0]
    out = {}
    pairs = {"block": (1, min(200, n - 1))}
    if n > 1024:
        pairs["strip"] = strip_rows(n)
        pairs["block 1"] = (256, 300)
    for where, (t1, t2) in pairs.items():
        if not t1 < t2 < n - 1:
            continue
        d = den.copy()
        d[t1] = d[t2] = 0
        out["two zero denominators in one %s" % where] = (num, d, z0, t1 + 1)
        m, d = num.copy(), den.copy()
        m[t2] = d[t1] = 0
        out["a zero denominator, then a zero numerator in one %s" % where] = (m, d, z0, t1 + 1)
        m, d = num.copy(), den.copy()
        m[t1] = d[t2] = 0
        out["a zero numerator, then a zero denominator in one %s" % where] = (m, d, z0, t1 + 1)
    out["every denominator zero"] = (num, np.zeros_like(den), z0, 1)
    out["z0 = 0"] = (num, den, from_int(0), 0)
    return out


def polynomials(fill, n: int):
    """-> {name: coefficients}"""
    out = {"random": fill(10, n), "stored r - 1 everywhere": np.tile(stored([R - 1]), (n, 1)), "zero": np.zeros((n, 4), np.uint64)}
    one = from_int(1)
    out["a lone 1 at coefficient n - 1"] = np.zeros((n, 4), np.uint64)
    out["a lone 1 at coefficient n - 1"][n - 1] = one
    out["a lone 1 at coefficient 0"] = np.zeros((n, 4), np.uint64)
    out["a lone 1 at coefficient 0"][0] = one
    out["the upper half zero"] = fill(11, n)
    out["the upper half zero"][(n + 1) // 2:] = 0
    out["only the constant term"] = np.zeros((n, 4), np.uint64)
    out["only the constant term"][0] = fill(12, 1)[0]
    return out


def points(fill, n: int, omega=None):
    """-> {name: point}; omega: the domain's generator where n is a power of two"""
    out = {"0": from_int(0), "1": from_int(1), "r - 1": from_int(R - 1), "stored r - 1": stored([R - 1])[0], "2": from_int(2),
           "random": fill(99, 1)[0]}
    if omega is not None:
        out["omega"] = np.asarray(omega, np.uint64)
    return out
