"""The judge of the field9 probe (tests/abi/field9_probe.hip): csrc/field9.h and the device path of csrc/field.h restated
in Python integers.  Nothing here comes from the library: the limb split, the value of a limb vector, what a Montgomery
reduction by 2^261 has to return, and the affine group law of BN254 G1 (y^2 = x^3 + 3).  Every check is exact.

A check returns None when the result is right and a one-line reason when it is not; tests/field9_cases.py adds the op, the
record and the operands to that line."""

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583  # base field of BN254 G1
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # scalar field
MODULI = (Q, R)  # the probe's field selector
W = 29
MASK = (1 << W) - 1
RADIX = 1 << (9 * W)  # 2^261, the Montgomery radix of the nine-limb form
SENTINEL = 0x5A5A5A5A  # what the probe fills its result records with: no limb of a valid result


def val(l):
    """sum l[i] 2^(29 i), limbs signed"""
    v = 0
    for x in reversed(l):
        v = (v << W) + x
    return v


def split(v):
    """the normalised limbs of v: l[0..7] in [0, 2^29), l[8] the signed rest"""
    l = [(v >> (W * i)) & MASK for i in range(8)]
    top = v >> (8 * W)
    assert -(1 << 31) <= top < (1 << 31), "top limb does not fit 32 bits"
    return l + [top]


def is_normalised(l):
    return all(0 <= x <= MASK for x in l[:8])


def val32(w):
    """8 x 32-bit words (given as signed or unsigned 32-bit integers), little endian"""
    return sum((x & 0xFFFFFFFF) << (32 * i) for i, x in enumerate(w))


def split32(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def mont(T, p):
    """What Field9::mul / mul2 / Dot9::reduce return for the exact integer T of their products: (T + m p) / 2^261 with the one
    m in [0, 2^261) that makes the division exact -- the integer in [T / 2^261, T / 2^261 + p) congruent to T 2^-261."""
    m = (-T * pow(p, -1, RADIX)) % RADIX
    assert (T + m * p) % RADIX == 0
    return (T + m * p) >> (9 * W)


def near(v, p):
    """v relative to the nearest multiple of p"""
    j = (v + p // 2) // p
    return "%d*p%+d" % (j, v - j * p)


def hexl(l):
    return "[" + " ".join(("-" if x < 0 else "") + "%x" % abs(x) for x in l) + "]"


def show(l, p):
    return "%s = %s" % (hexl(l), near(val(l), p))


# ---- BN254 G1, affine; None is the identity ----------------------------------------------------------------------------
G = (1, 2)


def on_curve(P):
    return P is None or (P[1] * P[1] - P[0] * P[0] * P[0] - 3) % Q == 0


def ec_neg(P):
    return None if P is None else (P[0], (-P[1]) % Q)


def ec_add(P, S):
    if P is None:
        return S
    if S is None:
        return P
    if P[0] == S[0]:
        if (P[1] + S[1]) % Q == 0:
            return None
        lam = 3 * P[0] * P[0] * pow(2 * P[1], -1, Q) % Q
    else:
        lam = (S[1] - P[1]) * pow(S[0] - P[0], -1, Q) % Q
    x = (lam * lam - P[0] - S[0]) % Q
    return (x, (lam * (P[0] - x) - P[1]) % Q)


def ec_mul(k, P):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, P)
        P = ec_add(P, P)
        k >>= 1
    return acc


# ---- checks ----------------------------------------------------------------------------------------------------------------
def check_limbs(got, want_value):
    """limb for limb the normalised split of want_value"""
    want = split(want_value)
    if list(got) != want:
        return "limbs %s, expected %s (value off by %d)" % (hexl(got), hexl(want), val(got) - want_value)
    return None


def check_mont(got, T, p):
    e = mont(T, p)
    err = check_limbs(got, e)
    if err:
        d = val(got) - e
        return err + (" = %d*p%+d" % (d // p, d % p) if d else " (same value, other limbs)")
    return None


def check_words(got, want_value):
    if val32(got) != want_value:
        return "words %064x, expected %064x" % (val32(got), want_value)
    return None


def affine_of(c):
    """the affine point of XYZZ coordinates given as integers in the 2^261 form (the radix cancels in x / zz and y / zzz);
    None for zz == 0 (mod q)"""
    x, y, zz, zzz = (v % Q for v in c)
    if zz == 0:
        return None
    return (x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q)


def check_point(c, want):
    """c: the four result coordinates as limb lists; want: the affine point, None for the identity (exactly all-zero limbs).
    A valid result is a valid operand of the next addition: every coordinate written, normalised and below 2^258."""
    names = ("x", "y", "zz", "zzz")
    for n, l in zip(names, c):
        if all(x == SENTINEL for x in l):
            return "%s was not written (sentinel)" % n
    if want is None:
        if any(x != 0 for l in c for x in l):
            return "expected the all-zero identity, got zz = %s" % hexl(c[2])
        return None
    for n, l in zip(names, c):
        if not is_normalised(l):
            return "%s = %s is not normalised" % (n, hexl(l))
        if abs(val(l)) >= 1 << 258:
            return "%s = %s is not below 2^258" % (n, hexl(l))
    v = [val(l) for l in c]
    rinv = pow(RADIX, -1, Q)
    zz, zzz = v[2] * rinv % Q, v[3] * rinv % Q
    if zz == 0 or zzz == 0:
        return "zz or zzz is 0 mod q for a point that is not the identity (zz = %s)" % show(c[2], Q)
    if (zz * zz * zz - zzz * zzz) % Q:
        return "zz^3 != zzz^2 (zz = %s, zzz = %s)" % (show(c[2], Q), show(c[3], Q))
    got = affine_of(v)
    if got != want:
        if got == ec_neg(want):
            return "the point is the NEGATIVE of the expected one (y negated)"
        return "point (%x, %x), expected (%x, %x)" % (got + want)
    return None
