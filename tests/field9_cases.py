"""Cases and judgement for the field9 probe (tests/abi/field9_probe.hip): the records of its IN file, built from the
contracts that csrc/field9.h and csrc/field.h state in their comments, and the verdict on its OUT file, from Python
integers (tests/field9_ref.py).  Before a case becomes a record its generator asserts that it lies INSIDE the contract of
the function it is for; the judge works from the raw operands of the record, not from what the generator meant.

Shared by tests/test_gpu_field9.py (the device) and tests/test_field9_host.py (the same plain-C++ functions on the host)."""
import functools
import random

import numpy as np

from field9_ref import (G, MASK, MODULI, Q, RADIX, affine_of, check_limbs, check_mont, check_point, check_words, ec_add,
                        ec_mul, ec_neg, hexl, is_normalised, near, show, split, split32, val, val32)

IN_WORDS, OUT_WORDS, OUT_SLOTS = 76, 112, 12
OP = dict(unpack=1, pack=2, norm=3, mul=4, sqr=5, mul2_add=6, mul2_sub=7, dot=8, canon=9, iszero=10, reduce_pack=11,
          mul_small=12, mul2_split=13, fe_mul=20, fe_sqr=21, fe_add=22, fe_sub=23, fe_neg=24, fe_dbl=25, fe_from_raw=26, fe_to_raw=27,
          madd=30, from_pair=31, dbl=32, add=33, to_xyzz=34, xaddl1=40, xaddl2=41, xaddl4=42, xadd1=43, xadd2=44, xadd4=45,
          xmadd_pair=50)
OP_NAME = {v: k for k, v in OP.items()}
HOST_OPS = {v for v in OP.values() if v < 40}  # plain C++: no DPP, no fences
LANES = {40: 1, 41: 2, 42: 4, 43: 1, 44: 2, 45: 4}
F9_SMALL_MAX = 1 << 12
B29, B30 = MASK, (1 << 30) - 1
TOP258 = (1 << 26) - 1  # with l[0..7] at 2^29 - 1 the value is 2^258 - 1
ZERO9 = [0] * 9


def fe_slot(v):
    return split32(v) + [0]


# ---- records ---------------------------------------------------------------------------------------------------------------
class Cases:
    """rows of (op, field, arg, eight slots)"""

    def __init__(self):
        self.rows = []

    def add(self, op, field, arg, slots):
        assert len(slots) <= 8 and all(len(s) == 9 for s in slots)
        self.rows.append((OP[op], field, arg, list(slots) + [ZERO9] * (8 - len(slots))))

    def add_groups(self, op, field, arg, groups):
        """groups of 8 / k slots each, packed k to a record; the last record is filled up by repeating its last group"""
        if not groups:
            return
        per = 8 // len(groups[0])
        for i in range(0, len(groups), per):
            chunk = list(groups[i:i + per])
            chunk += [chunk[-1]] * (per - len(chunk))
            self.add(op, field, arg, [s for g in chunk for s in g])

    def array(self):
        a = np.zeros((len(self.rows), IN_WORDS), dtype=np.int64)
        for i, (op, field, arg, slots) in enumerate(self.rows):
            a[i, 0], a[i, 1], a[i, 2] = op, field, arg
            a[i, 4:] = [x for s in slots for x in s]
        assert a.min() >= -(1 << 31) and a.max() < (1 << 32)
        return (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32)  # (words of the 8 x 32-bit ops wrap to negative)


def counts(rows):
    c = {}
    for op, field, _, _ in rows:
        k = "%s/%s" % (OP_NAME[op], "Fr" if field else "Fq")
        c[k] = c.get(k, 0) + 1
    return c


# ---- operands of the limb ops ------------------------------------------------------------------------------------------------
def rnd_norm(rng, lo, hi):
    return split(rng.randrange(lo, hi))


def denorm(l, rng):
    """another limb pattern of the same value, limb magnitudes <= 2^30 - 1"""
    o = list(l)
    for i in range(8):
        ks = [k for k in (-1, 0, 1) if abs(o[i] - (k << 29)) <= B30 and abs(o[i + 1] + k) <= B30]
        k = rng.choice(ks)
        o[i] -= k << 29
        o[i + 1] += k
    assert val(o) == val(l) and all(abs(x) <= B30 for x in o)
    return o


def bound_patterns():
    """every limb at the 2^29 bound, the top limb chosen so that the magnitude stays below 2^258"""
    pos = [B29] * 8 + [TOP258]
    alt = [B29 if i % 2 == 0 else -B29 for i in range(8)] + [TOP258]
    return [pos, [-x for x in pos], alt, [-x for x in alt]]


def special_limbs(p):
    return [split(v) for v in (0, 1, p - 1, p, 2 * p - 1, (1 << 256) - 1, RADIX % p)]


def in_mul_contract(a, b):
    """Field9::mul: limb magnitudes < 2^29, one operand may reach 2^30; values of magnitude < 2^258"""
    ma, mb = max(abs(x) for x in a), max(abs(x) for x in b)
    return (min(ma, mb) <= B29 and max(ma, mb) <= B30 and abs(val(a)) < 1 << 258 and abs(val(b)) < 1 << 258)


def dot_sum(s, n):
    """the probe's dot product of n terms: term t is pair t % 4 of the record"""
    T = sum(val(s[2 * t]) * val(s[2 * t + 1]) for t in range(4))
    return T * (n // 4) + sum(val(s[2 * t]) * val(s[2 * t + 1]) for t in range(n % 4))


def gen_limb_ops(c, rng):
    # f9_unpack / f9_pack: any 256-bit pattern
    pats = [0, (1 << 256) - 1]
    for i in range(1, 9):
        pats += [1 << b for b in (29 * i - 1, 29 * i, 29 * i + 1) if b < 256]
    for w in range(1, 8):
        pats += [1 << (32 * w - 1), 1 << (32 * w), (1 << (32 * w)) - 1, ((1 << 256) - 1) ^ ((1 << (32 * w)) - 1)]
    pats += [sum(0xFFFFFFFF << (64 * i) for i in range(4)), sum(0xFFFFFFFF << (64 * i + 32) for i in range(4))]
    pats += [sum(MASK << (58 * i) for i in range(5)) & ((1 << 256) - 1), sum(MASK << (58 * i + 29) for i in range(4))]
    pats += [rng.getrandbits(256) for _ in range(200)]
    for op in ("unpack", "pack"):
        c.add_groups(op, 0, 0, [[fe_slot(v)] for v in pats])
    # f9_norm: limbs up to +-(2^30 - 1), carry chains through all eight limbs in both directions
    ns = [[B30] * 9, [-B30] * 9, [B30 if i % 2 else -B30 for i in range(9)], [-B30 if i % 2 else B30 for i in range(9)],
          [1 << 29] + [B29] * 7 + [0], [B30] + [B29] * 7 + [-1], [-1] + [0] * 8, [-1] + [0] * 7 + [1],
          [-B30] + [0] * 7 + [5], [-(1 << 29)] + [-B29 - 1 + 1] * 7 + [0], [-1] + [-(1 << 29)] * 7 + [B30],
          [B29, 1] + [B29] * 6 + [-B30]]
    ns += [[rng.randint(-B30, B30) for _ in range(9)] for _ in range(300)]
    assert all(abs(x) <= B30 for l in ns for x in l)
    c.add_groups("norm", 0, 0, [[l] for l in ns])

    for f, p in enumerate(MODULI):
        lo, hi = -(1 << 256) + 1, (1 << 256) + p  # what a product returns
        S = special_limbs(p) + bound_patterns()
        diffs = []
        for _ in range(40):
            a, b = rnd_norm(rng, lo, hi), rnd_norm(rng, lo, hi)
            diffs.append([x - y for x, y in zip(a, b)])
        diffs.append([x - y for x, y in zip(split((1 << 256) + p - 1), split(lo))])
        diffs.append([x - y for x, y in zip([B29] * 8 + [0], [0] * 8 + [TOP258 // 2])])
        big = [[B30] * 8 + [TOP258 - 2], [-B30] * 8 + [-(TOP258 - 2)],
               [B30 if i % 2 == 0 else -B30 for i in range(8)] + [TOP258 - 2],
               [-B30 if i % 2 == 0 else B30 for i in range(8)] + [-(TOP258 - 2)]]
        rand = [rnd_norm(rng, lo, hi) for _ in range(600)]
        # mul
        pairs = [(a, b) for a in S for b in S]
        pairs += [(d, s) for d in diffs for s in (S[2], S[7], rand[0])] + [(diffs[i], diffs[-1 - i]) for i in range(20)]
        pairs += [(g, s) for g in big for s in S + diffs[:4]] + [(s, g) for g in big for s in S[:3]]
        pairs += [(rand[2 * i], rand[2 * i + 1]) for i in range(300)]
        assert all(in_mul_contract(a, b) for a, b in pairs)
        c.add_groups("mul", f, 0, [list(pr) for pr in pairs])
        # sqr: its one operand is both factors, so the doubled copy is the side that reaches 2^30 and the operand itself
        # stays below 2^29 (at 2^30 a column of the square alone passes 2^63)
        sq = S + diffs + rand[:300]
        assert all(in_mul_contract(a, a) and max(abs(x) for x in a) <= B29 for a in sq)
        c.add_groups("sqr", f, 0, [[a] for a in sq])
        # mul2: limb magnitudes < 2^29 on all four operands -- all NINE limbs at the bound fill a column to 27 * 2^58
        full, alt9 = [B29] * 9, [B29 if i % 2 == 0 else -B29 for i in range(9)]
        nf, na = [-x for x in full], [-x for x in alt9]
        P4 = S[7]
        quads = {False: [(full, full, full, full), (nf, nf, nf, nf), (nf, nf, full, full), (full, nf, full, nf), (nf, full, full, nf),
                         (alt9, alt9, alt9, alt9), (alt9, na, na, alt9), (P4, P4, P4, P4), (S[8], S[8], P4, P4)],
                 True: [(full, full, full, nf), (nf, nf, nf, full), (full, full, nf, full), (full, nf, full, full), (nf, full, nf, nf),
                        (alt9, alt9, alt9, na), (alt9, na, alt9, alt9), (P4, P4, P4, S[8]), (S[8], P4, P4, P4)]}
        for sub in (False, True):
            qs = list(quads[sub])
            T = S + diffs[:9]
            qs += [(T[i], T[(i + j) % len(T)], T[(i + 3 * j) % len(T)], T[(i + 5 * j + 1) % len(T)]) for i in range(len(T)) for j in (1, 2, 5)]
            qs += [(diffs[i], diffs[i + 1], diffs[i + 2], diffs[i + 3]) for i in range(0, 36, 2)]
            qs += [tuple(rand[(4 * i + k + (300 if sub else 0)) % 600] for k in range(4)) for i in range(300)]
            assert all(max(abs(x) for l in q for x in l) <= B29 for q in qs)
            c.add_groups("mul2_sub" if sub else "mul2_add", f, 0, [list(q) for q in qs])
            if sub:  # the same quadruples as two products reduced apart (mulq) and joined by sub_fused, as the lanes do;
                # mulq has the contract of mul, which also bounds the values: the nine-limb patterns at 2^29 are outside it
                sp = [q for q in qs if in_mul_contract(q[0], q[1]) and in_mul_contract(q[2], q[3])]
                assert len(sp) >= 300, len(sp)
                c.add_groups("mul2_split", f, 0, [list(q) for q in sp])
        # Dot9: unpacked canonical operands (limbs in [0, 2^29), below 2^256), at most 2^13 terms, the sum below 2^521
        maxc = split((1 << 256) - 1)
        pm1, z = split(p - 1), split(0)
        rc = [rnd_norm(rng, 0, p) for _ in range(64)]
        dots = [(3, [maxc] * 8), (6, [maxc] * 8), (4, [maxc] * 8)]
        for n in (1, 2, 3, 4, 5, 7, 8191, 8192):
            dots += [(n, [z] * 8), (n, [pm1] * 8), (n, rc[:8]), (n, [pm1, rc[8], z, rc[9], rc[10], pm1, pm1, pm1]), (n, rc[8:16])]
        dots += [(rng.randint(1, 64), [rng.choice(rc) for _ in range(8)]) for _ in range(200)]
        dots += [(rng.randint(1, 16), [split(rng.getrandbits(256)) for _ in range(8)]) for _ in range(100)]
        for n, sl in dots:
            assert 1 <= n <= 8192 and all(is_normalised(l) and 0 <= l[8] < 1 << 24 for l in sl)
            assert dot_sum(sl, n) < 1 << 521
            c.add("dot", f, n, sl)
        # canon: values in (-2p, 3p), normalised and not
        cv = [-2 * p + 1, -p, -1, 0, p - 1, p, 2 * p, 3 * p - 1, 1, p + 1, 2 * p - 1, -p + 1, -p - 1]
        cv += [rng.randrange(-2 * p + 1, 3 * p) for _ in range(200)]
        assert all(-2 * p < v < 3 * p for v in cv)
        cl = [split(v) for v in cv]
        cl += [denorm(l, rng) for l in cl] + [denorm(l, rng) for l in cl[:13]]
        c.add_groups("canon", f, 0, [[l] for l in cl])
        # is_zero_mod_p: normalised values in [0, 8p)
        zv = []
        for j in range(8):
            zv += [j * p + d for d in (-1, 0, 1) if j * p + d >= 0]
            zv += [j * p + d * (1 << (29 * i)) for i in range(1, 9) for d in (-1, 1) if j * p + d * (1 << (29 * i)) >= 0]
        zv += [8 * p - 1] + [rng.randrange(0, 8 * p) for _ in range(200)]
        assert all(0 <= v < 8 * p for v in zv) and len(zv) >= 8 * 19 - 9
        c.add_groups("iszero", f, 0, [[split(v)] for v in zv])
        # f9_reduce_pack: normalised, magnitude below 2^263
        K = (1 << 263) // p
        rv = [m * p + d for m in range(-K, K + 1) for d in (-1, 0, 1, p // 2) if abs(m * p + d) < 1 << 263]
        rv += [(1 << 263) - 1, -(1 << 263) + 1] + [rng.randrange(-(1 << 263) + 1, 1 << 263) for _ in range(200)]
        assert all(abs(v) < 1 << 263 for v in rv)
        c.add_groups("reduce_pack", f, 0, [[split(v)] for v in rv])
        # f9_mul_small: x normalised, |x| < 2^258, |c| <= F9_SMALL_MAX
        xs = [0, 1, -1, p - 1, p, 2 * p - 1, (1 << 256) + p - 1, -(1 << 256) + 1, (1 << 258) - 1, -(1 << 258) + 1]
        pool = [split(rng.randrange(-(1 << 258) + 1, 1 << 258)) for _ in range(96)]
        fixed = [split(v) for v in xs]
        assert all(abs(v) < 1 << 258 for v in xs)
        for k in range(-F9_SMALL_MAX, F9_SMALL_MAX + 1):
            c.add_groups("mul_small", f, k, [[l] for l in fixed + [pool[(6 * k + i) % 96] for i in range(6)]])
        for k in (1, 2, 3, 5, 7, 4095, 4096, -1, -4095, -4096):
            mmax = (abs(k) * ((1 << 258) - 1)) // p
            edge = []
            for t in range(81):
                m = -mmax + (2 * mmax * t) // 80
                x0 = (m * p) // k
                edge += [x for x in (x0 - 1, x0, x0 + 1) if abs(x) < 1 << 258]
            assert edge and all(abs(x) < 1 << 258 and abs(k) <= F9_SMALL_MAX for x in edge)
            c.add_groups("mul_small", f, k, [[split(x)] for x in edge])


# ---- the 8 x 32-bit path -------------------------------------------------------------------------------------------------------
def gen_fe_ops(c, rng):
    for f, p in enumerate(MODULI):
        Rm = (1 << 256) % p
        sp = [0, 1, 2, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, Rm, Rm * Rm % p]
        top = p >> 224 << 224  # the modulus's top word, nothing below it
        pat = [sum(0xFFFFFFFF << (64 * i) for i in range(4)), sum(0xFFFFFFFF << (64 * i + 32) for i in range(3)) + ((p >> 224) - 1 << 224),
               top, top + (1 << 223) if top + (1 << 223) < p else top + 1, (1 << 253) - 1, (1 << 224) - 1]
        V = sp + [1 << k for k in range(3, 254) if (1 << k) < p] + pat + [rng.randrange(p) for _ in range(60)]
        assert all(0 <= v < p for v in V)
        pairs = [(a, b) for a in sp + pat for b in V]
        pairs += [(rng.randrange(p), rng.randrange(p)) for _ in range(300)]
        land = []
        for a in sp[1:] + pat + [rng.randrange(1, p) for _ in range(20)]:
            land += [(a, p - 1 - a), (a, (p - a) % p), (a, a), (a, (a + 1) % p), ((a + 1) % p, a), (p - 1 - a, a), (0, a)]
        land += [(0, 0), (0, 1), (p - 1, p - 1), (p - 1, 1), (1, p - 1)]
        assert all(0 <= a < p and 0 <= b < p for a, b in pairs + land)
        for op in ("fe_mul", "fe_add", "fe_sub"):
            c.add_groups(op, f, 0, [[fe_slot(a), fe_slot(b)] for a, b in pairs + land])
        for op in ("fe_sqr", "fe_neg", "fe_dbl", "fe_from_raw", "fe_to_raw"):
            c.add_groups(op, f, 0, [[fe_slot(v)] for v in V + [rng.randrange(p) for _ in range(240)]])


# ---- curve operands ------------------------------------------------------------------------------------------------------------
LO9, HI9 = -(1 << 256), (1 << 256) + Q  # a coordinate is a product's output: any representative in (LO9, HI9)


def reps(residue):
    """every j for which residue + j q lies inside (LO9, HI9)"""
    js = [j for j in range(-7, 8) if LO9 < residue + j * Q < HI9]
    assert LO9 >= residue + (js[0] - 1) * Q and residue + (js[-1] + 1) * Q >= HI9
    return js


def m261(v):
    return v * RADIX % Q


def xyzz_res(P, lam):
    """the residues (2^261 form) of x, y, zz, zzz for the point P scaled by lam; all zero for the identity"""
    if P is None:
        return [0, 0, 0, 0]
    l2, l3 = lam * lam % Q, lam * lam * lam % Q
    return [m261(P[0] * l2), m261(P[1] * l3), m261(l2), m261(l3)]


def limbs_of(res, js):
    out = []
    for r, j in zip(res, js):
        v = r + j * Q
        assert LO9 < v < HI9
        out.append(split(v))
    return out


def rep_variants(res, kinds):
    """representative choices for a vector of residues: canonical; each coordinate alone through all its j; all of them
    together, counted from the low end and from the high end of their ranges"""
    n = len(res)
    if all(r == 0 for r in res):
        return [[0] * n]  # the identity is the all-zero limbs and nothing else
    rj = [reps(r) for r in res]
    out = [[0] * n]
    if "each" in kinds:
        for i in range(n):
            out += [[j if k == i else 0 for k in range(n)] for j in rj[i] if j]
    if "all" in kinds:
        depth = max(len(r) for r in rj)
        for t in range(depth):
            out.append([r[min(t, len(r) - 1)] for r in rj])
            out.append([r[max(len(r) - 1 - t, 0)] for r in rj])
    elif "ends" in kinds:
        out += [[r[0] for r in rj], [r[-1] for r in rj]]
    return out


def neg_limbs(res_y, j):
    """a y that arrives negated: f9_neg of the normalised limbs of -y (+ j q) -- negative limbs, the residue of y"""
    v = (-res_y) % Q + j * Q
    assert LO9 < v < HI9
    return [-x for x in split(v)]


@functools.lru_cache(maxsize=None)
def points():
    return [ec_mul(k, G) for k in (1, 2, 3, 5, 7, 11, 0x1234567, 0xDEADBEEFCAFE, Q // 3, MODULI[1] - 1)]


def pair_scenarios(rng):
    """(kind, P, lam_a, S, lam_b): generic sums, the same point twice under different scalings, a point and its negative"""
    pts = points()
    big = lambda: rng.randrange(2, Q)
    sc = []
    for i in range(4):
        sc.append(("generic", pts[i], (1, 2, big(), big())[i], pts[i + 3], (1, 3, 1, big())[i]))
    for P, la, lb in ((pts[0], 1, 1), (pts[1], 1, 2), (pts[4], 3, 5), (pts[6], big(), big()), (pts[9], Q - 1, 1), (pts[3], 2, Q - 2)):
        sc.append(("equal", P, la, P, lb))
        sc.append(("inverse", P, la, ec_neg(P), lb))
    return sc


def gen_add_cases(rng):
    """operand pairs of a full addition as (kind, a limbs x4, b limbs x4)"""
    by_kind = {"generic": [], "equal": [], "inverse": [], "identity": []}
    for n, (kind, P, la, S, lb) in enumerate(pair_scenarios(rng)):
        ra, rb = xyzz_res(P, la), xyzz_res(S, lb)
        kinds = ("each", "all") if n in (0, 1, 4, 5, 6, 7) else ("ends",)
        va, vb = rep_variants(ra, kinds), rep_variants(rb, kinds)
        combos = [(ja, vb[0]) for ja in va] + [(va[0], jb) for jb in vb[1:]]
        combos += [(va[-1 - t], vb[-1 - t]) for t in range(min(4, len(va), len(vb)))] + [(va[-1], vb[-2]), (va[-2], vb[-1])]
        for ja, jb in combos:
            by_kind[kind].append((kind, limbs_of(ra, ja), limbs_of(rb, jb)))
    ident = [ZERO9] * 4
    for P, lam in ((points()[2], 1), (points()[5], rng.randrange(2, Q)), (points()[8], 7)):
        r = xyzz_res(P, lam)
        for js in rep_variants(r, ("ends",)):
            by_kind["identity"] += [("identity", ident, limbs_of(r, js)), ("identity", limbs_of(r, js), ident)]
    by_kind["identity"].append(("identity", ident, ident))
    for _ in range(60):
        P, S = ec_mul(rng.randrange(1, MODULI[1]), G), ec_mul(rng.randrange(1, MODULI[1]), G)
        ra, rb = xyzz_res(P, rng.randrange(1, Q)), xyzz_res(S, rng.randrange(1, Q))
        by_kind["generic"].append(("generic", limbs_of(ra, [rng.choice(reps(r)) for r in ra]), limbs_of(rb, [rng.choice(reps(r)) for r in rb])))
    # neighbours of different kinds: a wave of the lane-split forms then diverges inside its pairs' and quads' neighbourhood
    order, n = [], max(len(v) for v in by_kind.values())
    for i in range(n):
        for k in ("generic", "equal", "identity", "inverse"):
            v = by_kind[k]
            if i < len(v) or k != "generic":
                order.append(v[i % len(v)])
    return order


def gen_curve_ops(c, rng):
    adds = gen_add_cases(rng)
    for _, a, b in adds:
        assert all(is_normalised(l) and LO9 < val(l) < HI9 for l in a + b)
    for op in ("add", "xaddl1", "xaddl2", "xaddl4", "xadd1", "xadd2", "xadd4"):
        for _, a, b in adds:
            c.add(op, 0, 0, a + b)
    # dbl, to_xyzz: one point
    singles = []
    for P, lam in zip(points(), (1, 2, 3, Q - 1, rng.randrange(2, Q), rng.randrange(2, Q), 1, 5, rng.randrange(2, Q), 1)):
        r = xyzz_res(P, lam)
        singles += [limbs_of(r, js) for js in rep_variants(r, ("each", "all") if lam in (1, 2) else ("ends",))]
    for a in singles:
        c.add("dbl", 0, 0, a)
        c.add("to_xyzz", 0, 0, a)
    c.add("dbl", 0, 0, [ZERO9] * 4)
    c.add("to_xyzz", 0, 0, [ZERO9] * 4)
    c.add("to_xyzz", 0, 1, singles[0])
    c.add("to_xyzz", 0, 1, [ZERO9] * 4)
    # madd (accumulator + affine point) and from_pair (affine + affine): the second y also with negative limbs
    for n, (kind, P, la, S, lb) in enumerate(pair_scenarios(rng)):
        ra, rq = xyzz_res(P, la), xyzz_res(S, 1)[:2]
        kinds = ("each", "all") if n in (0, 1, 4, 5, 6, 7) else ("ends",)
        va, vq = rep_variants(ra, kinds), rep_variants(rq, kinds)
        for ja, jq in [(ja, vq[0]) for ja in va] + [(va[0], jq) for jq in vq[1:]] + [(va[-1], vq[-1]), (va[-2], vq[-2])]:
            acc, qx = limbs_of(ra, ja), limbs_of(rq[:1], jq[:1])[0]
            for qy in (limbs_of(rq[1:], jq[1:])[0], neg_limbs(rq[1], jq[1] if LO9 < (-rq[1]) % Q + jq[1] * Q < HI9 else 0)):
                assert all(is_normalised(l) for l in acc + [qx]) and (is_normalised(qy) or is_normalised([-x for x in qy]))
                c.add("madd", 0, 0, acc + [qx, qy])
        # the accumulator is the identity: inf set, its coordinates are whatever the last sum left
        for jq in vq[:3] + vq[-2:]:
            qx, qy = limbs_of(rq, jq)
            c.add("madd", 0, 1, limbs_of(ra, va[0]) + [qx, qy])
            c.add("madd", 0, 1, [ZERO9] * 4 + [qx, neg_limbs(rq[1], 0)])
        r1 = xyzz_res(P, 1)[:2]
        v1 = rep_variants(r1, kinds)
        for j1, jq in [(j1, vq[0]) for j1 in v1] + [(v1[0], jq) for jq in vq[1:]] + [(v1[-1], vq[-1]), (v1[-2], vq[-2]), (v1[-1], vq[-2])]:
            x1, y1 = limbs_of(r1, j1)
            x2 = limbs_of(rq[:1], jq[:1])[0]
            for y2 in (limbs_of(rq[1:], jq[1:])[0], neg_limbs(rq[1], jq[1] if LO9 < (-rq[1]) % Q + jq[1] * Q < HI9 else 0)):
                c.add("from_pair", 0, 0, [x1, y1, x2, y2])
    # xmadd_pair: chains of eight mixed additions per lane pair, from inf; neighbouring pairs run different chains
    pts = points()
    for n in range(48):
        P, S, T = pts[n % 5], pts[5 + n % 4], pts[(n + 2) % 7 + 3] if (n + 2) % 7 + 3 != 5 + n % 4 else pts[9]
        if n >= 24:
            P, S, T = (ec_mul(rng.randrange(1, MODULI[1]), G) for _ in range(3))
        P2 = ec_add(P, P)
        if n % 2 == 0:
            steps = [(P, 0), (P, 0), (P2, 1), (S, 0), (S, 1), (S, 0), (T, 0), (P, 1)]
        else:
            ST = ec_add(S, T)
            steps = [(S, 0), (T, 1 if n % 4 == 3 else 0), (ec_add(S, ec_neg(T)) if n % 4 == 3 else ST, 1), (P, 1), (P, 1), (P2, 0), (T, 0), (S, 1)]
        for pt, negate in steps:
            rx, ry = xyzz_res(pt, 1)[:2]
            jx = rng.choice(reps(rx)) if n % 3 else 0
            if negate:  # add -pt: the y of pt, negated limb by limb
                jy = rng.choice(reps(ry)) if n % 3 else 0
                qy = [-x for x in split(ry + jy * Q)]
            else:
                qy = split(ry + (rng.choice(reps(ry)) if n % 3 else 0) * Q)
            c.add("xmadd_pair", 0, 0, [split(rx + jx * Q), qy])


@functools.lru_cache(maxsize=None)
def all_cases():
    """(rows, the IN array); lane-split records last, so that the host leg is a prefix-free filter on the op"""
    rng = random.Random(0x0F9)
    c = Cases()
    gen_limb_ops(c, rng)
    gen_fe_ops(c, rng)
    gen_curve_ops(c, rng)
    c.rows.sort(key=lambda r: r[0])  # one run of records, hence one launch, per op (stable: the order inside an op stays)
    return c.rows, c.array()


def host_cases():
    rows, arr = all_cases()
    keep = [i for i, r in enumerate(rows) if r[0] in HOST_OPS]
    return [rows[i] for i in keep], np.ascontiguousarray(arr[keep])


# ---- the judge -------------------------------------------------------------------------------------------------------------
def pt_of_limbs(c4):
    """the affine point that four operand coordinates stand for (identity: zz all-zero limbs)"""
    if all(x == 0 for x in c4[2]):
        return None
    return affine_of([val(l) for l in c4])


def affine_q(qx, qy):
    rinv = pow(RADIX, -1, Q)
    return (val(qx) * rinv % Q, val(qy) * rinv % Q)


def same_limbs(got, one_lane, who):
    """the sum of a lane-split form against the one-lane function's sum of the same launch: limb for limb, all four coordinates"""
    for k in range(4):
        if got[k] != one_lane[k]:
            return "coordinate %d %s differs from %s's %s (by %s)" % (k, hexl(got[k]), who, hexl(one_lane[k]),
                                                                     near(val(got[k]) - val(one_lane[k]), Q))
    return None


def judge_record(row, out, state):
    """reasons (slot, text) for one record; `out` is the record of the OUT file as a list of 112 integers.  `state` carries an
    xmadd_pair chain from one record to the next."""
    op, f, arg, s = row
    p = MODULI[f]
    name = OP_NAME[op]
    o = [out[9 * i:9 * i + 9] for i in range(OUT_SLOTS)]
    inf, wm, zero = out[108], out[109], out[110]
    bad = []

    def say(slot, err):
        if err:
            bad.append((slot, err))

    if name == "unpack":
        for i in range(8):
            say(i, check_limbs(o[i], val32(s[i][:8])))
    elif name == "pack":
        for i in range(8):
            say(i, check_words(o[i][:8], val32(s[i][:8])))
    elif name == "norm":
        for i in range(8):
            say(i, check_limbs(o[i], val(s[i])))
    elif name == "mul":
        for i in range(4):
            err = check_mont(o[i], val(s[2 * i]) * val(s[2 * i + 1]), p)
            if not err and not -(1 << 256) < val(o[i]) < (1 << 256) + p:
                err = "value %s outside (-2^256, 2^256 + p)" % near(val(o[i]), p)
            say(2 * i, err)
    elif name == "sqr":
        for i in range(8):
            say(i, check_mont(o[i], val(s[i]) ** 2, p))
    elif name in ("mul2_add", "mul2_sub", "mul2_split"):
        sg = 1 if name == "mul2_add" else -1
        for i in range(2):
            a, b, cc, d = (val(x) for x in s[4 * i:4 * i + 4])
            say(4 * i, check_mont(o[i], a * b + sg * cc * d, p))
    elif name == "dot":
        say(0, check_mont(o[0], dot_sum(s, arg), p))
    elif name == "canon":
        for i in range(8):
            say(i, check_limbs(o[i], val(s[i]) % p))
    elif name == "iszero":
        for i in range(8):
            if bool(zero >> i & 1) != (val(s[i]) % p == 0):
                say(i, "is_zero_mod_p says %s" % bool(zero >> i & 1))
    elif name == "reduce_pack":
        for i in range(8):
            say(i, check_words(o[i][:8], val(s[i]) % p))
    elif name == "mul_small":
        for i in range(8):
            v, e = val(o[i]), val(s[i]) * arg % p
            if not is_normalised(o[i]):
                say(i, "%s is not normalised" % hexl(o[i]))
            elif v != e and v != e + p:
                say(i, "value %s, expected x c mod p = %x or that + p (x c = %s)" % (near(v, p), e, near(val(s[i]) * arg, p)))
    elif name.startswith("fe_"):
        Ri = pow(1 << 256, -1, p)
        two = {"fe_mul": lambda a, b: a * b * Ri % p, "fe_add": lambda a, b: (a + b) % p, "fe_sub": lambda a, b: (a - b) % p}
        one = {"fe_sqr": lambda a: a * a * Ri % p, "fe_neg": lambda a: -a % p, "fe_dbl": lambda a: 2 * a % p,
               "fe_from_raw": lambda a: (a << 256) % p, "fe_to_raw": lambda a: a * Ri % p}
        if name in two:
            for i in range(4):
                say(2 * i, check_words(o[i][:8], two[name](val32(s[2 * i][:8]), val32(s[2 * i + 1][:8]))))
        else:
            for i in range(8):
                say(i, check_words(o[i][:8], one[name](val32(s[i][:8]))))
    elif name == "madd":
        q = affine_q(s[4], s[5])
        want = ec_add(None if arg else pt_of_limbs(s[:4]), q)
        if bool(inf) != (want is None):
            say(0, "inf = %d, expected %s" % (inf, want is None))
        elif want is not None:
            say(0, check_point(o[:4], want))
    elif name == "from_pair":
        want = ec_add(affine_q(s[0], s[1]), affine_q(s[2], s[3]))
        if bool(inf) != (want is None):
            say(0, "inf = %d, expected %s" % (inf, want is None))
        elif want is not None:
            say(0, check_point(o[:4], want))
    elif name == "dbl":
        P = pt_of_limbs(s[:4])
        say(0, check_point(o[:4], ec_add(P, P)))
    elif name == "add":
        say(0, check_point(o[:4], ec_add(pt_of_limbs(s[:4]), pt_of_limbs(s[4:8]))))
    elif name == "to_xyzz":
        if arg or all(x == 0 for x in s[2]):
            want = [0, (1 << 256) % Q, 0, 0]  # xyzz_identity()
        else:
            r5 = pow(32, -1, Q)  # x 2^261 -> x 2^256
            want = [val(l) * r5 % Q for l in s[:4]]
        for i in range(4):
            say(i, check_words(o[i][:8], want[i]))
    elif op in LANES:
        L = LANES[op]
        want = ec_add(pt_of_limbs(s[:4]), pt_of_limbs(s[4:8]))
        part, err = state.get("lanes", "all"), None
        if part in ("all", "point"):
            err = check_point(o[:4], want) or check_point(o[4:8], want)
            masks = [wm >> (4 * r) & 15 for r in range(4)]
            if not err and (sum(masks) != 15 or masks[0] | masks[1] | masks[2] | masks[3] != 15 or any(masks[L:])):
                err = "write masks %s of the %d lanes do not cover each coordinate once" % (masks, L)
        if part in ("all", "limbs") and not err:
            err = same_limbs(o[:4], o[4:8], "xyzz9_add")
        say(0, err)
    elif name == "xmadd_pair":
        step = state.get("step", 0)
        acc = None if step == 0 else state["acc"]
        acc = ec_add(acc, affine_q(s[0], s[1]))
        state["acc"], state["step"] = acc, (step + 1) % 8
        if inf != (7 if acc is None else 0):
            say(0, "inf flags (lane A, lane B, one lane) = %s, expected %s" % (bin(inf), acc is None))
        elif acc is not None:
            part, err = state.get("lanes", "all"), None
            if part in ("all", "point"):
                err = check_point(o[:4], acc) or check_point(o[4:8], acc)
                if not err and o[8] != o[3]:
                    err = "lane B's zzz %s differs from lane A's %s" % (hexl(o[8]), hexl(o[3]))
            if part in ("all", "limbs") and not err:
                err = same_limbs(o[:4], o[4:8], "xyzz9_madd")
            say(0, err)
    else:
        raise AssertionError("no judge for op %d" % op)
    return bad


def judge(rows, out, only=None, lanes="all"):
    """the failures of an OUT array (n x 112) as report lines: op, field, record, slot, the reason and the operands.
    lanes: which half of the lane-split forms' checks to make -- "point" (every coordinate written once, a valid operand, the
    Python point, from the lanes and from the one-lane function), "limbs" (limb for limb the one-lane function's sum), or "all" for both."""
    assert out.shape == (len(rows), OUT_WORDS), (out.shape, len(rows))
    assert lanes in ("all", "point", "limbs")
    outl = out.tolist()
    fails, state, first = [], {"lanes": lanes}, {}
    for i, row in enumerate(rows):
        op, f, arg, s = row
        first.setdefault(op, i)
        if only is not None and not only(OP_NAME[op]):
            continue
        p = MODULI[f]
        for slot, err in judge_record(row, outl[i], state):
            words = OP_NAME[op].startswith("fe_") or OP_NAME[op] in ("unpack", "pack")
            ops = s[slot:slot + (8 if op >= 30 else 4 if "mul2" in OP_NAME[op] else 2 if OP_NAME[op] in ("mul", "fe_mul", "fe_add", "fe_sub") else 1)]
            if OP_NAME[op] == "dot":
                ops = s
            shown = ["%064x" % val32(l[:8]) for l in ops] if words else [show(l, p) for l in ops]
            fails.append("%s/%s record %d (no. %d of its op) slot %d arg %d: %s\n    operands: %s"
                         % (OP_NAME[op], "Fr" if f else "Fq", i, i - first[op], slot, arg, err, "\n              ".join(shown)))
    return fails


def write_in(path):
    rows, arr = all_cases()
    arr.tofile(path)
    return rows


def read_out(path, n):
    out = np.fromfile(path, dtype=np.int32)
    assert out.size == n * OUT_WORDS, "OUT holds %d words for %d records" % (out.size, n)
    return out.reshape(n, OUT_WORDS)
