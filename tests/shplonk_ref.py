"""The comparator of the SHPLONK tests: halo2_proofs v2023_04_20's second multi-open argument (ProverSHPLONK /
VerifierSHPLONK, src/poly/kzg/multiopen/shplonk/) restated on Python integers -- nothing of the library under test.  The
order is the contract of DESIGN.md section 16.  Everything up to and including the evaluations is the GWC proof's
(tests/multi_ref.py); the scalar GWC squeezes as v behind them is SHPLONK's y.

  intermediate_sets(queries)                    construct_intermediate_sets: commitments, rotation sets, T
  verify(vk, instances, proof, circuits=1)      1 accepted, 0 rejected, -1 malformed (multi_ref.verify's classes)
  create_proof(be, vk, advice, instance)        the reference PROVER: the walk of tests/arith_level.py up to the evaluations
                                                (its GWC tail is cut off), then SHPLONK's tail in upstream's order -- per
                                                rotation set the numerator and its CHAINED divisions by (X - r), never the
                                                per-point form the device may use -- over the same backend interface
                                                (lincomb, kate, commit), so it runs on the host backend and on the device one.

Group work and the pairing: the oracle's primitives through orc, as in multi_ref.
"""
import ctypes

import numpy as np

import arith_level
import multi_ref
import orc
from circuit import ADVICE, DELTA, FIXED, INSTANCE, R, omega_for
from multi_ref import _add, _identity, _ints, _mul, _p, _Reader, circuit_queries, n_sets


def proof_len(cs, N: int) -> int:
    """multi_ref.proof_len with 2 in place of the number of point sets"""
    return multi_ref.proof_len(cs, N) - 64 * (multi_ref.n_point_sets(cs) - 2)


def intermediate_sets(queries):
    """queries: (point, commitment key) pairs in create_proof's order.  -> (sets, T): sets = [(points, keys)] -- the
    commitments in first-appearance order, those opened at the same SET of points together, the sets in the order of their
    first commitment, a set's points in the order its first commitment meets them; T = every distinct point."""
    order, points_of, T = [], {}, []
    for point, key in queries:
        if key not in points_of:
            points_of[key] = []
            order.append(key)
        if point not in points_of[key]:
            points_of[key].append(point)
        if point not in T:
            T.append(point)
    sets = []
    for key in order:
        for points, keys in sets:
            if set(points) == set(points_of[key]):
                keys.append(key)
                break
        else:
            sets.append((list(points_of[key]), [key]))
    return sets, T


def _inv(a: int) -> int:
    return pow(a % R, R - 2, R)


def _lagrange_at(points, values, u: int) -> int:
    """the interpolant of (points, values) at u"""
    acc = 0
    for a, pa in enumerate(points):
        num = den = 1
        for c, pc in enumerate(points):
            if c != a:
                num = num * (u - pc) % R
                den = den * (pa - pc) % R
        acc = (acc + values[a] * num % R * _inv(den)) % R
    return acc


def _interpolate(points, values) -> list:
    """coefficients (low first) of the interpolant"""
    out = [0] * len(points)
    for a, pa in enumerate(points):
        num, den = [1], 1
        for c, pc in enumerate(points):
            if c != a:
                num = [(lo - pc * hi) % R for lo, hi in zip([0] + num, num + [0])]
                den = den * (pa - pc) % R
        f = values[a] * _inv(den) % R
        out = [(o + f * x) % R for o, x in zip(out, num)]
    return out


def _replay(vk, instances, proof):
    """The proof read as multi_ref.verify reads it, up to and including the evaluations.  -> (reader, x, queries) with
    queries = [(point, key, commitment, evaluation)] in create_proof's order; None in the reader's place: malformed."""
    cs, N = vk.cs, len(instances)
    k, n = cs.k, 1 << cs.k
    A, NL, S, P = cs.n_advice, len(cs.lookups), n_sets(cs), len(cs.perm_columns)
    d, bf = cs.degree(), cs.blinding_factors()
    chunk, qpd = d - 2, d - 1
    w = omega_for(k)
    w_inv = pow(w, R - 2, R)
    inst = [_ints(i) for i in instances]

    def rot(x, r):
        return x * pow(w if r >= 0 else w_inv, abs(r), R) % R

    t = _Reader(proof)
    t.common_scalar(vk.vk_repr)
    for c in range(N):
        for col in inst[c]:
            for v in col:
                t.common_scalar(v)
    adv_c = [[t.point() for _ in range(A)] for _ in range(N)]
    theta = t.squeeze()
    pin_c, ptab_c = [[None] * NL for _ in range(N)], [[None] * NL for _ in range(N)]
    for c in range(N):
        for l in range(NL):
            pin_c[c][l] = t.point()
            ptab_c[c][l] = t.point()
    beta = t.squeeze()
    gamma = t.squeeze()
    pz_c = [[t.point() for _ in range(S)] for _ in range(N)]
    lz_c = [[t.point() for _ in range(NL)] for _ in range(N)]
    random_c = t.point()
    y = t.squeeze()
    h_c = [t.point() for _ in range(qpd)]
    x = t.squeeze()
    xn = pow(x, n, R)
    ev = {}
    for c in range(N):
        for i in range(len(cs.advice_queries)):
            ev[c, "adv", i] = t.scalar()
    fix_e = [t.scalar() for _ in cs.fixed_queries]
    random_e = t.scalar()
    sig_e = [t.scalar() for _ in range(P)]
    for c in range(N):
        for s in range(S):
            ev[c, "pz", s, 0] = t.scalar()
            ev[c, "pz", s, 1] = t.scalar()
            if s + 1 < S:
                ev[c, "pz", s, 2] = t.scalar()
    for c in range(N):
        for l in range(NL):
            for e in range(5):
                ev[c, "lk", l, e] = t.scalar()
    if t.bad:
        return None, 0, []

    num = (xn - 1) * pow(n, R - 2, R) % R
    l0 = llast = lblind = 0
    for r in range(-(bf + 1), 1):
        wi = rot(1, r)
        li = num * wi % R * pow((x - wi) % R, R - 2, R) % R
        if r == -(bf + 1):
            llast = li
        elif r == 0:
            l0 = li
        else:
            lblind = (lblind + li) % R
    lactive = (1 - llast - lblind) % R

    def inst_eval(c, col, r):
        pt, acc, wi = rot(x, r), 0, 1
        for v in inst[c][col]:
            acc = (acc + v * wi % R * pow((pt - wi) % R, R - 2, R)) % R
            wi = wi * w % R
        return acc * num % R

    acc = 0
    for c in range(N):
        def cell(qi, c=c):
            kind, col, r = cs.queries[qi]
            if kind == ADVICE:
                return ev[c, "adv", cs.advice_queries.index((col, r))]
            if kind == FIXED:
                return fix_e[cs.fixed_queries.index((col, r))]
            assert kind == INSTANCE
            return inst_eval(c, col, r)

        terms = [g.eval(cell) for g in cs.gates]
        if S:
            z = lambda s, e, c=c: ev[c, "pz", s, e]  # noqa: E731
            terms.append((1 - z(0, 0)) * l0)
            terms.append((z(S - 1, 0) ** 2 - z(S - 1, 0)) * llast)
            for s in range(1, S):
                terms.append((z(s, 0) - z(s - 1, 2)) * l0)
            for s in range(S):
                left, right = z(s, 1), z(s, 0)
                cd = beta * x % R * pow(DELTA, s * chunk, R) % R
                for pc in range(s * chunk, min(P, (s + 1) * chunk)):
                    kind, col = cs.perm_columns[pc]
                    ce = cell(cs.queries.index((kind, col, 0)))
                    left = left * (beta * sig_e[pc] + ce + gamma) % R
                    right = right * (ce + cd + gamma) % R
                    cd = cd * DELTA % R
                terms.append((left - right) * lactive)
        for l, (ins, tabs) in enumerate(cs.lookups):
            ai = ti = 0
            for e_in, e_tab in zip(ins, tabs):
                ai = (ai * theta + e_in.eval(cell)) % R
                ti = (ti * theta + e_tab.eval(cell)) % R
            zl, zn, ap, apm, sp = (ev[c, "lk", l, e] for e in range(5))
            terms.append((1 - zl) * l0)
            terms.append((zl * zl - zl) * llast)
            terms.append(((ap + beta) * (sp + gamma) % R * zn - (ai + beta) * (ti + gamma) % R * zl) * lactive)
            terms.append((ap - sp) * l0)
            terms.append((ap - apm) * (ap - sp) % R * lactive)
        for term in terms:
            acc = (acc * y + term) % R
    expected_h = acc * pow((xn - 1) % R, R - 2, R) % R

    h_commit = _identity()
    for i in reversed(range(qpd)):
        h_commit = _add(_mul(h_commit, xn), h_c[i])

    qs = []
    for c in range(N):
        com = {"adv": adv_c[c], "pz": pz_c[c], "lz": lz_c[c], "pin": pin_c[c], "ptab": ptab_c[c]}
        for r, fam, idx, key in circuit_queries(cs):
            qs.append((rot(x, r % n), (c, fam, idx), com[fam][idx], ev[(c,) + key]))
    for i, (col, r) in enumerate(cs.fixed_queries):
        qs.append((rot(x, r % n), ("fixed", col), vk.fixed_c[col], fix_e[i]))
    for pc in range(P):
        qs.append((x, ("sigma", pc), vk.sigma_c[pc], sig_e[pc]))
    qs.append((x, ("h",), h_commit, expected_h))
    qs.append((x, ("random",), random_c, random_e))
    return t, x, qs


def _set_scalars(sets, T, evals, y: int, v: int, u: int):
    """per rotation set v^i z'_i (z'_0 = 1, z'_i = z_i / z_0, z_i = prod over T minus S_i of (u - r)), the sum
    r = sum_i v^i z'_i sum_j y^j R_ij(u), and Z_0 = prod over S_0 of (u - r)"""
    def z(points):
        acc = 1
        for r in T:
            if r not in points:
                acc = acc * (u - r) % R
        return acc

    z0_inv = _inv(z(sets[0][0]))
    weights, rsum = [], 0
    for i, (points, keys) in enumerate(sets):
        wi = pow(v, i, R) * (z(points) * z0_inv % R if i else 1) % R
        weights.append(wi)
        for j, key in enumerate(keys):
            rsum = (rsum + wi * pow(y, j, R) % R * _lagrange_at(points, [evals[key, p] for p in points], u)) % R
    Z0 = 1
    for r in sets[0][0]:
        Z0 = Z0 * (u - r) % R
    return weights, rsum, Z0


def verify(vk, instances, proof: bytes, circuits: int = 1) -> int:
    """instances: one uint64[n_instance, len, 4] array per circuit of the proof (`circuits` of them)."""
    assert len(instances) == circuits
    t, _, qs = _replay(vk, instances, proof)
    if t is None:
        return -1
    y = t.squeeze()
    v = t.squeeze()
    h1 = t.point()
    if t.bad:
        return -1
    u = t.squeeze()
    h2 = t.point()
    if t.bad:
        return -1
    sets, T = intermediate_sets([(q[0], q[1]) for q in qs])
    commitment = {q[1]: q[2] for q in qs}
    evals = {(q[1], q[0]): q[3] for q in qs}
    weights, rsum, Z0 = _set_scalars(sets, T, evals, y, v, u)
    rb = _identity()
    for wi, (_, keys) in zip(weights, sets):
        for j, key in enumerate(keys):
            rb = _add(rb, _mul(commitment[key], wi * pow(y, j, R) % R))
    rb = _add(rb, _mul(vk.g0, (-rsum) % R))
    rb = _add(rb, _mul(h1, (-Z0) % R))
    rb = _add(rb, _mul(h2, u))
    L = orc.load()
    neg = np.zeros(12, np.uint64)
    L.orc_g1_neg(_p(neg), _p(rb))
    ps = np.zeros((2, 8), np.uint64)
    L.orc_g1_to_affine(_p(ps[0]), _p(h2))
    L.orc_g1_to_affine(_p(ps[1]), _p(neg))
    g2s = np.array([list(vk.params.s_g2), list(vk.params.g2)], dtype=np.uint64)
    if not L.orc_pairing_check(_p(ps), _p(g2s), ctypes.c_size_t(2)):
        return 0
    return 1 if t.pos == len(t.data) else 0


# ---------------------------------------------------------------------------------------------------- the reference prover
class _Recorder:
    """A backend of tests/arith_level.py that remembers the coefficient forms its create_proof makes: the five to_coeff
    results (advice, instance, permutation z, lookup z, permuted columns, in that order), the random polynomial and h(X)
    (the first lincomb without a constant to take off)."""

    def __init__(self, be):
        self._be, self.coeff, self.random_poly, self.h_poly = be, [], None, None

    def __getattr__(self, name):
        return getattr(self._be, name)

    def to_coeff(self, m):
        out = self._be.to_coeff(m)
        self.coeff.append(out)
        return out

    def rand(self, tag, count):
        out = self._be.rand(tag, count)
        if tag == arith_level.TAG_RANDOM_POLY:
            self.random_poly = out
        return out

    def lincomb(self, vs, coeffs, sub0, out):
        self._be.lincomb(vs, coeffs, sub0, out)
        if sub0 is None and self.h_poly is None:
            self.h_poly = out


class _OneEmptyInstanceColumn:
    """A circuit without instance columns as arith_level.create_proof can take it: that walk reshapes the instance to
    (n_instance, -1, 4), which numpy refuses for no columns.  One column of no rows adds nothing to the transcript and is
    read by no query, so the bytes are the circuit's own."""
    n_instance = 1

    def __init__(self, cs):
        self._cs = cs

    def __getattr__(self, name):
        return getattr(self._cs, name)


def _one_column(be, low: list):
    """a column of the backend with the given low coefficients"""
    col = np.zeros((1, be.n, 4), np.uint64)
    col[0, :len(low)] = np.stack([orc.fr_from_int(c) for c in low])
    return be.cols(col)[0]


def create_proof(be, vk, advice, instance) -> bytes:
    """One circuit.  vk: multi_ref.Vk of the key `be` was made for (its commitments are not used: the proof's prefix is
    read back only for the transcript's state, x and the evaluations)."""
    cs = vk.cs
    rec = _Recorder(be)
    if cs.n_instance:
        gwc = arith_level.create_proof(rec, cs, orc.fr_from_int(vk.vk_repr), advice, instance)
    else:
        gwc = arith_level.create_proof(rec, _OneEmptyInstanceColumn(cs), orc.fr_from_int(vk.vk_repr), advice, np.zeros((1, 0, 4), np.uint64))
    prefix = gwc[:len(gwc) - 64 * multi_ref.n_point_sets(cs)]
    t, x, qs = _replay(vk, [instance], prefix)
    assert t is not None and t.pos == len(prefix)
    adv_p, _, pz_p, lz_p, perm_p = rec.coeff
    poly = {("h",): rec.h_poly, ("random",): rec.random_poly}
    for key in {q[1] for q in qs}:
        if key[0] == 0:
            fam, idx = key[1], key[2]
            poly[key] = {"adv": adv_p, "pz": pz_p, "lz": lz_p}[fam][idx] if fam in ("adv", "pz", "lz") else \
                perm_p[2 * idx + (fam == "ptab")]
        elif key[0] == "fixed":
            poly[key] = be.fixed_polys[key[1]]
        elif key[0] == "sigma":
            poly[key] = be.sigma_polys[key[1]]
    tr = arith_level.Transcript(be.keccak)
    tr.buf, tr.out = t.buf, bytearray(prefix)

    # 1. y, v   2. per rotation set N_i = sum_j y^j (P_ij - R_ij) and Q_i = N_i / prod (X - r), one division after another
    y, v = tr.squeeze(), tr.squeeze()
    sets, T = intermediate_sets([(q[0], q[1]) for q in qs])
    evals = {(q[1], q[0]): q[3] for q in qs}
    quotients = be.zeros(len(sets))
    work = be.zeros(2)
    for i, (points, keys) in enumerate(sets):
        ypow = [pow(y, j, R) for j in range(len(keys))]
        be.lincomb([poly[key] for key in keys], ypow, None, work[0])
        low = [0] * len(points)  # sum_j y^j R_ij, at most |S_i| coefficients
        for yj, key in zip(ypow, keys):
            rij = _interpolate(points, [evals[key, p] for p in points])
            low = [(a + yj * c) % R for a, c in zip(low, rij)]
        be.put(work[0], 0, _one_column(be, [(be.get1(work[0], d) - low[d]) % R for d in range(len(points))]), 0, len(points))
        src, dst = work[0], work[1]
        for r in points:
            be.kate(src, r, dst)
            src, dst = dst, src
        be.lincomb([src], [1], None, quotients[i])
    # 3. h1_x = sum_i v^i Q_i   4. its commitment   5. u
    h1 = be.zeros(1)[0]
    be.lincomb([quotients[i] for i in range(len(sets))], [pow(v, i, R) for i in range(len(sets))], None, h1)
    tr.write_point(be.commit(h1[None], False)[0])
    u = tr.squeeze()

    # 6. z_i   7. L = sum_i v^i z_i sum_j y^j (P_ij - R_ij(u)) - Z_T(u) h1_x   8. h2_x = z_0^-1 L / (X - u)   9. its commitment
    def z_of(points):
        acc = 1
        for r in T:
            if r not in points:
                acc = acc * (u - r) % R
        return acc

    zT = z_of([])
    terms, coeffs, const = [], [], 0
    for i, (points, keys) in enumerate(sets):
        wi = pow(v, i, R) * z_of(points) % R
        for j, key in enumerate(keys):
            c = wi * pow(y, j, R) % R
            terms.append(poly[key])
            coeffs.append(c)
            const = (const + c * _lagrange_at(points, [evals[key, p] for p in points], u)) % R
    be.lincomb(terms + [h1], coeffs + [(-zT) % R], const, work[0])
    be.kate(work[0], u, work[1])
    h2 = be.zeros(1)[0]
    be.lincomb([work[1]], [_inv(z_of(sets[0][0]))], None, h2)
    tr.write_point(be.commit(h2[None], False)[0])
    return bytes(tr.out)
