"""The comparator of the proof tests: halo2's `verify_proof` restated on Python integers -- nothing of the library under
test -- for every proof form the library makes, all options at once:

  circuits     N instances of one circuit behind ONE transcript (`instances: &[&[&[F]]]`)
  multi-open   GWC or SHPLONK (halo2_proofs v2023_04_20 src/poly/kzg/multiopen/)
  transcript   EVM or BLAKE2B (tests/transcript_ref.py), chosen by argument
  phases       advice phases and challenges (src/plonk/verifier.rs): after the vk scalar and the
               instances the phases in ascending order -- the commitments of that phase's advice columns (every circuit's,
               ascending column), then one squeezed scalar per challenge of that phase (ascending index); theta follows
               the last phase; Expression::Challenge(j) evaluates to challenge j
  shuffles     cs.shuffles: [(inputs [Expr], shuffles [Expr])] (privacy-scaling-explorations/halo2 v0.3.0 on,
               src/plonk/shuffle/verifier.rs): each circuit's products z_j are read behind every
               circuit's lookup products, their evaluations z_j(x), z_j(wx) behind every circuit's lookup evaluations, their
               queries behind the circuit's lookup queries; in h(x), behind a circuit's lookup terms, per shuffle
               l_0 (1 - z), l_last (z^2 - z), (1 - (l_last + l_blind)) (z(wx) (s + gamma) - z (a + gamma)), a and s the
               theta-folds of the two tuples

KZG, QUERY_INSTANCE = false.  oracle/prover.c's orc_verify_proof_pairing is the case N = 1, GWC, EVM, one phase, no shuffle;
the host tests hold this file against it there, and tests/test_proof_golden_host.py against recorded proofs elsewhere.

  counts / proof_len / circuit_queries / n_point_sets / point_set_lengths     the proof's shape
  replay(vk, instances, proof, ...)   THE function that reads a proof: from the vk scalar through the evaluations; h(x) and
                                      the opening queries rebuilt
  verify(..., scheme)                 replay, then one multi-open tail -> Result, verdict 1 accepted, 0 rejected, -1 malformed
                                      (the classes of zg_verifier_verify_*)
  create_proof(be, vk, ...)           the reference PROVER of one circuit over a backend of tests/arith_level.py: that file's
                                      walk, and for SHPLONK its GWC tail cut off and SHPLONK's in upstream's order -- per
                                      rotation set the numerator and its CHAINED divisions by (X - r), never the per-point
                                      form the device may use

  expressions     Expr.eval of harness/circuit.py on the proof's evaluations and the challenge values
  instance evals  the Lagrange form, (x^n - 1)/n * sum_i inst_i w^i / (x w^rot - w^i)
  group work      the oracle's primitives through orc.load(): orc_g1_mul, orc_g1_add, orc_pairing_check
"""
import ctypes

import numpy as np

import arith_level
import orc
from arith_level import n_sets
from circuit import ADVICE, DELTA, FIXED, INSTANCE, R, omega_for
from transcript_ref import BLAKE2B, EVM, READER, WRITER, Q  # noqa: F401 -- the codes are this module's arguments

CHALLENGE = 3
GWC, SHPLONK = 0, 1


# ---------------------------------------------------------------------------------------------------- the proof's shape
def shuffles_of(cs):
    return list(getattr(cs, "shuffles", []))


def phases_of(cs, advice_phase, challenge_phase):
    """[(columns, challenges)] per phase; empty settings: one phase, no challenge squeezed"""
    adv = list(advice_phase) if advice_phase else [0] * cs.n_advice
    out = [([], []) for _ in range(max(adv + [0]) + 1)]
    for c, ph in enumerate(adv):
        out[ph][0].append(c)
    for j, ph in enumerate(challenge_phase or []):
        out[ph][1].append(j)
    return out


def advice_order(cs, N, advice_phase):
    """(phase, circuit, column) in the order a proof of N circuits holds its advice commitments"""
    return [(ph, c, col) for ph, (cols, _) in enumerate(phases_of(cs, advice_phase, [])) for c in range(N) for col in cols]


def circuit_queries(cs):
    """One circuit's own opening queries in create_proof's order: (rotation, family, index, evaluation key)."""
    S, NL, last = n_sets(cs), len(cs.lookups), -(cs.blinding_factors() + 1)
    out = [(rot, "adv", col, ("adv", i)) for i, (col, rot) in enumerate(cs.advice_queries)]
    for s in range(S):
        out += [(0, "pz", s, ("pz", s, 0)), (1, "pz", s, ("pz", s, 1))]
    for s in reversed(range(S - 1)):
        out.append((last, "pz", s, ("pz", s, 2)))
    for l in range(NL):
        out += [(0, "lz", l, ("lk", l, 0)), (0, "pin", l, ("lk", l, 2)), (0, "ptab", l, ("lk", l, 4)),
                (-1, "pin", l, ("lk", l, 3)), (1, "lz", l, ("lk", l, 1))]
    for j in range(len(shuffles_of(cs))):
        out += [(0, "sz", j, ("sh", j, 0)), (1, "sz", j, ("sh", j, 1))]
    return out


def point_set_lengths(cs, N: int) -> dict:
    """{rotation mod n: how many (circuit, polynomial) pairs a proof of N circuits opens at x * omega^rotation}: the lists
    that GWC's tail walks -- every circuit's own queries, then the fixed columns, the sigmas, h and the random polynomial
    at rotation 0."""
    n, out = 1 << cs.k, {}
    for r, *_ in circuit_queries(cs):
        out[r % n] = out.get(r % n, 0) + N
    for _, r in cs.fixed_queries:
        out[r % n] = out.get(r % n, 0) + 1
    out[0] = out.get(0, 0) + len(cs.perm_columns) + 2
    return out


def n_point_sets(cs) -> int:
    return len(point_set_lengths(cs, 1))


def counts(cs, N: int, scheme: int):
    """(points, scalars) of a proof of N circuits:
    N (A + 3 NL + S + NS) + 1 + (d - 1) + tail,  N (AQ + (S ? 3 S - 1 : 0) + 5 NL + 2 NS) + FQ + 1 + P"""
    A, NL, S, NS, P, d = cs.n_advice, len(cs.lookups), n_sets(cs), len(shuffles_of(cs)), len(cs.perm_columns), cs.degree()
    AQ, FQ = len(cs.advice_queries), len(cs.fixed_queries)
    tail = 2 if scheme == SHPLONK else n_point_sets(cs)
    return (N * (A + 3 * NL + S + NS) + 1 + (d - 1) + tail, N * (AQ + (3 * S - 1 if S else 0) + 5 * NL + 2 * NS) + FQ + 1 + P)


def proof_len(cs, N: int = 1, scheme: int = GWC, transcript: int = EVM) -> int:
    points, scalars = counts(cs, N, scheme)
    return READER[transcript].point_bytes * points + 32 * scalars


# ---------------------------------------------------------------------------------------------------- the key, group work
class Vk:
    """What the verifier holds of the key: the circuit (harness ConstraintSystem), the fixed and sigma commitments
    (commit_lagrange of the key's columns, by the oracle's MSM), g[0], [1]_2, [s]_2 and the transcript's vk scalar."""

    def __init__(self, cs, params, fixed_values, sigma_values, vk_repr):
        self.cs = cs
        self.params = params
        gl = params.g_lagrange_np()
        self.fixed_c = [orc.msm(col, gl, threads=16) for col in np.asarray(fixed_values)]
        self.sigma_c = [orc.msm(col, gl, threads=16) for col in np.asarray(sigma_values)]
        g0 = np.zeros(12, np.uint64)
        first = np.ascontiguousarray(params.g_np()[0])
        orc.load().orc_g1_from_affine(_p(g0), _p(first))
        self.g0 = g0
        self.vk_repr = orc.fr_to_int(vk_repr)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _mul(p, k: int):
    out, kk = np.zeros(12, np.uint64), orc.fr_from_int(k % R)  # (kk: the address must outlive the call)
    orc.load().orc_g1_mul(_p(out), _p(p), _p(kk))
    return out


def _add(p, q):
    return orc.g1_add(p, q)


def _identity():
    out = np.zeros(12, np.uint64)
    orc.load().orc_g1_identity(_p(out))
    return out


def _point(pt):
    """affine integers -> Jacobian (x, y, 1) in the oracle's Montgomery limbs; None stays None"""
    if pt is None:
        return None
    L = orc.load()
    aff = np.zeros(8, np.uint64)
    for off, v in ((0, pt[0]), (4, pt[1])):
        raw = np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        limbs = np.zeros(4, np.uint64)
        L.orc_fq_from_raw(_p(limbs), _p(raw))
        aff[off:off + 4] = limbs
    out = np.zeros(12, np.uint64)
    L.orc_g1_from_affine(_p(out), _p(aff))
    return out


def affine(pt) -> np.ndarray:
    """a commitment as read (or an oracle MSM result) -> uint64[8] affine Montgomery limbs"""
    out = np.zeros(8, np.uint64)
    src = np.ascontiguousarray(pt, dtype=np.uint64)
    orc.load().orc_g1_to_affine(_p(out), _p(src))
    return out


def _pairing(vk, left, right) -> bool:
    """e(left, [s]_2) = e(right, [1]_2)"""
    L = orc.load()
    neg = np.zeros(12, np.uint64)
    L.orc_g1_neg(_p(neg), _p(right))
    ps = np.zeros((2, 8), np.uint64)
    L.orc_g1_to_affine(_p(ps[0]), _p(left))
    L.orc_g1_to_affine(_p(ps[1]), _p(neg))
    g2s = np.array([list(vk.params.s_g2), list(vk.params.g2)], dtype=np.uint64)
    return bool(L.orc_pairing_check(_p(ps), _p(g2s), ctypes.c_size_t(2)))


def _ints(instance) -> list:
    """uint64[n_instance, len, 4] Montgomery limbs -> columns of canonical integers"""
    a = np.ascontiguousarray(instance, dtype=np.uint64)
    if a.ndim != 3 or a.shape[0] == 0:
        return []
    return [[orc.fr_to_int(a[c, i]) for i in range(a.shape[1])] for c in range(a.shape[0])]


# ---------------------------------------------------------------------------------------------------- reading a proof
class Result:
    def __init__(self):
        self.verdict = -1
        self.challenges = {}   # index -> int
        self.advice = {}       # (phase, circuit, column) -> the commitment as read (oracle Jacobian limbs)
        self.order = []        # (phase, circuit, column) in the order read
        self.shuffle_z = []    # [circuit][shuffle] -> the commitment as read
        self.named = {}        # theta, beta, gamma, y, x
        self.evals = {}        # (circuit, "sh", j, e) -> int: the shuffle evaluations
        self.reader = None     # the transcript behind the evaluations
        self.queries = None    # [(point, key, commitment, evaluation)] in create_proof's order; None: malformed


def replay(vk, instances, proof: bytes, advice_phase=None, challenge_phase=None, transcript=EVM) -> Result:
    """instances: one uint64[n_instance, len, 4] array per circuit of the proof, in the prover's order."""
    res = Result()
    cs, N = vk.cs, len(instances)
    shuffles = shuffles_of(cs)
    NS = len(shuffles)
    k, n = cs.k, 1 << cs.k
    A, NL, S, P = cs.n_advice, len(cs.lookups), n_sets(cs), len(cs.perm_columns)
    d, bf = cs.degree(), cs.blinding_factors()
    chunk, qpd = d - 2, d - 1
    w = omega_for(k)
    w_inv = pow(w, R - 2, R)
    inst = [_ints(i) for i in instances]

    def rot(x, r):
        return x * pow(w if r >= 0 else w_inv, abs(r), R) % R

    t = res.reader = READER[transcript](proof)

    def point():
        return _point(t.point())

    # 1. the key, then every circuit's instance values
    t.common_scalar(vk.vk_repr)
    for c in range(N):
        for col in inst[c]:
            for v in col:
                t.common_scalar(v)
    # 2. the phases: commitments, then the phase's challenges; theta
    adv_c = [[None] * A for _ in range(N)]
    chal = res.challenges
    for ph, (cols, squeezed) in enumerate(phases_of(cs, advice_phase, challenge_phase)):
        for c in range(N):
            for col in cols:
                adv_c[c][col] = point()
                res.advice[ph, c, col] = adv_c[c][col]
                res.order.append((ph, c, col))
        for j in squeezed:
            chal[j] = t.squeeze()
    theta = t.squeeze()
    # 3 - 6. the other commitments
    pin_c, ptab_c = [[None] * NL for _ in range(N)], [[None] * NL for _ in range(N)]
    for c in range(N):
        for l in range(NL):
            pin_c[c][l] = point()
            ptab_c[c][l] = point()
    beta = t.squeeze()
    gamma = t.squeeze()
    pz_c = [[point() for _ in range(S)] for _ in range(N)]
    lz_c = [[point() for _ in range(NL)] for _ in range(N)]
    sz_c = [[point() for _ in range(NS)] for _ in range(N)]
    res.shuffle_z = sz_c
    random_c = point()
    y = t.squeeze()
    h_c = [point() for _ in range(qpd)]
    x = t.squeeze()
    res.named = {"theta": theta, "beta": beta, "gamma": gamma, "y": y, "x": x}
    xn = pow(x, n, R)
    # 7. evaluations
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
    for c in range(N):
        for j in range(NS):
            for e in range(2):
                ev[c, "sh", j, e] = t.scalar()
    if t.bad:
        return res
    res.evals = {key: v for key, v in ev.items() if key[1] == "sh"}

    # l_0, l_last, l_blind, l_active at x
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

    # expected h(x): ONE Horner value in y through circuit 0's terms, then circuit 1's, ...
    acc = 0
    for c in range(N):
        def cell(qi, c=c):
            kind, col, r = cs.queries[qi]
            if kind == ADVICE:
                return ev[c, "adv", cs.advice_queries.index((col, r))]
            if kind == FIXED:
                return fix_e[cs.fixed_queries.index((col, r))]
            if kind == CHALLENGE:
                return chal[col]
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
        for j, (ins, shs) in enumerate(shuffles):
            ai = si = 0
            for e_in, e_sh in zip(ins, shs):
                ai = (ai * theta + e_in.eval(cell)) % R
                si = (si * theta + e_sh.eval(cell)) % R
            zj, zn = ev[c, "sh", j, 0], ev[c, "sh", j, 1]
            terms.append((1 - zj) * l0)
            terms.append((zj * zj - zj) * llast)
            terms.append((zn * (si + gamma) - zj * (ai + gamma)) % R * lactive)
        for term in terms:
            acc = (acc * y + term) % R
    expected_h = acc * pow((xn - 1) % R, R - 2, R) % R

    h_commit = _identity()
    for i in reversed(range(qpd)):
        h_commit = _add(_mul(h_commit, xn), h_c[i])

    # 8. the queries: circuit after circuit its own, then what the circuits share
    qs = res.queries = []
    for c in range(N):
        com = {"adv": adv_c[c], "pz": pz_c[c], "lz": lz_c[c], "pin": pin_c[c], "ptab": ptab_c[c], "sz": sz_c[c]}
        for r, fam, idx, key in circuit_queries(cs):
            qs.append((rot(x, r % n), (c, fam, idx), com[fam][idx], ev[(c,) + key]))
    for i, (col, r) in enumerate(cs.fixed_queries):
        qs.append((rot(x, r % n), ("fixed", col), vk.fixed_c[col], fix_e[i]))
    for pc in range(P):
        qs.append((x, ("sigma", pc), vk.sigma_c[pc], sig_e[pc]))
    qs.append((x, ("h",), h_commit, expected_h))
    qs.append((x, ("random",), random_c, random_e))
    return res


def verify(vk, instances, proof: bytes, advice_phase=None, challenge_phase=None, transcript=EVM, scheme=GWC) -> Result:
    """replay, then the scheme's tail: its points read behind the evaluations (a failure there is malformed too), the
    pairing, and nothing left in the stream."""
    res = replay(vk, instances, proof, advice_phase, challenge_phase, transcript)
    t, qs = res.reader, res.queries
    if qs is None:
        return res
    if scheme == SHPLONK:
        y = t.squeeze()
        v = t.squeeze()
        h1 = _point(t.point())
        if t.bad:
            return res
        u = t.squeeze()
        h2 = _point(t.point())
        if t.bad:
            return res
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
        ok = _pairing(vk, h2, rb)
    else:  # GWC: one W per point, the points in first-appearance order
        v = t.squeeze()
        ws, rs = [], []
        for z in dict.fromkeys(q[0] for q in qs):
            cb, eb = _identity(), 0
            for q in qs:
                if q[0] == z:
                    cb = _add(_mul(cb, v), q[2])
                    eb = (eb * v + q[3]) % R
            wj = _point(t.point())
            if t.bad:
                return res
            ws.append(wj)
            rs.append(_add(_mul(wj, z), _add(cb, _mul(vk.g0, (-eb) % R))))  # z W + C - e G
        u = t.squeeze()
        wsum, rsum = _identity(), _identity()
        for i in reversed(range(len(ws))):  # Horner in u
            wsum = _add(_mul(wsum, u), ws[i])
            rsum = _add(_mul(rsum, u), rs[i])
        ok = _pairing(vk, wsum, rsum)
    res.verdict = 1 if ok and t.pos == len(t.data) else 0
    return res


# ---------------------------------------------------------------------------------------------------- SHPLONK's sets
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


def _z(T, points, u: int) -> int:
    """prod over T minus `points` of (u - r)"""
    acc = 1
    for r in T:
        if r not in points:
            acc = acc * (u - r) % R
    return acc


def _set_scalars(sets, T, evals, y: int, v: int, u: int):
    """per rotation set v^i z'_i (z'_0 = 1, z'_i = z_i / z_0, z_i = prod over T minus S_i of (u - r)), the sum
    r = sum_i v^i z'_i sum_j y^j R_ij(u), and Z_0 = prod over S_0 of (u - r)"""
    z0_inv = _inv(_z(T, sets[0][0], u))
    weights, rsum = [], 0
    for i, (points, keys) in enumerate(sets):
        wi = pow(v, i, R) * (_z(T, points, u) * z0_inv % R if i else 1) % R
        weights.append(wi)
        for j, key in enumerate(keys):
            rsum = (rsum + wi * pow(y, j, R) % R * _lagrange_at(points, [evals[key, p] for p in points], u)) % R
    return weights, rsum, _z(sets[0][0], [], u)


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


def _one_column(be, low: list):
    """a column of the backend with the given low coefficients"""
    col = np.zeros((1, be.n, 4), np.uint64)
    col[0, :len(low)] = np.stack([orc.fr_from_int(c) for c in low])
    return be.cols(col)[0]


def create_proof(be, vk, advice, instance, scheme=GWC, transcript=EVM) -> bytes:
    """One circuit, one phase, no shuffle.  vk: the Vk of the key `be` was made for (its commitments are not used: under
    SHPLONK the proof's prefix is read back only for the transcript's state, the points and the evaluations)."""
    cs = vk.cs
    rec = _Recorder(be)
    gwc = arith_level.create_proof(rec, cs, orc.fr_from_int(vk.vk_repr), advice, instance, writer=WRITER[transcript])
    if scheme == GWC:
        return gwc
    res = replay(vk, [instance], gwc[:len(gwc) - READER[transcript].point_bytes * n_point_sets(cs)], transcript=transcript)
    qs = res.queries
    assert qs is not None and res.reader.pos == len(res.reader.data)
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
    tr = res.reader.writer(be.keccak)

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
    terms, coeffs, const = [], [], 0
    for i, (points, keys) in enumerate(sets):
        wi = pow(v, i, R) * _z(T, points, u) % R
        for j, key in enumerate(keys):
            c = wi * pow(y, j, R) % R
            terms.append(poly[key])
            coeffs.append(c)
            const = (const + c * _lagrange_at(points, [evals[key, p] for p in points], u)) % R
    be.lincomb(terms + [h1], coeffs + [(-_z(T, [], u)) % R], const, work[0])
    be.kate(work[0], u, work[1])
    h2 = be.zeros(1)[0]
    be.lincomb([work[1]], [_inv(_z(T, sets[0][0], u))], None, h2)
    tr.write_point(be.commit(h2[None], False)[0])
    return bytes(tr.out)


# ---------------------------------------------------------------------------------------------- the prover's intermediates
def shuffle_product(cs, j, cell_at, theta, gamma):
    """z of shuffle j on the rows 0 .. usable from the witness: cell_at(row) -> (query index -> int)"""
    ins, shs = shuffles_of(cs)[j]
    usable = cs.usable_rows()
    z = [1]
    for r in range(usable):
        f = cell_at(r)
        ai = si = 0
        for e_in, e_sh in zip(ins, shs):
            ai = (ai * theta + e_in.eval(f)) % R
            si = (si * theta + e_sh.eval(f)) % R
        z.append(z[-1] * (ai + gamma) % R * pow((si + gamma) % R, R - 2, R) % R)
    return z
