"""The comparator of the multi-circuit proof tests: `verify_proof` for a proof of N instances of one circuit, restated
on Python integers -- nothing of the library under test.

halo2_proofs v2023_04_20 `verify_proof` (KZG, GWC, EvmTranscript; one phase, QUERY_INSTANCE = false) takes
`instances: &[&[&[F]]]`: every instance of the circuit behind ONE transcript.  The order read here is the contract of
DESIGN.md section 11; oracle/prover.c's orc_verify_proof_pairing is its N = 1 case, and tests/test_multi_host.py holds this
file against it there.

  transcript      orc.keccak256 and the EvmTranscript rules of oracle/prover.c (tr_common_scalar .. tr_squeeze)
  expressions     Expr.eval of harness/circuit.py on the proof's evaluations
  instance evals  the Lagrange form, (x^n - 1)/n * sum_i inst_i w^i / (x w^rot - w^i)
  group work      the oracle's primitives through orc.load(): orc_g1_mul, orc_g1_add, orc_pairing_check

verify(vk, instances, proof) -> 1 accepted, 0 rejected, -1 malformed (the verdict classes of zg_verifier_verify_*).
"""
import ctypes

import numpy as np

import orc
from circuit import ADVICE, DELTA, FIXED, INSTANCE, R, omega_for

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def n_sets(cs) -> int:
    P, chunk = len(cs.perm_columns), cs.degree() - 2
    return (P + chunk - 1) // chunk if P else 0


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
    return out


def n_point_sets(cs) -> int:
    rots = [q[0] for q in circuit_queries(cs)] + [rot for _, rot in cs.fixed_queries] + [0]
    return len(set(r % (1 << cs.k) for r in rots))


def point_set_lengths(cs, N: int) -> dict:
    """{rotation mod n: how many (circuit, polynomial) pairs a proof of N circuits opens at x * omega^rotation}: the lists
    that step 8 of verify walks -- every circuit's own queries, then the fixed columns, the sigmas, h and the random
    polynomial at rotation 0."""
    n, out = 1 << cs.k, {}
    for r, *_ in circuit_queries(cs):
        out[r % n] = out.get(r % n, 0) + N
    for _, r in cs.fixed_queries:
        out[r % n] = out.get(r % n, 0) + 1
    out[0] = out.get(0, 0) + len(cs.perm_columns) + 2
    return out


def proof_len(cs, N: int) -> int:
    """64 (N (A + 3 NL + S) + 1 + (d - 1) + nsets) + 32 (N (AQ + (S ? 3 S - 1 : 0) + 5 NL) + FQ + 1 + P)"""
    A, NL, S, P, d = cs.n_advice, len(cs.lookups), n_sets(cs), len(cs.perm_columns), cs.degree()
    AQ, FQ = len(cs.advice_queries), len(cs.fixed_queries)
    return (64 * (N * (A + 3 * NL + S) + 1 + (d - 1) + n_point_sets(cs))
            + 32 * (N * (AQ + (3 * S - 1 if S else 0) + 5 * NL) + FQ + 1 + P))


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


def _fr(x: int) -> np.ndarray:
    return orc.fr_from_int(x % R)


def _mul(p, k: int):
    out, kk = np.zeros(12, np.uint64), _fr(k)  # (kk: the address must outlive the call)
    orc.load().orc_g1_mul(_p(out), _p(p), _p(kk))
    return out


def _add(p, q):
    return orc.g1_add(p, q)


def _identity():
    out = np.zeros(12, np.uint64)
    orc.load().orc_g1_identity(_p(out))
    return out


def _point(x: int, y: int):
    """Jacobian (x, y, 1) in the oracle's Montgomery limbs."""
    L = orc.load()
    aff = np.zeros(8, np.uint64)
    for off, v in ((0, x), (4, y)):
        raw = np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        limbs = np.zeros(4, np.uint64)
        L.orc_fq_from_raw(_p(limbs), _p(raw))
        aff[off:off + 4] = limbs
    out = np.zeros(12, np.uint64)
    L.orc_g1_from_affine(_p(out), _p(aff))
    return out


class _Reader:
    """EvmTranscript in read mode: the pending hash input, the proof stream, the first failure."""

    def __init__(self, proof: bytes):
        self.buf, self.data, self.pos, self.bad = b"", bytes(proof), 0, False

    def common_scalar(self, v: int):
        self.buf += (v % R).to_bytes(32, "big")

    def point(self):
        if self.pos + 64 > len(self.data):
            self.bad = True
            return None
        b = self.data[self.pos:self.pos + 64]
        self.pos += 64
        x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
        if x >= Q or y >= Q or (y * y - x * x * x - 3) % Q != 0:  # canonical coordinates, on the curve ((0, 0) is not)
            self.bad = True
            return None
        self.buf += b
        return _point(x, y)

    def scalar(self):
        if self.pos + 32 > len(self.data):
            self.bad = True
            return 0
        v = int.from_bytes(self.data[self.pos:self.pos + 32], "big")
        self.pos += 32
        if v >= R:
            self.bad = True
            return 0
        self.buf += v.to_bytes(32, "big")
        return v

    def squeeze(self) -> int:
        h = orc.keccak256(self.buf + (b"\x01" if len(self.buf) == 32 else b""))
        self.buf = h
        return int.from_bytes(h, "big") % R


def _ints(instance) -> list:
    """uint64[n_instance, len, 4] Montgomery limbs -> columns of canonical integers"""
    a = np.ascontiguousarray(instance, dtype=np.uint64)
    if a.ndim != 3 or a.shape[0] == 0:
        return []
    return [[orc.fr_to_int(a[c, i]) for i in range(a.shape[1])] for c in range(a.shape[0])]


def verify(vk: Vk, instances, proof: bytes) -> int:
    """instances: one uint64[n_instance, len, 4] array per circuit of the proof, in the prover's order."""
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
    # 1. the key, then every circuit's instance values
    t.common_scalar(vk.vk_repr)
    for c in range(N):
        for col in inst[c]:
            for v in col:
                t.common_scalar(v)
    # 2 - 6. commitments
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
    if t.bad:
        return -1

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

    # 8. the queries: circuit after circuit its own, then what the circuits share
    qs = []  # (rotation mod n, commitment, evaluation)
    for c in range(N):
        com = {"adv": adv_c[c], "pz": pz_c[c], "lz": lz_c[c], "pin": pin_c[c], "ptab": ptab_c[c]}
        for r, fam, idx, key in circuit_queries(cs):
            qs.append((r % n, com[fam][idx], ev[(c,) + key]))
    for i, (col, r) in enumerate(cs.fixed_queries):
        qs.append((r % n, vk.fixed_c[col], fix_e[i]))
    for pc in range(P):
        qs.append((0, vk.sigma_c[pc], sig_e[pc]))
    qs.append((0, h_commit, expected_h))
    qs.append((0, random_c, random_e))

    v = t.squeeze()
    done = [False] * len(qs)
    ws, rs = [], []
    for first in range(len(qs)):
        if done[first]:
            continue
        r0 = qs[first][0]
        cb, eb = _identity(), 0
        for j in range(first, len(qs)):
            if done[j] or qs[j][0] != r0:
                continue
            done[j] = True
            cb = _add(_mul(cb, v), qs[j][1])
            eb = (eb * v + qs[j][2]) % R
        wj = t.point()
        if t.bad:
            return -1
        z = x * pow(w, r0, R) % R
        ws.append(wj)
        rs.append(_add(_mul(wj, z), _add(cb, _mul(vk.g0, (-eb) % R))))  # z W + C - e G
    u = t.squeeze()
    wsum, rsum = _identity(), _identity()
    for i in reversed(range(len(ws))):  # Horner in u
        wsum = _add(_mul(wsum, u), ws[i])
        rsum = _add(_mul(rsum, u), rs[i])
    L = orc.load()
    neg = np.zeros(12, np.uint64)
    L.orc_g1_neg(_p(neg), _p(rsum))
    ps = np.zeros((2, 8), np.uint64)
    L.orc_g1_to_affine(_p(ps[0]), _p(wsum))
    L.orc_g1_to_affine(_p(ps[1]), _p(neg))
    g2s = np.array([list(vk.params.s_g2), list(vk.params.g2)], dtype=np.uint64)
    if not L.orc_pairing_check(_p(ps), _p(g2s), ctypes.c_size_t(2)):
        return 0
    return 1 if t.pos == len(t.data) else 0
