"""The comparator of the advice-phase tests: `verify_proof` with phases and challenges (halo2_proofs v2023_04_20
src/plonk/verifier.rs; KZG, QUERY_INSTANCE = false) restated on Python integers -- nothing of the library under test.

After the vk scalar and the instances the verifier walks the phases in ascending order: it reads the commitments of the
advice columns of that phase (every circuit's, ascending column), then squeezes one scalar per challenge of that phase
(ascending index); theta follows the last phase.  Evaluations, opening queries and both multi-open tails keep the order of
tests/multi_ref.py and tests/shplonk_ref.py; Expression::Challenge(j) evaluates to challenge j.

  transcript      its own replay over a reader: multi_ref._Reader (EvmTranscript, orc.keccak256) or blake2b_ref._Reader
                  (hashlib BLAKE2b), chosen by argument -- no module attribute is swapped
  expressions     Expr.eval with the challenge values
  instance evals  the Lagrange form
  group work      the oracle's primitives, as multi_ref does

verify(...) -> Result: verdict 1 / 0 / -1, the challenges replayed and the advice commitments by (phase, column)."""
import ctypes

import numpy as np

import blake2b_ref
import multi_ref
import orc
import shplonk_ref
from circuit import ADVICE, DELTA, FIXED, INSTANCE, R, omega_for
from multi_ref import _add, _identity, _ints, _mul, _p, circuit_queries, n_sets

CHALLENGE = 3
GWC, SHPLONK = 0, 1
EVM, BLAKE2B = 0, 1
Vk = multi_ref.Vk


class Result:
    def __init__(self):
        self.verdict = -1
        self.challenges = {}   # index -> int
        self.advice = {}       # (phase, circuit, column) -> the commitment as read (oracle Jacobian limbs)
        self.order = []        # (phase, circuit, column) in the order read


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


def proof_len(cs, scheme=GWC, transcript=EVM, N=1) -> int:
    points, scalars = blake2b_ref.counts(cs, N, scheme)
    return 32 * (points + scalars) if transcript == BLAKE2B else 64 * points + 32 * scalars


def verify(vk, instances, proof: bytes, advice_phase=None, challenge_phase=None, scheme=GWC, transcript=EVM) -> Result:
    """instances: one uint64[n_instance, len, 4] array per circuit of the proof."""
    res = Result()
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

    t = (blake2b_ref._Reader if transcript == BLAKE2B else multi_ref._Reader)(proof)
    t.common_scalar(vk.vk_repr)
    for c in range(N):
        for col in inst[c]:
            for v in col:
                t.common_scalar(v)
    # the phases: commitments, then the phase's challenges
    adv_c = [[None] * A for _ in range(N)]
    chal = res.challenges
    for ph, (cols, squeezed) in enumerate(phases_of(cs, advice_phase, challenge_phase)):
        for c in range(N):
            for col in cols:
                adv_c[c][col] = t.point()
                res.advice[ph, c, col] = adv_c[c][col]
                res.order.append((ph, c, col))
        for j in squeezed:
            chal[j] = t.squeeze()
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
        return res

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
        for term in terms:
            acc = (acc * y + term) % R
    expected_h = acc * pow((xn - 1) % R, R - 2, R) % R

    h_commit = _identity()
    for i in reversed(range(qpd)):
        h_commit = _add(_mul(h_commit, xn), h_c[i])

    # the queries in create_proof's order: (rotation mod n, key, commitment, evaluation)
    qs = []
    for c in range(N):
        com = {"adv": adv_c[c], "pz": pz_c[c], "lz": lz_c[c], "pin": pin_c[c], "ptab": ptab_c[c]}
        for r, fam, idx, key in circuit_queries(cs):
            qs.append((r % n, (c, fam, idx), com[fam][idx], ev[(c,) + key]))
    for i, (col, r) in enumerate(cs.fixed_queries):
        qs.append((r % n, ("fixed", col), vk.fixed_c[col], fix_e[i]))
    for pc in range(P):
        qs.append((0, ("sigma", pc), vk.sigma_c[pc], sig_e[pc]))
    qs.append((0, ("h",), h_commit, expected_h))
    qs.append((0, ("random",), random_c, random_e))

    L = orc.load()

    def pairing(left, right):  # e(left, [s]_2) = e(right, [1]_2)
        neg = np.zeros(12, np.uint64)
        L.orc_g1_neg(_p(neg), _p(right))
        ps = np.zeros((2, 8), np.uint64)
        L.orc_g1_to_affine(_p(ps[0]), _p(left))
        L.orc_g1_to_affine(_p(ps[1]), _p(neg))
        g2s = np.array([list(vk.params.s_g2), list(vk.params.g2)], dtype=np.uint64)
        return bool(L.orc_pairing_check(_p(ps), _p(g2s), ctypes.c_size_t(2)))

    if scheme == SHPLONK:
        sy = t.squeeze()
        v = t.squeeze()
        h1 = t.point()
        if t.bad:
            return res
        u = t.squeeze()
        h2 = t.point()
        if t.bad:
            return res
        at = [(rot(x, q[0]), q[1]) for q in qs]
        sets, T = shplonk_ref.intermediate_sets(at)
        commitment = {q[1]: q[2] for q in qs}
        evals = {(q[1], p[0]): q[3] for q, p in zip(qs, at)}
        weights, rsum, Z0 = shplonk_ref._set_scalars(sets, T, evals, sy, v, u)
        rb = _identity()
        for wi, (_, keys) in zip(weights, sets):
            for j, key in enumerate(keys):
                rb = _add(rb, _mul(commitment[key], wi * pow(sy, j, R) % R))
        rb = _add(rb, _mul(vk.g0, (-rsum) % R))
        rb = _add(rb, _mul(h1, (-Z0) % R))
        rb = _add(rb, _mul(h2, u))
        ok = pairing(h2, rb)
    else:
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
                cb = _add(_mul(cb, v), qs[j][2])
                eb = (eb * v + qs[j][3]) % R
            wj = t.point()
            if t.bad:
                return res
            zpt = x * pow(w, r0, R) % R
            ws.append(wj)
            rs.append(_add(_mul(wj, zpt), _add(cb, _mul(vk.g0, (-eb) % R))))
        u = t.squeeze()
        wsum, rsum = _identity(), _identity()
        for i in reversed(range(len(ws))):
            wsum = _add(_mul(wsum, u), ws[i])
            rsum = _add(_mul(rsum, u), rs[i])
        ok = pairing(wsum, rsum)
    res.verdict = 1 if ok and t.pos == len(t.data) else 0
    return res


def affine(pt) -> np.ndarray:
    """a commitment as read (or an oracle MSM result) -> uint64[8] affine Montgomery limbs"""
    out = np.zeros(8, np.uint64)
    src = np.ascontiguousarray(pt, dtype=np.uint64)
    orc.load().orc_g1_to_affine(_p(out), _p(src))
    return out
