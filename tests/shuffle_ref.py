"""The comparator of the shuffle tests: `verify_proof` with halo2's shuffle argument (privacy-scaling-explorations/halo2
v0.3.0 on: src/plonk/shuffle/verifier.rs beside src/plonk/verifier.rs; KZG, QUERY_INSTANCE = false) restated on Python
integers -- nothing of the library under test.  It extends tests/phases_ref.py, whose walk it keeps, by what a circuit's
shuffles add (cs.shuffles: [(inputs [Expr], shuffles [Expr])], tests/shuffle_circuits.py):

  transcript    each circuit's shuffle products z_j are read behind every circuit's lookup products and before the random
                polynomial's commitment
  evaluations   z_j(x), z_j(wx) per shuffle and circuit, behind every circuit's lookup evaluations
  h(x)          behind a circuit's lookup terms, per shuffle: l_0 (1 - z), l_last (z^2 - z),
                (1 - (l_last + l_blind)) (z(wx) (s + gamma) - z (a + gamma)), a and s the theta-folds of the two tuples
  queries       (z_j, x), (z_j, wx) behind the circuit's lookup queries
  lengths       NS points and 2 NS scalars more per circuit, under either multi-open argument

On a circuit without shuffles it is phases_ref.verify, statement for statement.

verify(...) -> Result: phases_ref's, and the shuffle commitments as read (shuffle_z[circuit][j]) and the challenges theta,
beta, gamma, y, x (named)."""
import ctypes

import numpy as np

import blake2b_ref
import multi_ref
import orc
import phases_ref
import shplonk_ref
from circuit import ADVICE, DELTA, FIXED, INSTANCE, R, omega_for
from multi_ref import _add, _identity, _ints, _mul, _p, n_sets
from phases_ref import BLAKE2B, CHALLENGE, EVM, GWC, SHPLONK, phases_of

Vk = multi_ref.Vk


def shuffles_of(cs):
    return list(getattr(cs, "shuffles", []))


def circuit_queries(cs):
    """One circuit's own opening queries in create_proof's order: multi_ref.circuit_queries, then the shuffles'."""
    out = multi_ref.circuit_queries(cs)
    for j in range(len(shuffles_of(cs))):
        out += [(0, "sz", j, ("sh", j, 0)), (1, "sz", j, ("sh", j, 1))]
    return out


def n_point_sets(cs) -> int:
    rots = [q[0] for q in circuit_queries(cs)] + [rot for _, rot in cs.fixed_queries] + [0]
    return len(set(r % (1 << cs.k) for r in rots))


def counts(cs, N: int, scheme: int):
    """(points, scalars) of a proof of N circuits"""
    NS = len(shuffles_of(cs))
    A, NL, S, P, d = cs.n_advice, len(cs.lookups), n_sets(cs), len(cs.perm_columns), cs.degree()
    AQ, FQ = len(cs.advice_queries), len(cs.fixed_queries)
    tail = 2 if scheme == SHPLONK else n_point_sets(cs)
    return (N * (A + 3 * NL + S + NS) + 1 + (d - 1) + tail, N * (AQ + (3 * S - 1 if S else 0) + 5 * NL + 2 * NS) + FQ + 1 + P)


def proof_len(cs, scheme=GWC, transcript=EVM, N=1) -> int:
    points, scalars = counts(cs, N, scheme)
    return 32 * (points + scalars) if transcript == BLAKE2B else 64 * points + 32 * scalars


class Result(phases_ref.Result):
    def __init__(self):
        super().__init__()
        self.shuffle_z = []  # [circuit][shuffle] -> the commitment as read
        self.named = {}      # theta, beta, gamma, y, x
        self.evals = {}      # (circuit, "sh", j, e) -> int


def verify(vk, instances, proof: bytes, advice_phase=None, challenge_phase=None, scheme=GWC, transcript=EVM) -> Result:
    """instances: one uint64[n_instance, len, 4] array per circuit of the proof."""
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

    t = (blake2b_ref._Reader if transcript == BLAKE2B else multi_ref._Reader)(proof)
    t.common_scalar(vk.vk_repr)
    for c in range(N):
        for col in inst[c]:
            for v in col:
                t.common_scalar(v)
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
    sz_c = [[t.point() for _ in range(NS)] for _ in range(N)]
    res.shuffle_z = sz_c
    random_c = t.point()
    y = t.squeeze()
    h_c = [t.point() for _ in range(qpd)]
    x = t.squeeze()
    res.named = {"theta": theta, "beta": beta, "gamma": gamma, "y": y, "x": x}
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
    for c in range(N):
        for j in range(NS):
            for e in range(2):
                ev[c, "sh", j, e] = t.scalar()
    if t.bad:
        return res
    res.evals = {key: v for key, v in ev.items() if key[1] == "sh"}

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

    qs = []
    for c in range(N):
        com = {"adv": adv_c[c], "pz": pz_c[c], "lz": lz_c[c], "pin": pin_c[c], "ptab": ptab_c[c], "sz": sz_c[c]}
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


affine = phases_ref.affine


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
