"""Test circuits with advice phases and challenges (create_proof's FirstPhase / SecondPhase / ThirdPhase schedule,
Expression::Challenge), on a thin extension of the harness ConstraintSystem: a challenge is one more query kind and
every advice column has a phase.  harness/circuit.py itself is untouched, so every existing circuit flattens as before.

A witness that depends on a challenge cannot be an array made ahead of time: each circuit comes as a `Phased` object
whose witness(phase, challenges, variant) returns the columns of that phase, given the challenges squeezed so far."""
import random

import numpy as np

from circuit import ADVICE, FIXED, INSTANCE, R, Assignment, ConstraintSystem, Expr, to_mont_array

CHALLENGE = 3


class PhasedCS(ConstraintSystem):
    """ConstraintSystem with Expression::Challenge: query kind 3, column = the challenge's index, rotation 0, degree 0."""

    def q(self, kind, column, rotation=0):
        if kind != CHALLENGE:
            return super().q(kind, column, rotation)
        key = (CHALLENGE, column, 0)
        if key not in self.queries:
            self.queries.append(key)
        return Expr({(self.queries.index(key),): 1})

    def challenge(self, j: int) -> Expr:
        return self.q(CHALLENGE, j)

    def expr_degree(self, e: Expr) -> int:
        return max((sum(1 for qi in key if self.queries[qi][0] != CHALLENGE) for key in e.terms), default=0)

    def degree(self) -> int:  # ConstraintSystem::degree, a challenge counting 0
        d = 3 if self.perm_columns else 1
        for ins, tabs in self.lookups:
            ind = max([1] + [self.expr_degree(e) for e in ins])
            td = max([1] + [self.expr_degree(e) for e in tabs])
            d = max(d, 4, 2 + ind + td)
        for g in self.gates:
            d = max(d, self.expr_degree(g))
        return d


def inv(x: int) -> int:
    return pow(x % R, R - 2, R)


class Phased:
    """cs + key columns + phases + the witness as a function of the challenges."""

    def __init__(self, name, cs, asg, advice_phase, challenge_phase, ilen, witness, instance=None):
        self.name, self.cs, self.asg, self.ilen = name, cs, asg, ilen
        self.advice_phase, self.challenge_phase = list(advice_phase), list(challenge_phase)
        self.n_phases = max(self.advice_phase + [0]) + 1
        self._witness, self._instance = witness, instance
        self.n, self.usable = 1 << cs.k, cs.usable_rows()

    def fixed_values(self):
        return self.asg.fixed_values()

    def sigma_values(self):
        return self.asg.sigma_values()

    def instance(self, variant: int = 0) -> np.ndarray:
        """uint64[n_instance, ilen, 4]"""
        if not self.cs.n_instance:
            return np.zeros((0, 0, 4), np.uint64)
        return np.stack([to_mont_array(col) for col in self._instance(variant)])

    def witness(self, phase: int, challenges, variant: int = 0) -> dict:
        """{advice column: n canonical integers} for the columns of `phase`; challenges: ints, as squeezed so far"""
        cols = self._witness(phase, list(challenges), variant)
        assert sorted(cols) == [c for c, ph in enumerate(self.advice_phase) if ph == phase], (phase, sorted(cols))
        return cols

    def synthesize(self, variants, seen=None):
        """The callback of Prover.prove_phased for a batch whose proof b has witness variant variants[b]; `seen`, a list,
        receives (phase, challenges as ints [count][n_challenges]) per call."""
        import orc

        def fn(phase, ch):
            ints = [[orc.fr_to_int(ch[b, j]) for j in range(ch.shape[1])] for b in range(ch.shape[0])]
            if seen is not None:
                seen.append((phase, ints))
            return [{c: to_mont_array(v) for c, v in self.witness(phase, ints[b], variants[b]).items()} for b in range(ch.shape[0])]

        return fn

    def full_advice(self, challenges, variant: int = 0) -> np.ndarray:
        """every phase's columns for given challenges: uint64[n_advice, n, 4] (for the plain entries: one phase)"""
        cols = {}
        for ph in range(self.n_phases):
            cols.update(self.witness(ph, challenges, variant))
        return np.stack([to_mont_array(cols[c]) for c in range(self.cs.n_advice)])


def _key(cs, fixed_cols, copies=()):
    """fixed columns and the permutation of a circuit whose advice is not known yet: copies between zero cells"""
    asg = Assignment(cs)
    for c, col in fixed_cols.items():
        for r, v in enumerate(col):
            asg.set(FIXED, c, r, v)
    for a, b in copies:
        asg.copy(a, b)
    return asg


def rlc(k: int = 5, high_gate: bool = False, constant=None) -> Phased:
    """Phase-0 columns a, b; challenge c behind phase 0; phase-1 column acc with q (acc(w) - acc c - a): a running random
    linear combination.  The instance is hashed before c exists, so the public cell is the one accumulated value that
    does not depend on c: acc[1] = a[0] (acc[0] = 0), copied to instance row 0.  high_gate (the k = 14 case): a degree-6
    restatement of the gate, q a^4 (acc(w) - acc c - a), beside the low one -- both read the challenge.
    constant: the same circuit with the challenge replaced by that constant and every column in one phase."""
    cs = PhasedCS(k)
    q = cs.fixed_column()
    a, b, acc = cs.advice_column(), cs.advice_column(), cs.advice_column()
    i0 = cs.instance_column()
    cs.enable_equality(ADVICE, acc)
    cs.enable_equality(INSTANCE, i0)
    c = cs.challenge(0) if constant is None else Expr.const(constant)
    base = cs.advice(acc, 1) - cs.advice(acc) * c - cs.advice(a)
    gates = [cs.fixed(q) * base, cs.fixed(q) * (cs.advice(b) - cs.advice(a) * cs.advice(a))]
    if high_gate:
        e = cs.fixed(q) * base
        for _ in range(4):
            e = e * cs.advice(a)
        gates.append(e)
    cs.create_gate(gates)
    n, m = 1 << k, cs.usable_rows() - 1
    asg = _key(cs, {q: [1] * m + [0] * (n - m)}, [((ADVICE, acc, 1), (INSTANCE, i0, 0))])

    def a_values(variant):
        rng = random.Random(100 + variant)
        return [rng.randrange(1 << 16) + 1 for _ in range(m)] + [0] * (n - m)

    def witness(phase, ch, variant):
        av = a_values(variant)
        if phase == 0 and constant is None:
            return {a: av, b: [x * x % R for x in av]}
        cv = ch[0] if constant is None else constant
        col = [0] * n
        for r in range(m):
            col[r + 1] = (col[r] * cv + av[r]) % R
        if constant is None:
            return {acc: col}
        return {a: av, b: [x * x % R for x in av], acc: col}

    def instance(variant):
        return [[a_values(variant)[0]]]

    return Phased("rlc", cs, asg, [0, 0, 1] if constant is None else [0, 0, 0], [0] if constant is None else [], 1, witness, instance)


def shuffle(k: int = 5) -> Phased:
    """b is a permutation of a (phase 0); phase-1 z with q (z(w) (b + c) - z (a + c)) and z = 1 on the first and last row."""
    cs = PhasedCS(k)
    q, qf, ql = cs.fixed_column(), cs.fixed_column(), cs.fixed_column()
    a, b, z = cs.advice_column(), cs.advice_column(), cs.advice_column()
    c = cs.challenge(0)
    cs.create_gate([cs.fixed(q) * (cs.advice(z, 1) * (cs.advice(b) + c) - cs.advice(z) * (cs.advice(a) + c)),
                    cs.fixed(qf) * (cs.advice(z) - 1), cs.fixed(ql) * (cs.advice(z) - 1)])
    n, m = 1 << k, cs.usable_rows() - 1
    asg = _key(cs, {q: [1] * m + [0] * (n - m), qf: [1] + [0] * (n - 1), ql: [0] * m + [1] + [0] * (n - m - 1)})

    def ab(variant):
        rng = random.Random(200 + variant)
        av = [rng.randrange(1 << 20) for _ in range(m)]
        bv = list(av)
        rng.shuffle(bv)
        return av + [0] * (n - m), bv + [0] * (n - m)

    def witness(phase, ch, variant):
        av, bv = ab(variant)
        if phase == 0:
            return {a: av, b: bv}
        col = [0] * n
        col[0] = 1
        for r in range(m):
            col[r + 1] = col[r] * (av[r] + ch[0]) % R * inv(bv[r] + ch[0]) % R
        assert col[m] == 1
        return {z: col}

    return Phased("shuffle", cs, asg, [0, 0, 1], [0], 0, witness)


def interleaved(k: int = 5) -> Phased:
    """Advice columns 0 and 2 in phase 1, column 1 in phase 0: the commitment order (1 | 0, 2) differs from the column
    order.  Queries at rotations -1, 0, 1: s = u(w^-1) + c and t = s(w) u on the rows where q is set."""
    cs = PhasedCS(k)
    q = cs.fixed_column()
    s, u, t = cs.advice_column(), cs.advice_column(), cs.advice_column()
    c = cs.challenge(0)
    cs.create_gate([cs.fixed(q) * (cs.advice(s) - cs.advice(u, -1) - c),
                    cs.fixed(q) * (cs.advice(t) - cs.advice(s, 1) * cs.advice(u))])
    n, m = 1 << k, cs.usable_rows() - 1
    asg = _key(cs, {q: [0] + [1] * (m - 1) + [0] * (n - m)})

    def uv(variant):
        rng = random.Random(300 + variant)
        return [rng.randrange(1 << 30) for _ in range(m + 1)] + [0] * (n - m - 1)

    def witness(phase, ch, variant):
        u_ = uv(variant)
        if phase == 0:
            return {u: u_}
        s_ = [0] * n
        for r in range(1, m + 1):
            s_[r] = (u_[r - 1] + ch[0]) % R
        t_ = [0] * n
        for r in range(1, m):
            t_[r] = s_[r + 1] * u_[r] % R
        return {s: s_, t: t_}

    return Phased("interleaved", cs, asg, [1, 0, 1], [0], 0, witness)


def three_phase(k: int = 5) -> Phased:
    """Phases 0, 1, 2; challenges 0 and 1 behind phase 0, 2 behind phase 1, 3 behind phase 2 and only in a gate.  A width-2
    lookup with a challenge in an input expression and in a table expression: (q a, q a c0) in {(t, t c0)}.  d = a c0 + c1
    (phase 1), e = d c2 (phase 2), c3 q (e - d c2); a[0] is public."""
    cs = PhasedCS(k)
    q, tab = cs.fixed_column(), cs.fixed_column()
    a, d, e = cs.advice_column(), cs.advice_column(), cs.advice_column()
    i0 = cs.instance_column()
    cs.enable_equality(ADVICE, a)
    cs.enable_equality(INSTANCE, i0)
    c0, c1, c2, c3 = (cs.challenge(j) for j in range(4))
    qe = cs.fixed(q)
    cs.create_gate([qe * (cs.advice(d) - cs.advice(a) * c0 - c1), qe * (cs.advice(e) - cs.advice(d) * c2),
                    c3 * qe * (cs.advice(e) - cs.advice(d) * c2)])
    cs.lookup([qe * cs.advice(a), qe * cs.advice(a) * c0], [cs.fixed(tab), cs.fixed(tab) * c0])
    n, usable = 1 << k, cs.usable_rows()
    m = usable - 1
    asg = _key(cs, {q: [1] * m + [0] * (n - m), tab: [r % 8 for r in range(usable)] + [0] * (n - usable)},
               [((ADVICE, a, 0), (INSTANCE, i0, 0))])

    def av(variant):
        rng = random.Random(400 + variant)
        return [rng.randrange(8) for _ in range(m)] + [0] * (n - m)

    def witness(phase, ch, variant):
        a_ = av(variant)
        if phase == 0:
            return {a: a_}
        d_ = [(a_[r] * ch[0] + ch[1]) % R if r < m else 0 for r in range(n)]
        if phase == 1:
            return {d: d_}
        return {e: [d_[r] * ch[2] % R for r in range(n)]}

    return Phased("three_phase", cs, asg, [0, 1, 2], [0, 0, 1, 2], 1, witness, lambda variant: [[av(variant)[0]]])


def gates_only_challenge(k: int = 5) -> Phased:
    """All advice in phase 0, a challenge in a gate: c0 q (a0^2 - a1).  No lookup, no permutation, no instance -- the plain
    zg_prover_prove proves it, the witness cannot depend on the challenge."""
    cs = PhasedCS(k)
    q = cs.fixed_column()
    a0, a1 = cs.advice_column(), cs.advice_column()
    cs.create_gate([cs.challenge(0) * cs.fixed(q) * (cs.advice(a0) * cs.advice(a0) - cs.advice(a1))])
    n, m = 1 << k, cs.usable_rows() - 1
    asg = _key(cs, {q: [1] * m + [0] * (n - m)})

    def witness(phase, ch, variant):
        rng = random.Random(500 + variant)
        v = [rng.randrange(1 << 20) for _ in range(m)] + [0] * (n - m)
        return {a0: v, a1: [x * x % R for x in v]}

    return Phased("gates_only_challenge", cs, asg, [0, 0], [0], 0, witness)


SMALL = {"rlc": rlc, "shuffle": shuffle, "interleaved": interleaved, "three_phase": three_phase,
         "gates_only_challenge": gates_only_challenge}


def rlc_k14() -> Phased:
    """rlc at k = 14 with cs_degree 6: the split 4n + n domain and the quotient's terms by degree are active, with one low
    gate and one high gate that both read the challenge."""
    p = rlc(14, high_gate=True)
    assert p.cs.degree() == 6
    return p
