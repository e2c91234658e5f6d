"""Test circuits with halo2's shuffle argument (ConstraintSystem::shuffle), on a thin extension of the phased
ConstraintSystem of tests/phases_circuits.py: a circuit keeps its shuffles beside its lookups, its degree counts
max(2 + deg a, 2 + deg s) per shuffle (an expression's degree at least 1, a challenge 0), and to_c() appends the shuffle
expressions' monomials to the image's and leaves their ranges in image.shuffles, what zg.Prover / zg.Verifier take as
`shuffles`.  harness/circuit.py itself is untouched.

Every circuit comes as a phases_circuits.Phased (most of them one phase, no challenge).  Witness variant BAD is variant
0 with ONE value of a shuffle column changed: no shuffle any more."""
import random

from circuit import ADVICE, MAX_LOOKUP_WIDTH, R, ConstraintSystem, Expr
from phases_circuits import Phased, PhasedCS, _key

BAD = 99


class ShuffleCS(PhasedCS):
    def __init__(self, k, **kw):
        super().__init__(k, **kw)
        self.shuffles = []  # (inputs [Expr], shuffles [Expr])

    def shuffle(self, inputs, shuffles):
        assert 1 <= len(inputs) == len(shuffles) <= MAX_LOOKUP_WIDTH
        self.shuffles.append((list(inputs), list(shuffles)))

    def shuffle_degree(self) -> int:
        d = 0
        for ins, shs in self.shuffles:
            d = max(d, 2 + max([1] + [self.expr_degree(e) for e in ins]), 2 + max([1] + [self.expr_degree(e) for e in shs]))
        return d

    def degree(self) -> int:
        return max(super().degree(), self.shuffle_degree())

    def to_c(self):
        """the image of the circuit without its shuffles (zg_circuit knows none), the shuffle expressions flattened behind
        everything else's monomials; image.shuffles: [(inputs [(first, count)], shuffles [(first, count)])]"""
        degree, real = self.degree(), self.lookups
        # (flattened as lookups behind the real ones -- zg_shuffle has zg_lookup's layout -- and taken out of the count again)
        self.lookups = real + [(list(i), list(s)) for i, s in self.shuffles]
        try:
            img = ConstraintSystem.to_c(self)
        finally:
            self.lookups = real
        img.c.n_lookups = len(real)
        img.c.cs_degree = degree
        img.shuffles = []
        for j in range(len(self.shuffles)):
            lk = img.lookups[len(real) + j]
            img.shuffles.append(([(lk.inputs[e].first, lk.inputs[e].count) for e in range(lk.width)],
                                 [(lk.tables[e].first, lk.tables[e].count) for e in range(lk.width)]))
        return img


def _perm(rng, count):
    p = list(range(count))
    rng.shuffle(p)
    return p


def _spoil(col, variant, row=2):
    if variant == BAD:
        col[row] = (col[row] + 1) % R
    return col


def plain(k: int = 5) -> Phased:
    """one shuffle of width 1, advice against advice over all usable rows, values with repeats"""
    cs = ShuffleCS(k)
    a, b = cs.advice_column(), cs.advice_column()
    cs.shuffle([cs.advice(a)], [cs.advice(b)])
    n, u = 1 << k, cs.usable_rows()
    asg = _key(cs, {})

    def witness(phase, ch, variant):
        rng = random.Random(600 + (0 if variant == BAD else variant))
        av = [rng.randrange(8) for _ in range(u)]
        bv = [av[i] for i in _perm(rng, u)]
        return {a: av + [0] * (n - u), b: _spoil(bv, variant) + [0] * (n - u)}

    return Phased("plain", cs, asg, [0, 0], [], 0, witness)


def wide(k: int = 5, high_gate: bool = False) -> Phased:
    """width ZG_MAX_LOOKUP_WIDTH with a selector column times advice on both sides: the shuffle's degree, 4, is the
    circuit's.  high_gate (the k = 14 case): a degree-6 gate q (a0^5 - p), a low one q (a0^2 - s) and a lookup q t in tab
    (degree 5: low) beside it, so the domain is split and the quotient's terms go by degree -- the library sorts them
    only for a circuit with a permutation or a lookup."""
    W = MAX_LOOKUP_WIDTH
    cs = ShuffleCS(k)
    q = cs.fixed_column()
    ac = [cs.advice_column() for _ in range(W)]
    bc = [cs.advice_column() for _ in range(W)]
    cs.shuffle([cs.fixed(q) * cs.advice(c) for c in ac], [cs.fixed(q) * cs.advice(c) for c in bc])
    if high_gate:
        p5, sq = cs.advice_column(), cs.advice_column()
        a0 = cs.advice(ac[0])
        cs.create_gate([cs.fixed(q) * (a0 * a0 * a0 * a0 * a0 - cs.advice(p5)), cs.fixed(q) * (a0 * a0 - cs.advice(sq))])
        tab, t = cs.fixed_column(), cs.advice_column()
        cs.lookup([cs.fixed(q) * cs.advice(t)], [cs.fixed(tab)])
    assert cs.degree() == (6 if high_gate else 4)
    n, u = 1 << k, cs.usable_rows()
    m = u - 3  # (the selector leaves the last usable rows out)
    key = {q: [1] * m + [0] * (n - m)}
    if high_gate:
        key[tab] = [r % 8 for r in range(u)] + [0] * (n - u)
    asg = _key(cs, key)

    def witness(phase, ch, variant):
        rng = random.Random(700 + (0 if variant == BAD else variant))
        rows = [[rng.randrange(1 << 30) for _ in range(W)] for _ in range(m)]
        pi = _perm(rng, m)
        # (where the selector is off both tuples are zero whatever the columns hold: arbitrary values there)
        cols = {c: [rows[r][e] for r in range(m)] + [rng.randrange(100) for _ in range(u - m)] + [0] * (n - u) for e, c in enumerate(ac)}
        for e, c in enumerate(bc):
            cols[c] = [rows[pi[r]][e] for r in range(m)] + [rng.randrange(100) for _ in range(u - m)] + [0] * (n - u)
        _spoil(cols[bc[1]], variant)
        if high_gate:
            cols[p5] = [pow(v, 5, R) for v in cols[ac[0]]]
            cols[sq] = [v * v % R for v in cols[ac[0]]]
            cols[t] = [rng.randrange(8) for _ in range(u)] + [0] * (n - u)
        return cols

    return Phased("wide", cs, asg, [0] * cs.n_advice, [], 0, witness)


def three(k: int = 5) -> Phased:
    """three shuffles (widths 1, 2, 1), two lookups and a permutation in one circuit"""
    cs = ShuffleCS(k)
    tab = cs.fixed_column()
    a, b, c, d, e = (cs.advice_column() for _ in range(5))
    cs.enable_equality(ADVICE, a)
    cs.enable_equality(ADVICE, e)
    cs.lookup([cs.advice(a)], [cs.fixed(tab)])
    cs.lookup([cs.advice(c)], [cs.fixed(tab)])
    cs.shuffle([cs.advice(a)], [cs.advice(b)])
    cs.shuffle([cs.advice(a), cs.advice(c)], [cs.advice(b), cs.advice(d)])
    cs.shuffle([cs.advice(c) + 1], [cs.advice(d) + 1])
    n, u = 1 << k, cs.usable_rows()
    asg = _key(cs, {tab: [r % 8 for r in range(u)] + [0] * (n - u)})
    # (a[0] = e[0] for every witness: both are 3)
    asg.set(ADVICE, a, 0, 3)
    asg.set(ADVICE, e, 0, 3)
    asg.copy((ADVICE, a, 0), (ADVICE, e, 0))

    def witness(phase, ch, variant):
        rng = random.Random(800 + (0 if variant == BAD else variant))
        av = [3] + [rng.randrange(8) for _ in range(u - 1)]
        cv = [rng.randrange(8) for _ in range(u)]
        pi = _perm(rng, u)
        pad = [0] * (n - u)
        return {a: av + pad, b: [av[i] for i in pi] + pad, c: cv + pad, d: _spoil([cv[i] for i in pi], variant) + pad,
                e: [3] + [0] * (n - 1)}

    return Phased("three", cs, asg, [0] * 5, [], 0, witness)


def only(k: int = 5) -> Phased:
    """shuffles and nothing else: no fixed column, no gate, no lookup, no permutation (two shuffles over three columns)"""
    cs = ShuffleCS(k)
    a, b, c = cs.advice_column(), cs.advice_column(), cs.advice_column()
    cs.shuffle([cs.advice(a)], [cs.advice(b)])
    cs.shuffle([cs.advice(b)], [cs.advice(c)])
    n, u = 1 << k, cs.usable_rows()
    asg = _key(cs, {})

    def witness(phase, ch, variant):
        rng = random.Random(900 + (0 if variant == BAD else variant))
        av = [rng.randrange(1 << 40) for _ in range(u)]
        bv = [av[i] for i in _perm(rng, u)]
        cv = [bv[i] for i in _perm(rng, u)]
        pad = [0] * (n - u)
        return {a: av + pad, b: bv + pad, c: _spoil(cv, variant) + pad}

    return Phased("only", cs, asg, [0, 0, 0], [], 0, witness)


def rotated(k: int = 5) -> Phased:
    """expressions at rotations -1 and +1: q (a(w^-1 X) + 2 a(w X)) against q b(w X), q off on the first and the last
    usable rows, whose neighbours are blinding rows"""
    cs = ShuffleCS(k)
    q = cs.fixed_column()
    a, b = cs.advice_column(), cs.advice_column()
    cs.shuffle([cs.fixed(q) * (cs.advice(a, -1) + 2 * cs.advice(a, 1))], [cs.fixed(q) * cs.advice(b, 1)])
    n, u = 1 << k, cs.usable_rows()
    rows = list(range(1, u - 1))
    asg = _key(cs, {q: [1 if r in rows else 0 for r in range(n)]})

    def witness(phase, ch, variant):
        rng = random.Random(1000 + (0 if variant == BAD else variant))
        av = [rng.randrange(1 << 20) for _ in range(u)] + [0] * (n - u)
        vals = [(av[r - 1] + 2 * av[r + 1]) % R for r in rows]
        pi = _perm(rng, len(rows))
        bv = [0] * n
        for i, r in enumerate(rows):
            bv[r + 1] = vals[pi[i]]
        return {a: av, b: _spoil(bv, variant, row=3)}

    return Phased("rotated", cs, asg, [0, 0], [], 0, witness)


def with_challenge(k: int = 5, phased: bool = False) -> Phased:
    """a challenge squeezed behind phase 0 inside both expressions: a + c0 a' against b + c0 b', (b, b') a row permutation
    of (a, a') -- a shuffle for every value of c0.  phased: b and b' are phase-1 columns (zg_prover_prove_phased)."""
    cs = ShuffleCS(k)
    a, a2, b, b2 = (cs.advice_column() for _ in range(4))
    c0 = cs.challenge(0)
    cs.shuffle([cs.advice(a) + c0 * cs.advice(a2)], [cs.advice(b) + c0 * cs.advice(b2)])
    assert cs.degree() == 3
    n, u = 1 << k, cs.usable_rows()
    asg = _key(cs, {})
    phases = [0, 0, 1, 1] if phased else [0, 0, 0, 0]

    def witness(phase, ch, variant):
        rng = random.Random(1100 + (0 if variant == BAD else variant))
        av = [rng.randrange(1 << 20) for _ in range(u)]
        a2v = [rng.randrange(1 << 20) for _ in range(u)]
        pi = _perm(rng, u)
        pad = [0] * (n - u)
        cols = {a: av + pad, a2: a2v + pad, b: [av[i] for i in pi] + pad, b2: _spoil([a2v[i] for i in pi], variant) + pad}
        return {c: v for c, v in cols.items() if phases[c] == phase}

    return Phased("with_challenge_phased" if phased else "with_challenge", cs, asg, phases, [0], 0, witness)


SMALL = {"plain": plain, "wide": wide, "three": three, "only": only, "rotated": rotated, "with_challenge": with_challenge,
         "with_challenge_phased": lambda: with_challenge(5, True)}


def cell_at(pc, advice_ints, challenges=()):
    """the witness as proof_ref.shuffle_product reads it: advice_ints[column][row] canonical integers (fixed from the key)"""
    cs, n = pc.cs, pc.n

    def at(row):
        def f(qi):
            kind, col, rot = cs.queries[qi]
            if kind == ADVICE:
                return advice_ints[col][(row + rot) % n]
            if kind == 3:
                return challenges[col]
            return pc.asg.col(kind)[col][(row + rot) % n]
        return f
    return at
