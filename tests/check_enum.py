"""The comparator of the witness-check tests: `Assignment.check()` (harness/circuit.py) made to LIST failures instead
of asserting, plus the copy walk over `Assignment.mapping` -- Python big integers, nothing of the library under test.

failures(cs, asg) -> (totals, records): totals = [gate, lookup, copy] counts, records = (kind, index, row, other_index,
other_row) tuples in ascending (kind, index, row) order, the order zg_prover_check_* reports in."""
import copy

from circuit import ADVICE, FIXED, INSTANCE, R, ConstraintSystem

GATE, LOOKUP, COPY = 0, 1, 2


def failures(cs, asg):
    n, usable = asg.n, cs.usable_rows()

    def cell_at(row):
        def f(qi):
            kind, c, rot = cs.queries[qi]
            return asg.col(kind)[c][(row + rot) % n]
        return f

    cells = [cell_at(r) for r in range(n)]
    recs = []
    for gi, g in enumerate(cs.gates):
        for row in range(usable):
            if g.eval(cells[row]) != 0:
                recs.append((GATE, gi, row, 0, 0))
    for li, (ins, tabs) in enumerate(cs.lookups):
        table = {tuple(t.eval(cells[r]) for t in tabs) for r in range(usable)}
        for row in range(usable):
            if tuple(e.eval(cells[row]) for e in ins) not in table:
                recs.append((LOOKUP, li, row, 0, 0))
    for c, (kind, col) in enumerate(cs.perm_columns):
        for r in range(n):
            c2, r2 = asg.mapping[c][r]
            kind2, col2 = cs.perm_columns[c2]
            if asg.col(kind)[col][r] != asg.col(kind2)[col2][r2]:
                recs.append((COPY, c, r, c2, r2))
    totals = [sum(1 for x in recs if x[0] == kd) for kd in (GATE, LOOKUP, COPY)]
    return totals, recs


def changed(asg, edits):
    """A copy of the assignment with cells overwritten: edits = [(kind, column, row, value or callable(old) -> new)].
    (Assignment.set on the copy: no copy constraint is re-asserted, the mapping stays the circuit's.)"""
    out = copy.copy(asg)
    out.fixed = asg.fixed  # (the key's: never edited)
    out.advice = [list(c) for c in asg.advice]
    out.instance = [list(c) for c in asg.instance]
    for kind, column, row, value in edits:
        assert kind in (ADVICE, INSTANCE)
        old = out.col(kind)[column][row]
        out.col(kind)[column][row] = (value(old) if callable(value) else value) % R
    return out


def satisfied_by_check(asg) -> bool:
    """Assignment.check()'s verdict (gates and lookups on the usable rows; it asserts copies when they are made)."""
    try:
        asg.check()
        return True
    except AssertionError:
        return False


# ---- circuits of the test files' own
def advice_table_circuit(k=5):
    """lookup([advice a0], [advice a1]): the table side is part of the witness.  a1[r] = r mod 7, a0[r] = 3r mod 7."""
    cs = ConstraintSystem(k)
    a0, a1 = cs.advice_column(), cs.advice_column()
    cs.enable_equality(ADVICE, a0)
    cs.lookup([cs.advice(a0)], [cs.advice(a1)])
    from circuit import Assignment

    asg = Assignment(cs)
    for r in range(cs.usable_rows()):
        asg.set(ADVICE, a1, r, r % 7)
        asg.set(ADVICE, a0, r, 3 * r % 7)
    return cs, asg, 0


def wrap_circuit(k=5):
    """A gate q * (a0 - a1(-1)) enabled on row 0 only: it reads a1 at row n - 1 (the rotation wraps).  Such a witness can
    be checked, not proved: the prover blinds row n - 1."""
    from circuit import Assignment

    cs = ConstraintSystem(k)
    q = cs.fixed_column()
    a0, a1 = cs.advice_column(), cs.advice_column()
    cs.enable_equality(ADVICE, a0)
    cs.create_gate([cs.fixed(q) * (cs.advice(a0) - cs.advice(a1, -1))])
    asg = Assignment(cs)
    asg.set(FIXED, q, 0, 1)
    asg.set(ADVICE, a0, 0, 41)
    asg.set(ADVICE, a1, asg.n - 1, 41)
    return cs, asg, 0
