"""The comparator of the zg_prover_check_circuit tests: tests/check_enum.py's enumeration for a circuit with challenges
and shuffles, on Python integers -- nothing of the library under test.

failures4(cs, key_asg, advice_ints, instance_ints, challenges) -> (totals, records)
  cs             a ConstraintSystem, possibly with challenge queries (kind 3) and cs.shuffles
  key_asg        the circuit's Assignment: its fixed columns and its permutation mapping are read, nothing else
  advice_ints    [n_advice][n] canonical integers; instance_ints [n_instance][<= n] (zero beyond); challenges [ints]
  totals         [gate, lookup, copy, shuffle] counts
  records        (kind, index, row, other_index, other_row) in ascending (kind, index, row) order

The shuffle kind restates MockProver::verify's shuffle check (privacy-scaling-explorations/halo2 from v0.3.0 on, dev.rs)
from the published source; it is not checked against upstream here.  Per shuffle: the usable rows of each side sorted by
(tuple, row) with sorted(), compared position by position; the input row at a position whose tuple differs from the
shuffle row's there fails and names that row."""
from circuit import ADVICE, FIXED, INSTANCE, R

GATE, LOOKUP, COPY, SHUFFLE = 0, 1, 2, 3
CHALLENGE = 3


def failures4(cs, key_asg, advice_ints, instance_ints, challenges=()):
    n, usable = 1 << cs.k, cs.usable_rows()
    instance = [list(c) + [0] * (n - len(c)) for c in instance_ints]
    cols = {FIXED: key_asg.fixed, ADVICE: advice_ints, INSTANCE: instance}

    def cell_at(row):
        def f(qi):
            kind, c, rot = cs.queries[qi]
            if kind == CHALLENGE:
                return challenges[c] % R
            return cols[kind][c][(row + rot) % n] % R
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
            c2, r2 = key_asg.mapping[c][r]
            kind2, col2 = cs.perm_columns[c2]
            if cols[kind][col][r] % R != cols[kind2][col2][r2] % R:
                recs.append((COPY, c, r, c2, r2))
    for j, (ins, shs) in enumerate(getattr(cs, "shuffles", [])):
        a = sorted((tuple(e.eval(cells[r]) for e in ins), r) for r in range(usable))
        b = sorted((tuple(e.eval(cells[r]) for e in shs), r) for r in range(usable))
        bad = sorted((ra, rb) for (ta, ra), (tb, rb) in zip(a, b) if ta != tb)
        recs += [(SHUFFLE, j, ra, 0, rb) for ra, rb in bad]
    totals = [sum(1 for x in recs if x[0] == kd) for kd in (GATE, LOOKUP, COPY, SHUFFLE)]
    return totals, recs


def columns_of(pc, challenges, variant=0):
    """a Phased circuit's whole witness for given challenge values: [n_advice][n] canonical integers"""
    cols = {}
    for ph in range(pc.n_phases):
        cols.update(pc.witness(ph, list(challenges), variant))
    return [list(cols[c]) for c in range(pc.cs.n_advice)]


def instance_of(pc, variant=0):
    return [list(c) for c in pc._instance(variant)] if pc.cs.n_instance else []


def report(pc, challenges=(), variant=0, advice=None):
    """failures4 on a Phased circuit's own witness (or on `advice`, columns of canonical integers)"""
    adv = columns_of(pc, challenges, variant) if advice is None else advice
    return failures4(pc.cs, pc.asg, adv, instance_of(pc, variant), list(challenges))
