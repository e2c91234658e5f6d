"""Lookup-only circuits, adversarial value families for their columns, and permute_expression_pair on Python integers.

What the lookup argument does depends on the column VALUES: the order the prover's bitonic sort leaves (csrc/sort.hip),
the run structure its flags and scans see, which left-over table entry goes to which repeated row, the coefficients the
run-form commitment of a' and s' recodes (csrc/msm.hip), and the order the checker sorts a table into (csrc/check.hip).
The families below are columns built so that each of those is decided at its edges; every family asserts the property it
exists for (`check_family`), so a change that quietly removed the property fails here and not as a green GPU test.

  lookup_circuit(k, table, inputs, ...)  -> (cs, asg, 0): lookup([advice], [fixed]) and its variants, nothing else
  permute_ref(inputs, table)             -> (a', s') on the usable rows, as halo2_proofs v2023_04_20
                                            src/plonk/lookup/prover.rs permute_expression_pair words it
  FAMILIES[name](usable, rng, table=None)-> (table, inputs), integers in [0, r)
"""
from collections import Counter

from circuit import ADVICE, FIXED, R, Assignment, ConstraintSystem

H = (R - 1) // 2
RINV = pow(1 << 256, -1, R)
M32 = (1 << 32) - 1
RUN_LENGTHS = (1023, 1, 1024, 1025)  # then the remainder: ends one short of, at, at, and one past a 1024-row boundary


# ---------------------------------------------------------------- circuits
def lookup_circuit(k, table, inputs, advice_table=False, width=1, lookups=1):
    """`lookups` independent lookups of `width` columns each: input columns are advice, table columns fixed (advice when
    advice_table).  No gate, no permutation, no instance column: degree 4, extended_k = k + 2, usable = 2^k - 6.
    width == 1: table / inputs are lists of `usable` integers; width == 2: pairs of such lists (t0, t1) / (a0, a1);
    lookups == 2: a list of two such arguments, one per lookup."""
    cs = ConstraintSystem(k)
    tabs = [table] if lookups == 1 else list(table)
    ins = [inputs] if lookups == 1 else list(inputs)
    assert len(tabs) == len(ins) == lookups
    cols = []
    for _ in range(lookups):
        tcols = [cs.advice_column() if advice_table else cs.fixed_column() for _ in range(width)]
        acols = [cs.advice_column() for _ in range(width)]
        tkind = ADVICE if advice_table else FIXED
        cs.lookup([cs.advice(c) for c in acols], [cs.q(tkind, c, 0) for c in tcols])
        cols.append((tkind, tcols, acols))
    assert cs.degree() == 4 and cs.extended_k() == k + 2 and cs.blinding_factors() == 5
    usable = cs.usable_rows()
    asg = Assignment(cs)
    for (tkind, tcols, acols), t, a in zip(cols, tabs, ins):
        t = [t] if width == 1 else list(t)
        a = [a] if width == 1 else list(a)
        assert len(t) == len(a) == width
        for e in range(width):
            assert len(t[e]) == usable and len(a[e]) == usable, (len(t[e]), len(a[e]), usable)
            for r in range(usable):
                assert 0 <= t[e][r] < R and 0 <= a[e][r] < R
                asg.set(tkind, tcols[e], r, t[e][r])
                asg.set(ADVICE, acols[e], r, a[e][r])
    return cs, asg, 0


def usable_rows(k):
    return (1 << k) - 6


def from_mont_array(a):
    """uint64[count, 4] Montgomery limbs -> canonical Python integers"""
    return [(int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192) * RINV % R for x in a]


def compress(columns, theta):
    """lookup::Argument::compress_expressions: fold acc * theta + column, from zero"""
    out = [0] * len(columns[0])
    for c in columns:
        out = [(o * theta + v) % R for o, v in zip(out, c)]
    return out


# ---------------------------------------------------------------- the reference
def permute_ref(inputs, table):
    """permute_expression_pair on the usable rows: a' = the inputs sorted; the first row of each distinct value takes that
    value into s' and removes one instance from the table multiset; the ascending left-overs then go to the repeated rows,
    taken from the end (upstream pops its Vec of repeated rows).  Raises ValueError for an input the table does not hold."""
    assert len(inputs) == len(table)
    a = sorted(inputs)
    left = Counter(table)
    s = [None] * len(a)
    repeated = []
    for row, v in enumerate(a):
        if row and a[row - 1] == v:
            repeated.append(row)
            continue
        if left[v] <= 0:
            raise ValueError(f"input {v:#x} is not in the table")
        left[v] -= 1
        s[row] = v
    for v in sorted(left.elements()):
        s[repeated.pop()] = v
    assert not repeated
    return a, s


def check_permuted(inputs, table, a, s):
    """Is (a, s) what permute_expression_pair returns for (inputs, table)?  AssertionError says which row differs."""
    wa, ws = permute_ref(inputs, table)
    assert len(a) == len(wa) and len(s) == len(ws), "row counts differ"
    for row, (x, y) in enumerate(zip(wa, a)):
        assert x == y, f"a' differs on row {row}: {y:#x}, expected {x:#x}"
    for row, (x, y) in enumerate(zip(ws, s)):
        assert x == y, f"s' differs on row {row}: {y:#x}, expected {x:#x}"


def run_lengths(inputs):
    """lengths of the runs of equal values in sorted order, ascending by value"""
    c = Counter(inputs)
    return [c[v] for v in sorted(c)]


def run_coefficients(column):
    """the run-form commitment's coefficients s_i - s_{i+1} mod r on the rows of `column` (csrc/msm.hip)"""
    return [(x - y) % R for x, y in zip(column, column[1:])]


def limbs(v):
    return [(v >> (32 * j)) & M32 for j in range(8)]


# ---------------------------------------------------------------- value families
def _distinct(count, rng, avoid=()):
    seen, out = set(avoid), []
    while len(out) < count:
        v = rng.randrange(R)
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def _fill(values, usable, rng):
    """a table of `usable` rows holding every value at least once, the rest drawn from them, shuffled"""
    assert len(values) <= usable, f"{len(values)} values do not fit {usable} rows"
    t = list(values) + [rng.choice(values) for _ in range(usable - len(values))]
    rng.shuffle(t)
    return t


def _draw(values, usable, rng):
    """inputs: every value at least once, the rest drawn from them, shuffled"""
    return _fill(values, usable, rng)


def limb_values(rng):
    """the `limbs` family's distinct values, by group"""
    base = rng.randrange(1 << 224) | (0x10000000 << 224)  # eight random limbs, limb 7 well below r's 0x30644e72
    top = [base & ((1 << 224) - 1) | (t << 224) for t in (0, 1, 0x0fffffff, 0x10000001, 0x30644e71)]
    low = [base & ~M32 | t for t in (0, 1, 0x7fffffff, 0x80000000, M32)]
    ones = [1 << (32 * j) for j in range(8)]
    # (2^32 - 1) * 2^(32 j); for j = 7 that is not below r: r's own top limb instead, the largest limb-7-only value below r
    full = [M32 << (32 * j) for j in range(7)] + [(R >> 224) << 224]
    ends = [0, 1, R - 2, R - 1]
    return dict(base=base, top=top, low=low, ones=ones, full=full, ends=ends)


def all_equal(usable, rng, table=None):
    table = table or _distinct(usable, rng)
    inputs = [table[rng.randrange(usable)]] * usable
    return table, inputs


def permutation(usable, rng, table=None):
    table = table or _distinct(usable, rng)
    inputs = list(table)
    rng.shuffle(inputs)
    return table, inputs


def one_heavy_table(usable, rng, table=None):
    assert table is None
    v, w = _distinct(2, rng)
    table = [v] * (usable - 1)
    table.insert(rng.randrange(usable), w)
    inputs = [v, w] + [rng.choice((v, v, w)) for _ in range(usable - 2)]
    rng.shuffle(inputs)
    return table, inputs


def planned_runs(usable):
    """RUN_LENGTHS for as long as they fit, then the remainder as the last run"""
    out = []
    for length in RUN_LENGTHS:
        if sum(out) + length >= usable:
            break
        out.append(length)
    return out + [usable - sum(out)]


def runs(usable, rng, table=None):
    lengths = planned_runs(usable)
    if table is None:
        table = _distinct(usable, rng)
    values = sorted(rng.sample(table, len(lengths)))  # ascending: run i of the sorted column has length lengths[i]
    inputs = [v for v, c in zip(values, lengths) for _ in range(c)]
    rng.shuffle(inputs)
    return table, inputs


def limbs_family(usable, rng, table=None):
    assert table is None
    g = limb_values(rng)
    values = sorted(set(g["top"] + g["low"] + g["ones"] + g["full"] + g["ends"]))
    return _fill(values, usable, rng), _draw(values, usable, rng)


def pow2_gap_list():
    return [1] + [g for j in range(252) for g in ((1 << j) - 1, 1 << j) if g]


def pow2_gaps(usable, rng, table=None):
    assert table is None
    values, acc = [], 0
    for g in pow2_gap_list():
        acc += g
        values.append(acc)
    return _fill(values, usable, rng), _draw(values, usable, rng)


HALF_R_VALUES = (0, 1, H - 1, H, H + 1, H + 2, R - 2, R - 1)


def half_r(usable, rng, table=None):
    """The table holds the eight values, 0 once.  The inputs are 0 on all rows but four, which take h + 1, h + 2, r - 2 and
    r - 1: a' steps from 0 to h + 1 (coefficient -(h + 1) = h, the larger side of the decision: kept as it is), and s' puts
    the smallest left-over, 1, on the last repeated row, right before h + 1 (coefficient -h = h + 1: negated to h)."""
    if table is None:
        others = [v for v in HALF_R_VALUES if v]
        table = [0] + list(others) + [rng.choice(others) for _ in range(usable - 8)]
        rng.shuffle(table)
    inputs = [0] * (usable - 4) + [H + 1, H + 2, R - 2, R - 1]
    rng.shuffle(inputs)
    return table, inputs


def zipf(usable, rng, table=None):
    assert table is None
    values = _distinct(max(8, usable // 8), rng)
    weights = [1.0 / (i + 1) for i in range(len(values))]
    table = list(values) + rng.choices(values, weights, k=usable - len(values))
    rng.shuffle(table)
    inputs = rng.choices(values, weights, k=usable)
    return table, inputs


FAMILIES = {
    "all_equal": all_equal,
    "permutation": permutation,
    "one_heavy_table": one_heavy_table,
    "runs": runs,
    "limbs": limbs_family,
    "pow2_gaps": pow2_gaps,
    "half_r": half_r,
    "zipf": zipf,
}


def check_family(name, table, inputs, usable):
    """The property family `name` exists for, asserted on (table, inputs); the message names the family and the property."""
    def need(cond, what):
        assert cond, f"family {name}: {what}"

    need(len(table) == usable and len(inputs) == usable, f"columns are {usable} rows long")
    need(all(isinstance(v, int) and 0 <= v < R for v in table), "every table value is in [0, r)")
    need(all(isinstance(v, int) and 0 <= v < R for v in inputs), "every input value is in [0, r)")
    tset = set(table)
    need(all(v in tset for v in inputs), "every input is in the table")
    lens = run_lengths(inputs)
    m_rep = usable - len(lens)
    if name == "all_equal":
        need(len(tset) == usable, "the table's values are distinct")
        need(lens == [usable], "every input is the same value (m_rep = usable - 1)")
    elif name == "permutation":
        need(len(tset) == usable, "the table's values are distinct")
        need(sorted(inputs) == sorted(table) and m_rep == 0, "the inputs are a shuffle of the table (m_rep = m_left = 0)")
    elif name == "one_heavy_table":
        need(sorted(Counter(table).values()) == [1, usable - 1], "the table is one value usable - 1 times plus one other")
        need(len(lens) == 2, "the inputs hold both values")
    elif name == "runs":
        need(lens == planned_runs(usable), f"run lengths of the sorted inputs are exactly {planned_runs(usable)}, found {lens[:8]}")
        need(usable < sum(RUN_LENGTHS) or lens[:4] == list(RUN_LENGTHS), "all four boundary runs fit")
        ends = [sum(lens[:i + 1]) for i in range(len(lens) - 1)]
        need(usable <= 1024 or (1023 in ends and 1024 in ends), "runs end one short of and at the first 1024-row boundary")
    elif name == "limbs":
        vals = sorted(set(inputs))
        need(set(vals) == tset, "every table value is looked up")
        need({0, 1, R - 2, R - 1} <= tset, "0, 1, r - 2, r - 1 are present")
        for j in range(8):
            need(1 << (32 * j) in tset, f"2^(32*{j}) is present")
            need((M32 << (32 * j) if j < 7 else (R >> 224) << 224) in tset, f"the full limb {j} is present")
        for limb in (7, 0):
            group = [v for v in vals if any(u != v and [j for j in range(8) if limbs(u)[j] != limbs(v)[j]] == [limb] for u in vals)]
            need(len(group) >= 5, f"at least five keys differ from another key in limb {limb} only")
    elif name == "pow2_gaps":
        vals = sorted(set(inputs))
        need(set(vals) == tset, "every table value is looked up")
        gaps = [vals[0]] + [y - x for x, y in zip(vals, vals[1:])]
        need(gaps == pow2_gap_list(), "consecutive distinct values differ by 1, 1, 1, 2, 3, 4, 7, 8, ..., 2^251 - 1, 2^251")
        need(vals[-1] < R and vals[-1] + (1 << 252) - 1 + (1 << 252) >= R, "the sum stays below r with j <= 251 and would not with j <= 252")
        coeff = set(run_coefficients(sorted(inputs)))
        need(all((R - g) % R in coeff for g in pow2_gap_list()), "a' has every gap as a negated run-form coefficient")
    elif name == "half_r":
        need(set(HALF_R_VALUES) <= tset, "the table holds 0, 1, h - 1, h, h + 1, h + 2, r - 2, r - 1")
        a, s = permute_ref(inputs, table)
        ca, cs_ = set(run_coefficients(a)), set(run_coefficients(s))
        need(H in ca, "a' has the run-form coefficient h = (r - 1) / 2 (kept: r - h = h + 1 is larger)")
        need(H + 1 in cs_, "s' has the run-form coefficient h + 1 (negated: r - (h + 1) = h is smaller)")
    elif name == "zipf":
        need(len(tset) < usable // 4, "the table is heavily duplicated")
        need(len(set(lens)) >= 6 and m_rep > usable // 2 and max(lens) > 8 * min(lens), "the inputs have many different run lengths")
    else:
        raise KeyError(name)


def make(name, k, seed=0, table=None):
    """(table, inputs) of family `name` at 2^k rows, checked"""
    import random

    usable = usable_rows(k)
    rng = random.Random(f"{name}/{k}/{seed}")
    table, inputs = FAMILIES[name](usable, rng, table)
    check_family(name, table, inputs, usable)
    return table, inputs


def shared_table(k, seed=0):
    """One distinct table that serves all_equal, permutation, runs and half_r at once: the half_r values plus random ones."""
    import random

    usable = usable_rows(k)
    rng = random.Random(f"shared/{k}/{seed}")
    table = list(HALF_R_VALUES) + _distinct(usable - len(HALF_R_VALUES), rng, avoid=HALF_R_VALUES)
    rng.shuffle(table)
    return table


def wide_case(k, seed=0):
    """width = 2: the first table column takes three values, the second the `limbs` family: tuples tie on the first element.
    Returns ((t0, t1), (a0, a1)); the inputs are table rows drawn at random, every table row's tuple at least once."""
    import random

    usable = usable_rows(k)
    rng = random.Random(f"wide/{k}/{seed}")
    t1, _ = limbs_family(usable, rng)
    check_family("limbs", t1, list(t1), usable)
    firsts = _distinct(3, rng)
    t0 = [firsts[r % 3] for r in range(usable)]
    rows = list(range(usable))
    rng.shuffle(rows)
    rows = [rows[i] if i < usable // 2 else rng.choice(rows) for i in range(usable)]
    a0, a1 = [t0[r] for r in rows], [t1[r] for r in rows]
    pairs = Counter(zip(t0, t1))
    assert len(set(t0)) == 3 and max(Counter(t0).values()) > usable // 4, "family wide: three first elements, each on many rows"
    assert any(x == y and u != v and limbs(u)[:7] == limbs(v)[:7] for (x, u) in pairs for (y, v) in pairs), \
        "family wide: two table tuples tie on the first element and differ in limb 7 of the second only"
    return (t0, t1), (a0, a1)
