"""The oracle's lookup argument pinned to permute_expression_pair on Python integers (tests/lookup_cases.py), on the
adversarial column families and at multi-chunk sizes; no GPU.  tests/test_gpu_lookup.py compares the HIP prover with the
oracle on the same circuits: this file is why the oracle may be trusted there -- permute_ref shares no code with it."""
import pytest

import lookup_cases as lc
from check_enum import LOOKUP, changed, failures
from circuit import ADVICE, R


def proving_key(orc, cs, asg, k):
    img = cs.to_c()
    params = orc.params_new(k, 0xABCDEF)
    return orc.ProvingKey(img, asg.fixed_values(), asg.sigma_values(), params, orc.fr_from_int(0x1234567))


def oracle_matches_reference(orc, cs, asg, k, pairs, seed=1):
    """pairs[l] = (input columns, table columns) of lookup l as integer lists.  Proves with the oracle and compares its
    a' / s' on the usable rows with permute_ref of the theta-compressed columns; the pairing verifier must accept."""
    pk = proving_key(orc, cs, asg, k)
    adv, inst = asg.advice_values(), asg.instance_values(0)
    st, proof, tr = orc.create_proof(pk, adv, inst, seed, want_trace=True)
    assert st == 0
    n, usable = 1 << k, cs.usable_rows()
    theta = orc.fr_to_int(tr.fe("theta"))
    got_a = tr.array("permuted_input", len(pairs) * n)
    got_s = tr.array("permuted_table", len(pairs) * n)
    for l, (ins, tabs) in enumerate(pairs):
        a = lc.from_mont_array(got_a[l * n:l * n + usable])
        s = lc.from_mont_array(got_s[l * n:l * n + usable])
        lc.check_permuted(lc.compress(ins, theta), lc.compress(tabs, theta), a, s)
    orc.trace_free(tr)
    assert orc.verify_proof_pairing(pk, inst, proof) == 1


@pytest.mark.parametrize("k", [11, 13])
@pytest.mark.parametrize("name", list(lc.FAMILIES))
def test_oracle_permuted_columns_equal_the_integer_reference(orc, name, k):
    table, inputs = lc.make(name, k)
    cs, asg, _ = lc.lookup_circuit(k, table, inputs)
    oracle_matches_reference(orc, cs, asg, k, [([inputs], [table])])


def test_oracle_wide_lookup_equals_the_integer_reference(orc):
    tabs, ins = lc.wide_case(11)
    cs, asg, _ = lc.lookup_circuit(11, tabs, ins, width=2)
    oracle_matches_reference(orc, cs, asg, 11, [(list(ins), list(tabs))])


def test_oracle_two_lookups_equal_the_integer_reference(orc):
    (t0, a0), (t1, a1) = lc.make("runs", 11), lc.make("zipf", 11)
    cs, asg, _ = lc.lookup_circuit(11, [t0, t1], [a0, a1], lookups=2)
    assert len(cs.lookups) == 2
    oracle_matches_reference(orc, cs, asg, 11, [([a0], [t0]), ([a1], [t1])])


def test_oracle_advice_table_equals_the_integer_reference(orc):
    table, inputs = lc.make("limbs", 11)
    cs, asg, _ = lc.lookup_circuit(11, table, inputs, advice_table=True)
    assert cs.n_fixed == 0 and cs.n_advice == 2
    oracle_matches_reference(orc, cs, asg, 11, [([inputs], [table])])


def test_a_missing_input_is_refused_by_oracle_reference_and_enumerator(orc):
    k = 11
    table, inputs = lc.make("zipf", k)
    cs, asg, _ = lc.lookup_circuit(k, table, inputs)
    row = 1500
    missing = next(v for v in (R - 1, R - 2, R - 3) if v not in set(table))
    bad = changed(asg, [(ADVICE, 0, row, missing)])
    pk = proving_key(orc, cs, asg, k)
    st, proof, _ = orc.create_proof(pk, bad.advice_values(), bad.instance_values(0), 1)
    assert st == -5
    with pytest.raises(ValueError):
        lc.permute_ref(inputs[:row] + [missing] + inputs[row + 1:], table)
    assert failures(cs, bad) == ([0, 1, 0], [(LOOKUP, 0, row, 0, 0)])
    assert failures(cs, asg) == ([0, 0, 0], [])


def test_the_reference_and_the_family_assertions_can_fail():
    k = 11
    usable = lc.usable_rows(k)
    table, inputs = lc.make("zipf", k)
    a, s = lc.permute_ref(inputs, table)
    lc.check_permuted(inputs, table, a, s)
    i = next(r for r in range(usable - 1) if s[r] != s[r + 1])
    swapped = s[:i] + [s[i + 1], s[i]] + s[i + 2:]
    with pytest.raises(AssertionError, match=f"s' differs on row {i}"):
        lc.check_permuted(inputs, table, a, swapped)
    j = next(r for r in range(usable - 1) if a[r] != a[r + 1])  # (the end of the first run)
    with pytest.raises(AssertionError, match=f"a' differs on row {j}"):
        lc.check_permuted(inputs, table, a[1:] + a[:1], s)
    # a' and s' are permutations of the inputs and of the table (the argument's own claim)
    assert sorted(s) == sorted(table) and a == sorted(inputs)
    for name in lc.FAMILIES:
        table, inputs = lc.make(name, k)
        big = [R + (v & 0xffff) if j == 7 else v for j, v in enumerate(inputs)]
        with pytest.raises(AssertionError, match=f"family {name}: every input value is in"):
            lc.check_family(name, table, big, usable)
        with pytest.raises(AssertionError, match=f"family {name}: columns are"):
            lc.check_family(name, table, inputs[:-1], usable)
    # ... and each family's own property: inputs of another family do not pass for it
    table, inputs = lc.make("permutation", k)
    for name, what in (("all_equal", "every input is the same value"), ("runs", "run lengths of the sorted inputs are exactly")):
        with pytest.raises(AssertionError, match=f"family {name}: {what}"):
            lc.check_family(name, table, inputs, usable)
    with pytest.raises(AssertionError, match="family permutation: the inputs are a shuffle"):
        lc.check_family("permutation", table, [inputs[0]] * usable, usable)
    t2, i2 = lc.make("half_r", k)
    with pytest.raises(AssertionError, match="family half_r: a' has the run-form coefficient h"):
        lc.check_family("half_r", t2, [lc.H if v == lc.H + 1 else v for v in i2], usable)
    t3, i3 = lc.make("pow2_gaps", k)
    drop = sorted(set(i3))[100]
    with pytest.raises(AssertionError, match="family pow2_gaps: every table value is looked up"):
        lc.check_family("pow2_gaps", t3, [i3[0] if v == drop else v for v in i3], usable)
    t4, i4 = lc.make("limbs", k)
    with pytest.raises(AssertionError, match="family limbs: "):
        lc.check_family("limbs", [1 if v == 1 << 224 else v for v in t4], [1 if v == 1 << 224 else v for v in i4], usable)


def test_the_families_have_the_shapes_the_kernels_branch_on():
    """what the GPU tests rely on, stated once: run boundaries against the 1024-row tiles and m_rep at its ends"""
    for k in (10, 11, 12, 13, 14):
        usable = lc.usable_rows(k)
        for name in ("runs", "zipf") if k == 14 else lc.FAMILIES:
            table, inputs = lc.make(name, k)
            assert len(table) == len(inputs) == usable
        t = lc.shared_table(k)
        for name in ("all_equal", "permutation", "runs", "half_r"):
            lc.make(name, k, table=t)
    assert lc.run_lengths(lc.make("runs", 12)[1]) == [1023, 1, 1024, 1025, 1017]
    assert lc.run_lengths(lc.make("runs", 11)[1]) == [1023, 1, 1018]
    assert lc.run_lengths(lc.make("permutation", 12)[1]) == [1] * lc.usable_rows(12)
