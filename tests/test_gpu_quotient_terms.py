"""The quotient's terms by degree on the split extended domain (zg_prover_quotient_terms).

A term of degree d <= m1 + 1 contributes a quotient part of degree < m1 n, which the first part of the split domain
(m1 n points) fixes alone; the throughput form therefore evaluates only the higher terms on the second part and transforms
only the polynomials they read onto it.  Here: the classification itself, and that nothing a verifier sees depends on it --
field arithmetic is exact, so every comparison is equality: h on EvaluationDomain's coset, the h pieces and the proof
bytes against the oracle, against the same prover with every term on both parts (set_quotient_terms(False)), against a
prover without the split domain (ZG_SPLIT_DOMAIN=0) and against the latency form."""
import random

import numpy as np
import pytest

from circuit import ADVICE, FIXED, R, Assignment, ConstraintSystem
from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu


def degree_circuit(k, perm_cols=8, high_deg=6, low_gate=True, lookups=(2, 3), rotations=False, seed=7):
    """`perm_cols` advice columns with equal rows under the permutation argument (sets of high_deg - 2 columns), then
    gate 0 of degree high_deg: q * (x * y^(high_deg - 2) - o_hi) -- or, `rotations`, q * (x(+1) x(-1) y^(high_deg - 3) - o_hi);
    gate 1 (`low_gate`) of degree 3: q * (x * y - o_lo), which reads the high gate's columns; one lookup per entry of
    `lookups`, with an input of that degree (q * b, q * b * c, q * b * c * c) into a 16-entry table.  Satisfied; o_hi and
    o_lo are read by their gate alone, so altering one of their cells breaks exactly that gate."""
    rng = random.Random(seed)
    cs = ConstraintSystem(k)
    q, tab = cs.fixed_column(), cs.fixed_column()
    cols = [cs.advice_column() for _ in range(max(perm_cols, 2))]
    o_hi = cs.advice_column()
    o_lo = cs.advice_column() if low_gate else None
    b = cs.advice_column() if lookups else None
    c = cs.advice_column() if any(d > 2 for d in lookups) else None  # (no column without a query)
    for col in cols[:perm_cols]:
        cs.enable_equality(ADVICE, col)
    A, qe = cs.advice, cs.fixed(q)
    x, y = cols[0], cols[1]
    hi = A(x, 1) * A(x, -1) if rotations else A(x) * A(y)
    for _ in range(high_deg - 3):
        hi = hi * A(y)
    gates = [qe * (hi - A(o_hi))]
    if low_gate:
        gates.append(qe * (A(x) * A(y) - A(o_lo)))
    cs.create_gate(gates)
    for d in lookups:
        e = qe * A(b)
        for _ in range(d - 2):
            e = e * A(c)
        cs.lookup([e], [cs.fixed(tab)])
    assert cs.degree() == high_deg
    asg = Assignment(cs)
    usable = cs.usable_rows()
    val = [rng.randrange(R) for _ in range(usable)]
    for r in range(usable):
        asg.set(FIXED, tab, r, r % 16)
        for col in cols:
            asg.set(ADVICE, col, r, val[r])
        if b is not None:
            asg.set(ADVICE, b, r, rng.randrange(16))
        if c is not None:
            asg.set(ADVICE, c, r, rng.randrange(2))
    for r in range(1, usable - 1):
        asg.set(FIXED, q, r, 1)
        v = val[r]
        top = val[r + 1] * val[r - 1] * pow(v, high_deg - 3, R) if rotations else pow(v, high_deg - 1, R)
        asg.set(ADVICE, o_hi, r, top % R)
        if low_gate:
            asg.set(ADVICE, o_lo, r, v * v % R)
    for r in range(0, usable, 3):
        for i in range(perm_cols - 1):
            asg.copy((ADVICE, cols[i], r), (ADVICE, cols[i + 1], r))
    return (cs, asg, 0), dict(o_hi=o_hi, o_lo=o_lo, x=x, y=y, b=b, c=c, n_cols=len(cols))


def keys(orc, zg, ctx, built, k, **knobs):
    cs, asg, ilen = built
    img = cs.to_c()
    params = orc.params_new(k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x7654321)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    pk = orc.ProvingKey(img, fixed, sigma, params, vk_repr)
    before = {name: zg.tuning_get(name) for name in knobs}
    try:
        for name, v in knobs.items():
            zg.tuning_set(name, v)
        prover = zg.Prover(ctx, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr)
    finally:
        for name, v in before.items():
            zg.tuning_set(name, v)
    return pk, prover, (img, fixed, sigma, params, vk_repr)


def slabs(cs):
    """where a proof's coset slabs start: advice, instance, permutation z, lookup z, a'/s' (interleaved)"""
    chunk = cs.degree() - 2
    sets = (len(cs.perm_columns) + chunk - 1) // chunk if cs.perm_columns else 0
    adv, inst = 0, cs.n_advice
    pz = inst + cs.n_instance
    lz = pz + sets
    perm = lz + len(cs.lookups)
    return dict(adv=adv, inst=inst, pz=pz, lz=lz, perm=perm, total=perm + 2 * len(cs.lookups), sets=sets)


def same_everywhere(orc, zg, ctx, built, k, seed=5, batch=None):
    """The throughput form by degree == the oracle (h on the extended coset, h pieces, bytes) == every term on both parts ==
    no split domain == the latency form.  batch: seeds of a lock-step batch proved as well (slot 1's pieces compared)."""
    cs, asg, ilen = built
    pk, prover, _ = keys(orc, zg, ctx, built, k)
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    n, en, qpd = 1 << k, 1 << cs.extended_k(), cs.degree() - 1
    st, want, tr = orc.create_proof(pk, adv, inst, seed, want_trace=True)
    assert st == 0
    prover.set_overlap(False)
    assert prover.prove(adv, inst, seed) == want, "bytes, by degree"
    assert np.array_equal(prover.fetch(0, 0, en), tr.array("h_ext", en)), "h on the extended coset"
    assert np.array_equal(prover.fetch(5, 0, qpd * n), tr.array("h_pieces", qpd * n)), "h pieces"
    orc.trace_free(tr)
    if batch:
        prover.set_batch(len(batch))
        got, sts = prover.prove_batch([adv] * len(batch), [inst] * len(batch), batch)
        assert sts == [0] * len(batch)
        for s, (seed_b, proof) in enumerate(zip(batch, got)):
            st, want_b, tr = orc.create_proof(pk, adv, inst, seed_b, want_trace=True)
            assert st == 0 and proof == want_b, ("batch", s)
            if s == 1:
                assert np.array_equal(prover.fetch(5, 0, qpd * n, slot=1), tr.array("h_pieces", qpd * n)), "slot 1's h pieces"
                assert np.array_equal(prover.fetch(0, 0, en, slot=1), tr.array("h_ext", en)), "slot 1's h"
            orc.trace_free(tr)
    prover.set_quotient_terms(False)
    assert prover.prove(adv, inst, seed) == want, "bytes, every term on both parts"
    prover.set_quotient_terms(True)
    assert prover.prove(adv, inst, seed) == want, "bytes, by degree again"
    prover.set_overlap(True)
    assert prover.prove(adv, inst, seed) == want, "bytes, latency form"
    info = prover.quotient_terms()
    prover.close()
    _pk, single, _ = keys(orc, zg, ctx, built, k, ZG_SPLIT_DOMAIN=0)
    single.set_overlap(False)
    assert single.prove(adv, inst, seed) == want, "bytes, ZG_SPLIT_DOMAIN=0"
    assert not single.quotient_terms()["active"]
    single.close()
    assert orc.verify_proof_pairing(pk, inst, want) == 1
    return info


def test_mixed_degrees(ctx, zg, orc):
    """degree 6 (4n + n): gate 0 high, gate 1 low; lookup 0 (input degree 2: product term 5) low, lookup 1 (input degree 3:
    product term 6) high; eight permutation columns in two full sets, both high"""
    built, c = degree_circuit(7)
    info = same_everywhere(orc, zg, ctx, built, 7)
    cs = built[0]
    at = slabs(cs)
    assert info["active"] and info["gates"] == [1, 0] and info["sets"] == [1, 1] and info["lookups"] == [0, 1]
    off = sorted(i for i, f in enumerate(info["part2"]) if not f)
    # o_lo is read by the low gate alone; b by both lookups, c by the high one
    assert off == sorted([c["o_lo"], at["lz"], at["perm"], at["perm"] + 1])
    assert len(info["part2"]) == at["total"]


def test_short_last_set(ctx, zg, orc):
    """five permutation columns at degree 6: sets of 4 + 1; the last set's product term has degree 3 and is low, and its z is
    read by low terms only (its own product, l_last, the chaining term), the first set's z by its high product term"""
    built = toy_circuit(7, force_degree=6)
    info = same_everywhere(orc, zg, ctx, built, 7)
    at = slabs(built[0])
    assert at["sets"] == 2 and info["active"] and info["sets"] == [1, 0] and info["lookups"] == [0]
    assert info["gates"] == [0, 0, 1]
    assert info["part2"][at["pz"]] == 1 and info["part2"][at["pz"] + 1] == 0
    assert info["part2"][at["lz"]:] == [0, 0, 0]
    assert info["part2"][:at["pz"]] == [1, 1, 1, 1]  # a0, a1, a2 (the high gate, the first set) and the instance column (the first set)


def test_high_gate_with_rotations(ctx, zg, orc):
    """the high gate reads x at rotations +1 and -1 (rows 4 apart on the first part, 1 apart on the second) and shares x and y
    with the low gate: both stay on the second part"""
    built, c = degree_circuit(7, perm_cols=3, lookups=(2,), rotations=True)
    info = same_everywhere(orc, zg, ctx, built, 7)
    assert info["active"] and info["gates"] == [1, 0] and info["sets"] == [0] and info["lookups"] == [0]
    assert info["part2"][c["x"]] == 1 and info["part2"][c["y"]] == 1 and info["part2"][c["o_hi"]] == 1
    assert info["part2"][c["o_lo"]] == 0 and info["part2"][c["b"]] == 0
    assert sum(info["part2"]) == 3


def test_everything_high(ctx, zg, orc):
    """Gates only, all of degree 6: no term is low and the feature is off.  With a lookup whose product term has degree 6
    beside the high gate, every gate, set and product term is high -- a lookup's other four terms (degree 2 - 3) never are."""
    built, _c = degree_circuit(6, perm_cols=0, low_gate=False, lookups=())
    info = same_everywhere(orc, zg, ctx, built, 6)
    assert not info["active"] and info["gates"] == [1] and info["sets"] == [] and info["lookups"] == []
    built, _c = degree_circuit(6, perm_cols=4, low_gate=False, lookups=(3,))
    info = same_everywhere(orc, zg, ctx, built, 6)
    assert info["gates"] == [1] and info["sets"] == [1] and info["lookups"] == [1]
    assert info["part2"][-3:] == [1, 1, 1]


@pytest.mark.parametrize("kind", ["gates_only", "no_lookup"])
def test_gates_only_and_no_lookups(ctx, zg, orc, kind):
    built = variant_circuit(kind, k=6)
    info = same_everywhere(orc, zg, ctx, built, 6)
    # gates_only, degree 4 (2n + n; low: degree <= 3): classified, but without permutation and lookups evaluate_h is not
    # in its grouped form, which the terms by degree need; no_lookup, degree 3: one coset.  Inert both times.
    assert not info["active"]
    if kind == "gates_only":
        assert info["gates"] == [0, 1] and info["part2"] == [1, 0]


@pytest.mark.parametrize("force_degree,active", [(7, True), (5, False), (8, False)])
def test_other_splits(ctx, zg, orc, force_degree, active):
    """degree 7: 4n + 2n; degrees 5 and 8: EvaluationDomain's coset is minimal already and the feature is inert"""
    built = toy_circuit(7, force_degree=force_degree)
    info = same_everywhere(orc, zg, ctx, built, 7)
    assert info["active"] == active
    if active:
        assert info["gates"] == [0, 0, 1] and info["sets"] == [1] and info["lookups"] == [0]


def test_a_batch_of_three(ctx, zg, orc):
    built, _c = degree_circuit(8)
    same_everywhere(orc, zg, ctx, built, 8, seed=11, batch=[11, 12, 13])


@pytest.mark.parametrize("which", ["o_lo", "o_hi"])
def test_a_statement_that_does_not_hold(ctx, zg, orc, which):
    """One cell altered so that the low (then the high) gate fails on a row.  Neither share of the quotient is a polynomial
    then; the throughput form promises what it promised before: the same bytes every time and from both entries, and no
    verifier accepts them."""
    built, c = degree_circuit(7)
    cs, asg, ilen = built
    pk, prover, _ = keys(orc, zg, ctx, built, 7)
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    bad = adv.copy()
    bad[c[which], 9] = orc.fr_from_int(12345)
    prover.set_overlap(False)
    prover.set_batch(3)
    first = prover.prove(bad, inst, 21)
    assert prover.prove(bad, inst, 21) == first
    got, sts = prover.prove_batch([adv, bad, bad], [inst] * 3, [20, 21, 21])
    assert sts == [0, 0, 0] and got[1] == first and got[2] == first
    assert got[0] == orc.create_proof(pk, adv, inst, 20)[1]
    assert orc.verify_proof_pairing(pk, inst, first) != 1
    assert orc.verify_proof_pairing(pk, inst, got[0]) == 1
    prover.close()


def test_the_tiny_model_k14(ctx, zg, orc):
    import wnn_circuit
    import wnn_model

    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    cs, asg, ilen, _scores = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), k)
    pk, prover, _ = keys(orc, zg, ctx, (cs, asg, ilen), k)
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    prover.set_overlap(False)
    st, want, _ = orc.create_proof(pk, adv, inst, 31)
    assert st == 0 and prover.prove(adv, inst, 31) == want
    info = prover.quotient_terms()
    prover.close()
    at = slabs(cs)
    assert cs.degree() == 6 and info["active"]
    assert [g for g, hi in enumerate(info["gates"]) if hi] == [0, 4, 5, 8] and len(info["gates"]) == 12
    assert info["sets"] == [1, 1] and info["lookups"] == [0, 0, 0, 1]
    off = [i for i, f in enumerate(info["part2"]) if not f]
    # 9 of the 21 polynomials: z, a' and s' of lookups 0 - 2
    assert at["total"] == 21 and len(info["part2"]) == 21
    assert off == [at["lz"], at["lz"] + 1, at["lz"] + 2] + list(range(at["perm"], at["perm"] + 6))
