"""tests/check_enum_ext.failures4, the comparator of the zg_prover_check_circuit tests, held to the references the suite
already has: check_enum.failures for gates, lookups and copies (the challenges substituted first) and
proof_ref.shuffle_product for the shuffles; and the conditions the GPU test's capped cases rest on.  No device."""
import copy
import random
import types

import pytest

import check_circuit_cases as cases
import check_enum
import phases_circuits
import proof_ref
import shuffle_circuits
from check_enum_ext import CHALLENGE, SHUFFLE, columns_of, failures4, instance_of, report
from circuit import R, Expr
from shuffle_circuits import BAD

CIRCUITS = {**shuffle_circuits.SMALL, **phases_circuits.SMALL}


def substituted(cs, challenges):
    """the circuit's gates and lookups with every challenge query replaced by its value: what check_enum.failures reads"""
    def sub(e):
        terms = {}
        for key, coeff in e.terms.items():
            rest = tuple(q for q in key if cs.queries[q][0] != CHALLENGE)
            for q in key:
                if cs.queries[q][0] == CHALLENGE:
                    coeff = coeff * challenges[cs.queries[q][1]] % R
            terms[rest] = (terms.get(rest, 0) + coeff) % R
        return Expr(terms)

    return types.SimpleNamespace(k=cs.k, queries=cs.queries, perm_columns=cs.perm_columns, usable_rows=cs.usable_rows,
                                 gates=[sub(g) for g in cs.gates], lookups=[([sub(e) for e in i], [sub(e) for e in t]) for i, t in cs.lookups])


def assignment(pc, adv, variant):
    asg = copy.copy(pc.asg)
    asg.advice = [list(c) for c in adv]
    asg.instance = [list(c) + [0] * (pc.n - len(c)) for c in instance_of(pc, variant)]
    return asg


def witnesses(pc, name):
    """(challenges, variant, columns): the circuit's own variants and, for three_phase and rlc, a witness made for other
    challenge values than the ones checked with"""
    ch = cases.challenges_for(pc)
    out = [(ch, v, columns_of(pc, ch, v)) for v in ((0, 1, 2, BAD) if name in shuffle_circuits.SMALL else (0, 1))]
    if name in ("three_phase", "rlc"):
        out.append((ch, 0, columns_of(pc, cases.challenges_for(pc, 9), 0)))
    return out


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_gates_lookups_and_copies_are_check_enum_s(name):
    pc = CIRCUITS[name]()
    seen_failure = False
    for ch, variant, adv in witnesses(pc, name):
        totals, recs = failures4(pc.cs, pc.asg, adv, instance_of(pc, variant), ch)
        want = check_enum.failures(substituted(pc.cs, ch), assignment(pc, adv, variant))
        assert totals[:3] == want[0] and [r for r in recs if r[0] != SHUFFLE] == want[1]
        seen_failure |= sum(want[0]) > 0
    assert seen_failure == (name in ("three_phase", "rlc"))


@pytest.mark.parametrize("name", sorted(shuffle_circuits.SMALL))
def test_shuffle_failures_iff_the_product_does_not_close(name):
    pc = shuffle_circuits.SMALL[name]()
    rng = random.Random(31)
    for ch, variant, adv in witnesses(pc, name):
        totals, recs = failures4(pc.cs, pc.asg, adv, instance_of(pc, variant), ch)
        assert (totals[SHUFFLE] == 0) == (variant != BAD)
        at = shuffle_circuits.cell_at(pc, adv, ch)
        for j in range(len(pc.cs.shuffles)):
            clean = not any(r[0] == SHUFFLE and r[1] == j for r in recs)
            closes = [proof_ref.shuffle_product(pc.cs, j, at, rng.randrange(R), rng.randrange(R))[pc.usable] == 1 for _ in range(2)]
            assert closes == [clean, clean], (variant, j)


def test_records_are_ordered_and_name_the_row_met():
    pc, adv = cases.cascade()
    totals, recs = failures4(pc.cs, pc.asg, adv, [], [])
    assert recs == sorted(recs) and totals[SHUFFLE] == len(recs)
    ins, shs = pc.cs.shuffles[1]
    for kind, j, a, zero, b in recs:
        assert (kind, j, zero) == (SHUFFLE, 1, 0) and a < pc.usable and b < pc.usable and adv[1][a] != adv[2][b]


def test_the_capped_cases_of_the_gpu_test_cap_below_the_total():
    """a test that caps a report must not hide a failure: per witness capped on the GPU, every shuffle's failures stay
    within the usable rows, the caps the test takes for cutting ones are below the total, and every cap the GPU test uses
    beside them is the total or above"""
    capped = [(shuffle_circuits.SMALL[name](), None) for name in sorted(shuffle_circuits.SMALL)] + [cases.cascade()]
    for i, (pc, adv) in enumerate(capped):
        ch = cases.challenges_for(pc)
        totals, recs = report(pc, ch, BAD) if adv is None else report(pc, ch, 0, adv)
        total = sum(totals)
        assert 1 <= totals[SHUFFLE] <= pc.usable * len(pc.cs.shuffles)
        for j in range(len(pc.cs.shuffles)):
            assert sum(1 for r in recs if r[0] == SHUFFLE and r[1] == j) <= pc.usable
        cutting = [cap for cap in cases.CAPS if cap < total]
        assert 0 in cutting
        if adv is not None:  # the cascade: every cap of CAPS cuts
            assert cutting == list(cases.CAPS) and total > 7
    for name, k in cases.SIZES:  # (these run with cap = total + 5: nothing is cut)
        pc = cases.circuit(name, k)
        assert sum(report(pc, (), BAD)[0]) >= 1


def test_the_adversarial_columns_are_what_their_names_say():
    got = {name: failures4(cases.shuffle_circuits.plain(k).cs, cases.shuffle_circuits.plain(k).asg, adv, [], []) for name, (k, adv) in cases.plain_cases().items()}
    assert got["swap_across_chunks"] == ([0, 0, 0, 0], [])
    for k in (5, 11):
        u = shuffle_circuits.plain(k).usable
        assert got["one_above_k%d" % k] == ([0, 0, 0, 1], [(SHUFFLE, 0, u - 1, 0, u // 2)])
        assert got["one_below_k%d" % k] == ([0, 0, 0, 1], [(SHUFFLE, 0, 0, 0, u // 2)])
    assert got["top_limb"][0][SHUFFLE] >= 1 and got["low_limb"][0][SHUFFLE] >= 1
