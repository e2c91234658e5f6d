"""The lookup argument on adversarial columns at multi-chunk sizes: the prover's sort and permute (csrc/sort.hip), the
run-form commitment digits of a' and s' (csrc/msm.hip) and the checker's sort and search (csrc/check.hip).

The circuits are lookup-only (tests/lookup_cases.py), so a proof costs little beside its lookup argument, and the columns
are the value families of that file: all-equal inputs, inputs without a repeat, runs that end at / next to the 1024-row
chunk and tile boundaries, keys that differ in one limb, gaps at every digit-window boundary, the (r - 1) / 2 boundary of
the run form's sign decision.  Sizes: k = 10 is one LDS chunk and one scan tile (the control), k = 11 .. 14 add one fused
global sort level and one more scan tile each.

Every comparison is exact: stage arrays and proof bytes against the oracle, whose a' / s' are in turn compared with
permute_ref on Python integers here and in tests/test_lookup_cases_host.py; check reports against tests/check_enum.py."""
import numpy as np
import pytest

import lookup_cases as lc
from check_enum import LOOKUP, changed
from check_enum import failures as report
from circuit import ADVICE, R

pytestmark = pytest.mark.gpu

CLEAN = ([0, 0, 0], [])
FORMS = (True, "tables", False)  # latency form, latency form over digit tables, throughput form
SEEDS = (1, 2)


class Case:
    """one circuit and witness, the oracle's key, its proofs and traces for SEEDS, and the integer reference"""

    def __init__(self, orc, params, k, cs, asg, pairs):
        self.k, self.cs, self.asg, self.pairs = k, cs, asg, pairs
        self.n, self.usable = 1 << k, cs.usable_rows()
        self.img = cs.to_c()
        self.params = params
        self.vk_repr = orc.fr_from_int(0x1234567)
        self.fixed, self.sigma = asg.fixed_values(), asg.sigma_values()
        self.g, self.gl = params.g_np(), params.g_lagrange_np()
        self.pk = orc.ProvingKey(self.img, self.fixed, self.sigma, params, self.vk_repr)
        self.adv, self.inst = asg.advice_values(), asg.instance_values(0)
        self.want, self.trace = {}, {}
        nl = len(pairs)
        for seed in SEEDS:
            st, proof, tr = orc.create_proof(self.pk, self.adv, self.inst, seed, want_trace=True)
            assert st == 0
            self.want[seed] = proof
            self.trace[seed] = dict(a=tr.array("permuted_input", nl * self.n), s=tr.array("permuted_table", nl * self.n),
                                    z=tr.array("lookup_z", nl * self.n), theta=orc.fr_to_int(tr.fe("theta")))
            orc.trace_free(tr)
        # the oracle's own a' / s' against Python integers, once (seed 1's theta compresses a wide lookup)
        theta = self.trace[1]["theta"]
        self.ref = [lc.permute_ref(lc.compress(ins, theta), lc.compress(tabs, theta)) for ins, tabs in pairs]
        for l, (a, s) in enumerate(self.ref):
            at = slice(l * self.n, l * self.n + self.usable)
            assert lc.from_mont_array(self.trace[1]["a"][at]) == a and lc.from_mont_array(self.trace[1]["s"][at]) == s, "oracle"

    def prover(self, zg, ctx):
        return zg.Prover(ctx, self.img, self.fixed, self.sigma, self.g, self.gl, self.vk_repr)


@pytest.fixture(scope="module")
def cases(orc):
    """cases(key, build): the Case of `key`, made once for the module; build(params_of_k) -> Case arguments"""
    orc.load().orc_set_threads(16)
    memo, params = {}, {}

    def params_of(k):
        if k not in params:
            params[k] = orc.params_new(k, 0xABCDEF)
        return params[k]

    def get(key, k, build):
        if key not in memo:
            cs, asg, pairs = build()
            memo[key] = Case(orc, params_of(k), k, cs, asg, pairs)
        return memo[key]

    return get


def family_case(cases, k, name):
    def build():
        table, inputs = lc.make(name, k)
        cs, asg, _ = lc.lookup_circuit(k, table, inputs)
        return cs, asg, [([inputs], [table])]

    return cases((k, name), k, build)


def stages_forms_and_check(zg, ctx, orc, c, forms=FORMS):
    """The order names the stage that went wrong: a', s', the product, then the bytes (the commitments of a' and s' are in
    them: the run-form digits), in each scheduling form, then the witness check."""
    prover = c.prover(zg, ctx)
    try:
        n, usable = c.n, c.usable
        prover.set_overlap(True)
        got = prover.prove(c.adv, c.inst, 1)
        tr = c.trace[1]
        for l in range(len(c.pairs)):
            at = slice(l * n, (l + 1) * n)
            a, s = prover.fetch(3, l, n), prover.fetch(4, l, n)
            assert lc.from_mont_array(a[:usable]) == c.ref[l][0], ("a' against permute_ref", l)
            assert np.array_equal(a, tr["a"][at]), ("a'", l)
            assert lc.from_mont_array(s[:usable]) == c.ref[l][1], ("s' against permute_ref", l)
            assert np.array_equal(s, tr["s"][at]), ("s'", l)
            assert np.array_equal(prover.fetch(2, l, n), tr["z"][at]), ("lookup z", l)
        assert got == c.want[1], "proof bytes, latency form"
        for form in forms:
            prover.set_overlap(form)
            for seed in SEEDS:
                got = prover.prove(c.adv, c.inst, seed)
                assert got == c.want[seed], ("proof bytes", form, seed)
            assert orc.verify_proof_pairing(c.pk, c.inst, got) == 1, form
        assert prover.check(c.adv, c.inst) == CLEAN
    finally:
        prover.close()


# ---------------------------------------------------------------- 1. every family at every sort depth
SIZES = [(k, name) for k in (10, 11, 12, 13) for name in lc.FAMILIES] + [(14, "runs"), (14, "zipf")]


@pytest.mark.parametrize("k,name", SIZES, ids=[f"k{k}-{name}" for k, name in SIZES])
def test_family_stages_bytes_and_check(ctx, zg, orc, cases, k, name):
    stages_forms_and_check(zg, ctx, orc, family_case(cases, k, name))


# ---------------------------------------------------------------- 2. both recodings of the run form
RECODINGS = {"default": {}, "window_form": {"ZG_MSM_NAF_GL": 0}, "no_runs": {"ZG_MSM_RUNS": 0}}


@pytest.mark.parametrize("recoding", list(RECODINGS))
@pytest.mark.parametrize("name", ["pow2_gaps", "half_r", "limbs"])
def test_run_form_recodings_give_the_oracles_bytes(ctx, zg, orc, cases, name, recoding):
    """ZG_MSM_NAF_GL at its default recodes the run-form coefficients at free positions (msm_digits_naf_kernel), 0 in
    windows (msm_digits_kernel, with its t * r balancing of large values); ZG_MSM_RUNS = 0 is the control without the
    run form.  The knob is set before the prover exists: it shapes the prover's tables."""
    c = family_case(cases, 12, name)
    knobs = RECODINGS[recoding]
    before = {kn: zg.tuning_get(kn) for kn in knobs}
    try:
        for kn, v in knobs.items():
            zg.tuning_set(kn, v)
        prover = c.prover(zg, ctx)
        for form in FORMS:
            prover.set_overlap(form)
            for seed in SEEDS:
                assert prover.prove(c.adv, c.inst, seed) == c.want[seed], (name, recoding, form, seed)
        prover.close()
    finally:
        for kn, v in before.items():
            zg.tuning_set(kn, v)


# ---------------------------------------------------------------- 3. a batch whose slots differ
SLOTS = ("all_equal", "permutation", "runs", "half_r")
BATCH_K = 12


class Batch:
    def __init__(self, orc, cases):
        k = BATCH_K
        self.table = lc.shared_table(k)
        self.inputs = [lc.make(name, k, table=self.table)[1] for name in SLOTS]

        def build():
            cs, asg, _ = lc.lookup_circuit(k, self.table, self.inputs[0])
            return cs, asg, [([self.inputs[0]], [self.table])]

        self.c = cases(("batch", k), k, build)
        self.cs = self.c.cs
        self.asgs = [self.c.asg] + [changed(self.c.asg, [(ADVICE, 0, r, v) for r, v in enumerate(inp)]) for inp in self.inputs[1:]]
        self.advs = [a.advice_values() for a in self.asgs]
        self.insts = [self.c.inst] * len(SLOTS)
        self.seeds = [11, 12, 13, 14]
        self.ref = [lc.permute_ref(inp, self.table) for inp in self.inputs]
        self.want = []
        for adv, seed in zip(self.advs, self.seeds):
            st, proof, _ = orc.create_proof(self.c.pk, adv, self.c.inst, seed)
            assert st == 0
            self.want.append(proof)


@pytest.fixture(scope="module")
def batch(orc, cases):
    return Batch(orc, cases)


def test_batch_of_different_slots_equals_oracle_and_lone_proofs(ctx, zg, orc, batch):
    """m = nb * NL = 4 rows of the batched sort, each with another run structure: m_rep = usable - 1, 0, the boundary runs,
    usable - 5"""
    prover = batch.c.prover(zg, ctx)
    try:
        prover.set_batch(4)
        for form in (False, True):
            prover.set_overlap(form)
            got, sts = prover.prove_batch(batch.advs, batch.insts, batch.seeds)
            assert sts == [0, 0, 0, 0], form
            for b, name in enumerate(SLOTS):
                assert got[b] == batch.want[b], ("batch slot against the oracle", form, name)
                a, s = batch.ref[b]
                n, usable = batch.c.n, batch.c.usable
                assert lc.from_mont_array(prover.fetch(3, 0, n, slot=b)[:usable]) == a, ("a'", form, name)
                assert lc.from_mont_array(prover.fetch(4, 0, n, slot=b)[:usable]) == s, ("s'", form, name)
            for b, name in enumerate(SLOTS):
                assert prover.prove(batch.advs[b], batch.c.inst, batch.seeds[b]) == got[b], ("lone proof", form, name)
        assert prover.check_batch(batch.advs, batch.insts) == [CLEAN] * 4
    finally:
        prover.close()


def missing_values(table):
    """values the table lacks, by where the search for them ends (the shared table holds 0, 1, r - 2 and r - 1: nothing
    is below or above ALL of it, so the first two are the smallest and the largest value it lacks)"""
    have = set(table)
    low = next(v for v in range(R) if v not in have)
    high = next(v for v in range(R - 1, 0, -1) if v not in have)
    plain = [v for v in table if v not in lc.HALF_R_VALUES]
    limb7 = next(v ^ (1 << 224) for v in plain if v ^ (1 << 224) < R and v ^ (1 << 224) not in have)
    limb0 = next(v ^ 1 for v in plain if v ^ 1 not in have)
    return {"low": low, "high": high, "limb7": limb7, "limb0": limb0}


@pytest.mark.parametrize("kind", ["low", "high", "limb7", "limb0"])
def test_one_bad_slot_fails_alone(ctx, zg, orc, batch, kind):
    v = missing_values(batch.table)[kind]
    assert v not in set(batch.table) and 0 <= v < R
    if kind == "limb7":
        assert any(lc.limbs(t)[:7] == lc.limbs(v)[:7] for t in batch.table)
    if kind == "limb0":
        assert any(lc.limbs(t)[1:] == lc.limbs(v)[1:] for t in batch.table)
    row = 2500
    asgs = list(batch.asgs)
    asgs[2] = changed(asgs[2], [(ADVICE, 0, row, v)])
    advs = [a.advice_values() for a in asgs]
    want_reports = [report(batch.cs, a) for a in asgs]
    assert want_reports == [CLEAN, CLEAN, ([0, 1, 0], [(LOOKUP, 0, row, 0, 0)]), CLEAN]
    st, _, _ = orc.create_proof(batch.c.pk, advs[2], batch.c.inst, batch.seeds[2])
    assert st == -5
    prover = batch.c.prover(zg, ctx)
    try:
        prover.set_batch(4)
        prover.set_overlap(False)
        got, sts = prover.prove_batch(advs, batch.insts, batch.seeds, raise_on_error=False)
        assert sts == [0, 0, -5, 0], kind
        for b in (0, 1, 3):
            assert got[b] == batch.want[b], (kind, b)
        assert prover.check_batch(advs, batch.insts) == want_reports
    finally:
        prover.close()


def test_missing_values_below_and_above_the_whole_table_are_refused(ctx, zg, orc, cases):
    """0 and r - 1 against a table that holds neither: the search ends before the first and behind the last table row"""
    c = family_case(cases, 12, "zipf")
    table = c.pairs[0][1][0]
    assert 0 < min(table) and max(table) < R - 1
    prover = c.prover(zg, ctx)
    try:
        for v, row in ((0, 7), (R - 1, c.usable - 1)):
            bad = changed(c.asg, [(ADVICE, 0, row, v)])
            adv = bad.advice_values()
            assert orc.create_proof(c.pk, adv, c.inst, 1)[0] == -5
            with pytest.raises(zg.ZgError) as e:
                prover.prove(adv, c.inst, 1)
            assert e.value.status == -5
            want = report(c.cs, bad)
            assert want == ([0, 1, 0], [(LOOKUP, 0, row, 0, 0)]) and prover.check(adv, c.inst) == want
        assert prover.prove(c.adv, c.inst, 1) == c.want[1]  # (a refused witness leaves nothing behind)
    finally:
        prover.close()


# ---------------------------------------------------------------- 4. two lookups, a wide lookup
def test_two_lookups_with_different_run_structure(ctx, zg, orc, cases):
    k = 12

    def build():
        (t0, a0), (t1, a1) = lc.make("runs", k), lc.make("permutation", k)
        cs, asg, _ = lc.lookup_circuit(k, [t0, t1], [a0, a1], lookups=2)
        return cs, asg, [([a0], [t0]), ([a1], [t1])]

    c = cases(("two", k), k, build)
    assert len(c.cs.lookups) == 2
    stages_forms_and_check(zg, ctx, orc, c)


def wide(cases, k=12):
    def build():
        tabs, ins = lc.wide_case(k)
        cs, asg, _ = lc.lookup_circuit(k, tabs, ins, width=2)
        return cs, asg, [(list(ins), list(tabs))]

    return cases(("wide", k), k, build)


def test_wide_lookup_with_ties_on_the_first_element(ctx, zg, orc, cases):
    stages_forms_and_check(zg, ctx, orc, wide(cases))


def test_wide_lookup_tuple_that_ties_on_the_first_element_and_misses_on_the_second(ctx, zg, orc, cases):
    """One changed cell of the second input column: its tuple ties table tuples on the first element and misses on the
    second in the top limb only -- of the canonical value in one case, of the Montgomery representative (what the checker
    compares) in the other."""
    c = wide(cases)
    (a0, a1), (t0, t1) = c.pairs[0]
    have = set(zip(t0, t1))
    row = 3000
    mont_top = (1 << 224) * lc.RINV % R  # adding it adds 2^224 to the Montgomery representative
    cands = {"canonical": [a1[row] ^ (1 << 224), a1[row] ^ (3 << 224)], "montgomery": [(a1[row] + mont_top) % R, (a1[row] - mont_top) % R]}
    prover = c.prover(zg, ctx)
    try:
        for which, vs in cands.items():
            rep = (lambda x: x) if which == "canonical" else (lambda x: x * (1 << 256) % R)
            v = next(x for x in vs if x < R and (a0[row], x) not in have and lc.limbs(rep(x))[:7] == lc.limbs(rep(a1[row]))[:7])
            assert rep(v) != rep(a1[row]) and any(t == a0[row] for t in t0)
            bad = changed(c.asg, [(ADVICE, 1, row, v)])
            want = report(c.cs, bad)
            assert want == ([0, 1, 0], [(LOOKUP, 0, row, 0, 0)])
            assert prover.check(bad.advice_values(), c.inst) == want, which
        assert prover.check(c.adv, c.inst) == CLEAN
    finally:
        prover.close()


# ---------------------------------------------------------------- 5. a table that is part of the witness
def test_advice_tables_are_sorted_per_witness(ctx, zg, orc, cases):
    k = 12
    ta, ia = lc.make("limbs", k)
    tb, ib = lc.make("one_heavy_table", k)

    def build():
        cs, asg, _ = lc.lookup_circuit(k, ta, ia, advice_table=True)
        return cs, asg, [([ia], [ta])]

    c = cases(("advice_table", k), k, build)
    usable = c.usable
    other = changed(c.asg, [(ADVICE, 0, r, tb[r]) for r in range(usable)] + [(ADVICE, 1, r, ib[r]) for r in range(usable)])
    only_a = next(v for v in ta if v not in set(tb))
    only_b = next(v for v in tb if v not in set(ta))
    bad_a = changed(c.asg, [(ADVICE, 1, 2047, only_b)])
    bad_b = changed(other, [(ADVICE, 1, 1024, only_a)])
    prover = c.prover(zg, ctx)
    try:
        prover.set_batch(2)
        for asgs in ([c.asg, other], [other, c.asg], [bad_a, bad_b], [bad_b, bad_a]):
            want = [report(c.cs, a) for a in asgs]
            got = prover.check_batch([a.advice_values() for a in asgs], [c.inst, c.inst])
            assert got == want
        assert report(c.cs, c.asg) == CLEAN and report(c.cs, other) == CLEAN
        assert report(c.cs, bad_a) == ([0, 1, 0], [(LOOKUP, 0, 2047, 0, 0)])
        assert report(c.cs, bad_b) == ([0, 1, 0], [(LOOKUP, 0, 1024, 0, 0)])
        prover.set_batch(1)
        assert prover.prove(c.adv, c.inst, 1) == c.want[1]
    finally:
        prover.close()
