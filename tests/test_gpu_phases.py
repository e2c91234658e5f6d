"""Advice phases and challenges on the device: zg_prover_set_phases / zg_prover_prove_phased / zg_verifier_set_phases and
the ZG_CHALLENGE query kind.  The oracle knows no challenges, so the judge is tests/proof_ref.py,
the Python-integer verify_proof (pinned to the oracle on one-phase circuits by tests/test_phases_host.py and to recorded
proofs with phases by tests/test_proof_golden_host.py),
next to the library's own batch verifier.  Circuits: tests/phases_circuits.py, k = 5 except the one k = 14 case."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401 -- before the first HIP call of the process (tests/conftest.py)

import phases_circuits
import proof_ref
from circuit import R
from circuits import toy_circuit

pytestmark = pytest.mark.gpu

GWC, SHPLONK, EVM, BLAKE2B = 0, 1, 0, 1
TWO_PHASE = ["rlc", "shuffle", "interleaved", "three_phase"]


class Setup:
    """prover + verifier (both told the phases) + the reference's key for one phased circuit"""

    def __init__(self, orc, zg, ctx, pc, seed=0xABCDEF, vk=0x1234567, set_phases=True):
        self.pc, self.cs = pc, pc.cs
        self.img = pc.cs.to_c()
        self.params = orc.params_new(pc.cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        fixed, sigma = pc.fixed_values(), pc.sigma_values()
        self.prover = zg.Prover(ctx, self.img, fixed, sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr)
        fc, sc = self.prover.vk_commitments()
        self.verifier = zg.Verifier(ctx, self.img, fc, sc, self.params.g_np()[0], np.array(self.params.g2, np.uint64),
                                    np.array(self.params.s_g2, np.uint64), self.vk_repr)
        if set_phases:
            self.prover.set_phases(pc.advice_phase, pc.challenge_phase)
            self.verifier.set_phases(pc.advice_phase, pc.challenge_phase)
        self.vk = proof_ref.Vk(pc.cs, self.params, fixed, sigma, self.vk_repr)

    def prove(self, variants, seeds, seen=None, prover=None):
        p = prover or self.prover
        proofs, st = p.prove_phased(self.pc.synthesize(variants, seen), [self.pc.instance(v) for v in variants], seeds)
        assert st == 0
        return proofs

    def ref(self, proof, variant=0, instance=None, scheme=GWC, transcript=EVM):
        inst = self.pc.instance(variant) if instance is None else instance
        return proof_ref.verify(self.vk, [inst], proof, advice_phase=self.pc.advice_phase, challenge_phase=self.pc.challenge_phase,
                                scheme=scheme, transcript=transcript)

    def dev(self, proofs, variants=None, instances=None):
        insts = instances if instances is not None else [self.pc.instance(v) for v in (variants or [0] * len(proofs))]
        return self.verifier.verify(proofs, insts, 0xFEED)

    def close(self):
        self.verifier.close()
        self.prover.close()


def scalar_offset(cs):
    S = proof_ref.n_sets(cs)
    return 64 * (cs.n_advice + 3 * len(cs.lookups) + S + 1 + cs.degree() - 1)


def flip(proof, at):
    b = bytearray(proof)
    b[at] ^= 1
    return bytes(b)


# ---------------------------------------------------------------------------------------------- acceptance and rejection
@pytest.mark.parametrize("name", sorted(phases_circuits.SMALL))
def test_proofs_are_accepted_and_tampered_ones_rejected(ctx, zg, orc, name):
    pc = phases_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    assert s.prover.phases == (pc.n_phases, pc.advice_phase, pc.challenge_phase) == s.verifier.phases
    (proof,) = s.prove([0], [7])
    assert len(proof) == proof_ref.proof_len(pc.cs) <= s.prover.proof_cap
    r = s.ref(proof)
    assert r.verdict == 1 and sorted(r.challenges) == list(range(len(pc.challenge_phase)))
    assert s.dev([proof]) == [1]
    if pc.n_phases == 1:  # the plain entry: the witness cannot depend on a challenge
        assert s.prover.prove(pc.full_advice([0] * len(pc.challenge_phase)), pc.instance(0), 7) == proof
    # a byte of the LAST phase's first commitment, of an advice evaluation, and a wrong instance
    first_of_last = sum(1 for ph in pc.advice_phase if ph < pc.n_phases - 1)
    for bad in (flip(proof, 64 * first_of_last + 40), flip(proof, scalar_offset(pc.cs) + 31)):
        assert s.ref(bad).verdict <= 0 and s.dev([bad])[0] <= 0
    if pc.cs.n_instance:
        wrong = pc.instance(0).copy()
        wrong[0, 0] = orc.fr_from_int(5)
        assert s.ref(proof, instance=wrong).verdict <= 0 and s.dev([proof], instances=[wrong])[0] <= 0
    # a batch of verdicts: each is its own
    assert s.dev([proof, flip(proof, scalar_offset(pc.cs) + 31), proof]) == [1, 0, 1]
    s.close()


@pytest.mark.parametrize("name", ["rlc", "interleaved"])
def test_a_verifier_without_the_phases_rejects(ctx, zg, orc, name):
    pc = phases_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    (proof,) = s.prove([0], [3])
    assert s.dev([proof]) == [1]
    fc, sc = s.prover.vk_commitments()
    plain = zg.Verifier(ctx, s.img, fc, sc, s.params.g_np()[0], np.array(s.params.g2, np.uint64), np.array(s.params.s_g2, np.uint64),
                        s.vk_repr)
    assert plain.phases == (1, [0] * pc.cs.n_advice, [0] * len(pc.challenge_phase))
    assert plain.verify([proof], [pc.instance(0)], 1)[0] <= 0
    assert proof_ref.verify(s.vk, [pc.instance(0)], proof, advice_phase=None, challenge_phase=[0] * len(pc.challenge_phase)).verdict <= 0
    plain.close()
    s.close()


# ---------------------------------------------------------------------------------------------- the callback's challenges, batches
@pytest.mark.parametrize("name", ["rlc", "three_phase"])
def test_callback_challenges_batches_and_determinism(ctx, zg, orc, name):
    pc = phases_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    s.prover.set_batch(3)
    variants, seeds, seen = [0, 1, 2], [11, 12, 13], []
    proofs = s.prove(variants, seeds, seen)
    assert [ph for ph, _ in seen] == list(range(pc.n_phases))
    assert all(c == 0 for b in seen[0][1] for c in b)  # nothing is squeezed before phase 0
    for b in range(3):
        r = s.ref(proofs[b], variants[b])
        assert r.verdict == 1
        for ph, ch in seen:
            for j, phj in enumerate(pc.challenge_phase):  # squeezed behind an earlier phase: the value; else zero
                assert ch[b][j] == (r.challenges[j] if phj < ph else 0), (b, ph, j)
    assert len({tuple(ch[b]) for _, ch in seen[-1:] for b in range(3)}) == 3  # (the witnesses differ, so do the challenges)
    assert s.dev(proofs, variants) == [1, 1, 1]
    assert s.prove(variants, seeds) == proofs                                        # the same keys, the same bytes
    assert [s.prove([v], [sd])[0] for v, sd in zip(variants, seeds)] == proofs      # a batch is its single calls
    for overlap in (False, True):                                                    # both scheduling forms
        s.prover.set_overlap(overlap)
        assert s.prove(variants, seeds) == proofs
    child_ctx = zg.Ctx(0)
    child = s.prover.fork(child_ctx)                                                 # a fork inherits the phases
    assert child.phases == s.prover.phases
    assert s.prove(variants, seeds, prover=child) == proofs
    child.close()
    child_ctx.close()
    s.close()


# ---------------------------------------------------------------------------------------------- the order of the commitments
def read_slot(prover, slot=0):
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.zeros((prover.n_advice, prover.n, 4), np.uint64)
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(prover.advice_slot(slot)), ctypes.c_size_t(out.nbytes), 2) == 0
    return out


@pytest.mark.parametrize("name", ["interleaved", "three_phase"])
def test_each_commitment_is_its_column_at_its_phases_place(ctx, zg, orc, name):
    pc = phases_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    (proof,) = s.prove([1], [21])
    r = s.ref(proof, 1)
    assert r.verdict == 1 and r.order == proof_ref.advice_order(pc.cs, 1, pc.advice_phase)
    cols = read_slot(s.prover)  # as committed: the blinding rows included
    gl = s.params.g_lagrange_np()
    for (ph, _, col) in r.order:
        want = orc.msm(np.ascontiguousarray(cols[col]), gl, threads=16)
        assert np.array_equal(proof_ref.affine(r.advice[ph, 0, col]), proof_ref.affine(want)), (ph, col)
    assert cols[:, pc.usable:].any()  # (the blinding rows are drawn)
    # the usable rows are the callback's witness for the challenges the proof replays
    ch = [r.challenges[j] for j in range(len(pc.challenge_phase))]
    for ph in range(pc.n_phases):
        seen = [c if pc.challenge_phase[j] < ph else 0 for j, c in enumerate(ch)]
        for col, vals in pc.witness(ph, seen, 1).items():
            assert [orc.fr_to_int(v) for v in cols[col][:pc.usable]] == vals[:pc.usable], (ph, col)
    s.close()


# ---------------------------------------------------------------------------------------------- transcripts and multi-opens
@pytest.mark.parametrize("name", ["rlc", "three_phase"])
@pytest.mark.parametrize("scheme,transcript", [(GWC, EVM), (SHPLONK, EVM), (GWC, BLAKE2B), (SHPLONK, BLAKE2B)])
def test_every_multiopen_and_transcript(ctx, zg, orc, name, scheme, transcript):
    pc = phases_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    for obj in (s.prover, s.verifier):
        obj.set_multiopen(scheme)
        obj.set_transcript(transcript)
    (proof,) = s.prove([0], [5])
    assert len(proof) == proof_ref.proof_len(pc.cs, scheme=scheme, transcript=transcript) <= s.prover.proof_cap
    assert s.ref(proof, scheme=scheme, transcript=transcript).verdict == 1
    assert s.dev([proof]) == [1]
    bad = flip(proof, len(proof) - 40)
    assert s.ref(bad, scheme=scheme, transcript=transcript).verdict <= 0 and s.dev([bad])[0] <= 0
    s.close()


# ---------------------------------------------------------------------------------------------- the fill kernel, the split domain
def test_pseudo_columns_hold_the_constant_on_every_part(ctx, zg, orc):
    """rlc with its degree-6 gate at k = 5: the single coset in the latency form, the split 4n + n domain in the throughput form"""
    pc = phases_circuits.rlc(5, high_gate=True)
    assert pc.cs.degree() == 6
    s = Setup(orc, zg, ctx, pc)
    qt = s.prover.quotient_terms()
    assert qt["active"] and qt["gates"] == [0, 0, 1]  # one low and one high gate read the challenge
    assert qt["part2"][pc.cs.n_advice + pc.cs.n_instance] == 1  # ... so its slab is wanted on the second part
    n, ek = pc.n, pc.cs.extended_k()
    s.prover.set_batch(2)
    proofs = {}
    for overlap in (True, False):
        s.prover.set_overlap(overlap)
        proofs[overlap] = s.prove([0, 1], [31, 32])
        for b in range(2):
            r = s.ref(proofs[overlap][b], b)
            assert r.verdict == 1
            c = orc.fr_from_int(r.challenges[0])
            const = np.zeros((n, 4), np.uint64)
            const[0] = c
            assert np.array_equal(s.prover.fetch(6, 0, n, slot=b), np.tile(c, (n, 1)))
            assert np.array_equal(s.prover.fetch(7, 0, n, slot=b), const)
            if overlap:
                want = ctx.coeff_to_extended(const, pc.cs.k, ek)
                assert np.array_equal(want, np.tile(c, (1 << ek, 1)))  # (the constant polynomial is the constant on any coset)
                assert np.array_equal(s.prover.fetch(8, 0, 1 << ek, slot=b), want)
                for what in (9, 10):
                    with pytest.raises(zg.ZgError):
                        s.prover.fetch(what, 0, 4 * n, slot=b)
            else:
                assert np.array_equal(s.prover.fetch(9, 0, 4 * n, slot=b), np.tile(c, (4 * n, 1)))
                assert np.array_equal(s.prover.fetch(10, 0, n, slot=b), np.tile(c, (n, 1)))
                with pytest.raises(zg.ZgError):
                    s.prover.fetch(8, 0, 1 << ek, slot=b)
    assert proofs[True] == proofs[False]
    s.prover.set_quotient_terms(False)  # every term on both parts
    assert s.prove([0, 1], [31, 32]) == proofs[True]
    s.prover.set_quotient_terms(True)
    assert s.dev(proofs[True], [0, 1]) == [1, 1]
    with pytest.raises(zg.ZgError):
        s.prover.fetch(6, 1, n)  # the circuit has one challenge
    s.close()
    # ZG_SPLIT_DOMAIN off: the throughput form on the single coset, the same bytes
    zg.tuning_set("ZG_SPLIT_DOMAIN", 0)
    try:
        s2 = Setup(orc, zg, ctx, pc)
        s2.prover.set_batch(2)
        s2.prover.set_overlap(False)
        assert s2.prove([0, 1], [31, 32]) == proofs[True]
        s2.close()
    finally:
        zg.tuning_set("ZG_SPLIT_DOMAIN", -1)


def test_rlc_at_k14_on_the_split_domain_by_degree(ctx, zg, orc):
    pc = phases_circuits.rlc_k14()
    orc.load().orc_set_threads(16)
    s = Setup(orc, zg, ctx, pc, seed=0x5EED)
    qt = s.prover.quotient_terms()
    assert qt["active"] and qt["gates"] == [0, 0, 1]
    s.prover.set_overlap(False)  # the throughput form: 4n + n points, the terms by degree
    (proof,) = s.prove([0], [41])
    assert s.ref(proof).verdict == 1 and s.dev([proof]) == [1]
    s.prover.set_quotient_terms(False)
    assert s.prove([0], [41]) == [proof]
    s.prover.set_quotient_terms(True)
    s.prover.set_overlap(True)
    assert s.prove([0], [41]) == [proof]
    s.close()


# ---------------------------------------------------------------------------------------------- unchanged without challenges
def test_a_circuit_without_challenges_is_untouched(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(5)
    img = cs.to_c()
    params = orc.params_new(cs.k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x1234567)
    pk = orc.ProvingKey(img, asg.fixed_values(), asg.sigma_values(), params, vk_repr)
    prover = zg.Prover(ctx, img, asg.fixed_values(), asg.sigma_values(), params.g_np(), params.g_lagrange_np(), vk_repr)
    assert prover.phases == (1, [0] * cs.n_advice, [])
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    calls = []

    def one_phase(phase, ch):
        calls.append((phase, ch.shape))
        return [{c: adv[c] for c in range(cs.n_advice)}]

    want = orc.create_proof(pk, adv, inst, 7)[1]
    assert prover.prove(adv, inst, 7) == want  # (a first proof makes twiddle tables: not part of the comparison below)
    ctx.profile(True)
    try:
        ctx.profile_collect()
        got, st = prover.prove_phased(one_phase, [inst], [7])
        phased_profile = ctx.profile_collect()
        assert prover.prove(adv, inst, 7) == want
        plain_profile = ctx.profile_collect()
    finally:
        ctx.profile(False)
    assert st == 0 and got == [want] and calls == [(0, (1, 0, 4))]
    assert "challenge_fill" not in phased_profile and "challenge_fill" not in plain_profile
    launches = lambda prof: {k: v[0] for k, v in prof.items()}  # noqa: E731
    assert launches(phased_profile) == launches(plain_profile)  # the identical launch sequence, counted by kernel
    prover.set_phases([0] * cs.n_advice, [])  # saying "one phase" changes nothing
    assert prover.prove(adv, inst, 7) == want
    prover.close()
    # ... and a circuit with a challenge does launch the kernel, once per phase that squeezes one it uses
    pc = phases_circuits.three_phase()
    s = Setup(orc, zg, ctx, pc)
    ctx.profile(True)
    try:
        ctx.profile_collect()
        s.prove([0], [1])
        prof = ctx.profile_collect()
    finally:
        ctx.profile(False)
    assert prof["challenge_fill"][0] == 3
    s.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_prover_working(ctx, zg, orc):
    pc = phases_circuits.rlc()
    s = Setup(orc, zg, ctx, pc)
    s.prover.set_batch(2)
    (proof,) = s.prove([0], [9])
    before = s.prover.phases

    def refused(fn, status):
        with pytest.raises(zg.ZgError) as e:
            fn()
        assert e.value.status == status, str(e.value)
        return str(e.value)

    # zg_prover_set_phases / zg_verifier_set_phases: a phase 3, a gap, too few challenges, a challenge behind a phase nobody has
    for obj in (s.prover, s.verifier):
        for adv, ch in (([0, 0, 3], [0]), ([0, 0, 2], [0]), ([0, 0, 1], []), ([0, 0, 1], [2]), ([0, 0, 1], [0] * 17)):
            refused(lambda: obj.set_phases(adv, ch), -1)
        assert obj.phases == before
    inst, adv = pc.instance(0), pc.full_advice([5])
    # the plain entries on a circuit with a later-phase column
    assert "zg_prover_prove_phased" in refused(lambda: s.prover.prove(adv, inst, 9), -1)
    assert "zg_prover_prove_phased" in refused(lambda: s.prover.prove_batch([adv, adv], [inst, inst], [1, 2]), -1)
    # out of scope on a circuit with a challenge
    refused(lambda: s.prover.prove_multi([adv, adv], [inst, inst], [1, 2]), -4)
    refused(lambda: s.prover.check_batch([adv], [inst]), -4)
    refused(lambda: s.verifier.verify_multi([proof], [[inst, inst]], 1, 2), -4)
    refused(lambda: s.prover.set_shard(0, 2, 0, lambda send, recv: None), -4)
    # (no plan is at hand for this circuit -- the witness program has no field operand -- and none is needed: the refusal
    #  comes before anything is asked of the other arguments)
    assert ctx.lib.zg_prover_prove_images(s.prover.h, None, None, ctypes.c_size_t(1), None, None, ctypes.c_size_t(0), None, None, None) == -4
    # a callback that gives up
    out, st = s.prover.prove_phased(lambda phase, ch: 1 // 0, [inst], [9], raise_on_error=False)
    assert st == -1 and out == [b""]
    calls = []

    def stops_in_phase_1(phase, ch):
        calls.append(phase)
        if phase == 1:
            raise RuntimeError("no witness")
        return pc.synthesize([0])(phase, ch)

    out, st = s.prover.prove_phased(stops_in_phase_1, [inst], [9], raise_on_error=False)
    assert st == -1 and out == [b""] and calls == [0, 1]
    # ... and after all of it the prover proves what it proved before
    assert s.prove([0], [9]) == [proof] and s.dev([proof]) == [1]
    s.close()
    # a circuit with a challenge but one phase: the plain entries work, the out-of-scope ones are refused all the same
    g = phases_circuits.gates_only_challenge()
    sg = Setup(orc, zg, ctx, g)
    ga = g.full_advice([0])
    p0 = sg.prover.prove(ga, g.instance(0), 3)
    refused(lambda: sg.prover.check_batch([ga], [g.instance(0)]), -4)
    assert sg.prover.prove(ga, g.instance(0), 3) == p0 and sg.dev([p0]) == [1]
    sg.close()
