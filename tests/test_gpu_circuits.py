"""One proof of several circuits for every circuit the library proves (zg_prover_prove_circuits / _dev / _phased,
zg_verifier_verify_circuits): shuffles, challenges and advice phases behind ONE transcript.  The oracle
knows none of the three, so the judge of every proof is tests/proof_ref.py, the Python-integer verify_proof for N circuits
(pinned to recorded proofs of this form by tests/test_circuits_host.py), next to the library's own batch verifier.
Circuits: tests/shuffle_circuits.py and tests/phases_circuits.py at k = 5 except the k = 14 case; circuit c of a proof has
witness variant c and a key of its own -- a circuit's key columns do not depend on the variant.

Tolerances: none -- everything here is exact arithmetic mod r or bytes."""
import ctypes
import random

import numpy as np
import pytest
import torch  # noqa: F401 -- before the first HIP call of the process (tests/conftest.py)

import phases_circuits
import proof_ref
import shuffle_circuits
from circuit import ADVICE
from circuits import toy_circuit
from shuffle_circuits import BAD

pytestmark = pytest.mark.gpu

GWC, SHPLONK, EVM, BLAKE2B = 0, 1, 0, 1
ZG_ERR_INVALID_ARG, ZG_ERR_UNSUPPORTED, ZG_ERR_CONSTRAINT = -1, -4, -5
VARIANTS = [0, 1, 2]


class Setup:
    """prover + verifier (told the circuit's shuffles and phases) + the reference's key, for proofs of up to `slots` circuits"""

    def __init__(self, orc, zg, ctx, pc, slots=3, seed=0xABCDEF, vk=0x1234567, scheme=GWC, transcript=EVM):
        self.pc, self.cs, self.zg, self.orc = pc, pc.cs, zg, orc
        self.scheme, self.transcript = scheme, transcript
        self.img = pc.cs.to_c()
        self.params = orc.params_new(pc.cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        fixed, sigma = pc.fixed_values(), pc.sigma_values()
        shuffles = getattr(self.img, "shuffles", None)
        self.prover = zg.Prover(ctx, self.img, fixed, sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr, shuffles=shuffles)
        fc, sc = self.prover.vk_commitments()
        self.verifier = zg.Verifier(ctx, self.img, fc, sc, self.params.g_np()[0], np.array(self.params.g2, np.uint64),
                                    np.array(self.params.s_g2, np.uint64), self.vk_repr, shuffles=shuffles)
        for obj in (self.prover, self.verifier):
            if scheme != GWC:
                obj.set_multiopen(scheme)
            if transcript != EVM:
                obj.set_transcript(transcript)
            if pc.n_phases > 1 or pc.challenge_phase:
                obj.set_phases(pc.advice_phase, pc.challenge_phase)
        self.prover.set_batch(slots)
        self.phased = pc.n_phases > 1
        self._advice = {}
        self.vk = proof_ref.Vk(pc.cs, self.params, fixed, sigma, self.vk_repr)

    def advice(self, variant):
        if variant not in self._advice:
            self._advice[variant] = self.pc.full_advice([0] * len(self.pc.challenge_phase), variant)
        return self._advice[variant]

    def insts(self, variants):
        return [self.pc.instance(v) for v in variants]

    def prove(self, variants, seeds, seen=None, prover=None) -> bytes:
        """ONE proof of len(variants) circuits, through the entry the circuit needs"""
        p = prover or self.prover
        if self.phased:
            proof, st = p.prove_circuits_phased(self.pc.synthesize(variants, seen), self.insts(variants), seeds)
            assert st == 0
            return proof
        return p.prove_circuits([self.advice(v) for v in variants], self.insts(variants), seeds)

    def ref(self, proof, variants=None, insts=None):
        insts = self.insts(variants) if insts is None else insts
        return proof_ref.verify(self.vk, insts, proof, advice_phase=self.pc.advice_phase, challenge_phase=self.pc.challenge_phase,
                                scheme=self.scheme, transcript=self.transcript)

    def dev(self, proof, variants=None, insts=None, key=0xFEED):
        insts = self.insts(variants) if insts is None else insts
        return self.verifier.verify_circuits([proof], [insts], key, len(insts))[0]

    def accepted(self, proof, variants):
        """length, the reference's verdict and the device's, for a proof that must be accepted"""
        N = len(variants)
        assert len(proof) == proof_ref.proof_len(self.cs, N, self.scheme, self.transcript) <= self.prover.proof_size_multi(N)
        r = self.ref(proof, variants)
        assert r.verdict == 1 and self.dev(proof, variants) == 1
        return r

    def rejected(self, proof, variants=None, insts=None):
        assert self.ref(proof, variants, insts).verdict <= 0 and self.dev(proof, variants, insts) <= 0

    def close(self):
        self.verifier.close()
        self.prover.close()


def flip(proof, at):
    b = bytearray(proof)
    b[at] ^= 1
    return bytes(b)


def offsets(cs, N):
    """byte offsets (EVM transcript, GWC) in a proof of N circuits: the LAST circuit's first shuffle commitment, the last
    evaluation -- the last circuit's last shuffle evaluation where the circuit has shuffles -- and the last circuit's first
    advice evaluation"""
    S, NL, NS = proof_ref.n_sets(cs), len(cs.lookups), len(proof_ref.shuffles_of(cs))
    _, scalars = proof_ref.counts(cs, N, GWC)
    com = 64 * (N * (cs.n_advice + 3 * NL + S) + (N - 1) * NS)
    ev0 = 64 * (N * (cs.n_advice + 3 * NL + S + NS) + 1 + cs.degree() - 1)
    return com, ev0 + 32 * (scalars - 1), ev0 + 32 * (N - 1) * len(cs.advice_queries)


def swapped(insts):
    return [insts[1], insts[0]] + insts[2:]


def read_slot(prover, slot):
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.zeros((prover.n_advice, prover.n, 4), np.uint64)
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(prover.advice_slot(slot)), ctypes.c_size_t(out.nbytes), 2) == 0
    return out


def refused(zg, fn, status):
    with pytest.raises(zg.ZgError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    return str(e.value)


# ---------------------------------------------------------------------------------------------- 1. shuffle circuits
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("name", sorted(shuffle_circuits.SMALL))
def test_shuffle_circuits_are_accepted_and_tampered_proofs_rejected(ctx, zg, orc, name, N):
    pc = shuffle_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc, N)
    variants, seeds = VARIANTS[:N], [7 + c for c in range(N)]
    proof = s.prove(variants, seeds)
    r = s.accepted(proof, variants)
    assert len(r.shuffle_z) == N and sorted(r.challenges) == list(range(len(pc.challenge_phase)))
    com, last_ev, _ = offsets(pc.cs, N)
    s.rejected(flip(proof, com + 40), variants)   # the LAST circuit's first shuffle commitment
    s.rejected(flip(proof, last_ev + 31), variants)  # the last shuffle evaluation
    if pc.cs.n_instance:
        assert s.insts(variants)[0].tobytes() != s.insts(variants)[1].tobytes()
        s.rejected(proof, insts=swapped(s.insts(variants)))
    # ONE shuffled value changed in circuit 1 only: the call succeeds, the proof has full length, nobody accepts it
    spoiled = [0, BAD, 2][:N]
    bad = s.prove(spoiled, seeds)
    assert len(bad) == len(proof)
    assert s.ref(bad, spoiled).verdict == 0 and s.dev(bad, spoiled) == 0
    s.close()


# ---------------------------------------------------------------------------------------------- 2. phased circuits
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("name", sorted(phases_circuits.SMALL))
def test_phased_circuits_callback_order_and_commitments(ctx, zg, orc, name, N):
    pc = phases_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc, N)
    variants, seeds, seen = VARIANTS[:N], [17 + c for c in range(N)], []
    proof, st = s.prover.prove_circuits_phased(pc.synthesize(variants, seen), s.insts(variants), seeds)
    assert st == 0
    r = s.accepted(proof, variants)
    _, last_ev, adv_ev = offsets(pc.cs, N)
    s.rejected(flip(proof, 64 * (N * pc.cs.n_advice - 1) + 40), variants)  # the last circuit's last advice commitment
    s.rejected(flip(proof, adv_ev + 31), variants)                          # the last circuit's first advice evaluation
    s.rejected(flip(proof, last_ev + 31), variants)
    if pc.cs.n_instance:
        assert s.insts(variants)[0].tobytes() != s.insts(variants)[1].tobytes()
        s.rejected(proof, insts=swapped(s.insts(variants)))
    # the callback: once per phase, in order, count = N, every row the one transcript's challenges squeezed so far
    assert [ph for ph, _ in seen] == list(range(pc.n_phases))
    assert sorted(r.challenges) == list(range(len(pc.challenge_phase)))
    for ph, ch in seen:
        assert len(ch) == N and all(row == ch[0] for row in ch), ph
        assert ch[0] == [r.challenges[j] if phj < ph else 0 for j, phj in enumerate(pc.challenge_phase)], ph
    assert r.order == proof_ref.advice_order(pc.cs, N, pc.advice_phase)
    if name in ("rlc", "interleaved"):  # every commitment is its circuit's column, blinding rows included, at its phase's place
        gl = s.params.g_lagrange_np()
        for c in range(N):
            cols = read_slot(s.prover, c)
            assert cols[:, pc.usable:].any()
            for col, ph in enumerate(pc.advice_phase):
                want = orc.msm(np.ascontiguousarray(cols[col]), gl, threads=16)
                assert np.array_equal(proof_ref.affine(r.advice[ph, c, col]), proof_ref.affine(want)), (ph, c, col)
    s.close()


# ---------------------------------------------------------------------------------------------- 3. one circuit
def test_one_circuit_is_the_single_proof(ctx, zg, orc):
    for pc in (shuffle_circuits.three(), phases_circuits.gates_only_challenge()):  # the plain entries
        s = Setup(orc, zg, ctx, pc, 1)
        adv, inst = s.advice(1), pc.instance(1)
        one = s.prover.prove(adv, inst, 7)
        assert len(one) == proof_ref.proof_len(pc.cs) and s.prover.prove_circuits([adv], [inst], [7]) == one
        assert s.ref(one, [1]).verdict == 1
        assert s.verifier.verify_circuits([one], [[inst]], 5, 1) == s.verifier.verify([one], [inst], 5) == [1]
        s.close()
    for pc in (phases_circuits.rlc(), shuffle_circuits.with_challenge(5, True)):  # the phased ones
        s = Setup(orc, zg, ctx, pc, 1)
        (one,), st = s.prover.prove_phased(pc.synthesize([1]), [pc.instance(1)], [7])
        assert st == 0 and s.prove([1], [7]) == one
        assert s.ref(one, [1]).verdict == 1
        bad = flip(one, len(one) - 40)
        assert s.verifier.verify_circuits([one, bad], [[pc.instance(1)]] * 2, 5, 1) == s.verifier.verify([one, bad], [pc.instance(1)] * 2, 5)
        assert s.verifier.verify_circuits([one], [[pc.instance(1)]], 5, 1) == [1]
        s.close()


# ---------------------------------------------------------------------------------------------- 4. scheduling forms, forks
@pytest.mark.parametrize("name", ["three", "with_challenge_phased"])
def test_both_forms_and_a_fork_give_the_same_bytes(ctx, zg, orc, name):
    pc = shuffle_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc, 3)
    seeds = [21, 22, 23]
    proof = s.prove(VARIANTS, seeds)
    s.accepted(proof, VARIANTS)
    for overlap in (False, True):
        s.prover.set_overlap(overlap)
        assert s.prove(VARIANTS, seeds) == proof, overlap
    child_ctx = zg.Ctx(0)
    child = s.prover.fork(child_ctx)
    child.set_batch(3)
    assert s.prove(VARIANTS, seeds, prover=child) == proof
    assert s.prove(VARIANTS, [21, 22, 24]) != proof  # (the last circuit's key is in the bytes)
    child.close()
    child_ctx.close()
    s.close()


# ---------------------------------------------------------------------------------------------- 5. multi-opens, transcripts
@pytest.mark.parametrize("scheme,transcript", [(GWC, EVM), (SHPLONK, EVM), (GWC, BLAKE2B), (SHPLONK, BLAKE2B)])
@pytest.mark.parametrize("maker", ["with_challenge_phased", "interleaved"])
def test_every_multiopen_and_transcript(ctx, zg, orc, maker, scheme, transcript):
    pc = shuffle_circuits.with_challenge(5, True) if maker == "with_challenge_phased" else phases_circuits.interleaved()
    s = Setup(orc, zg, ctx, pc, 2, scheme=scheme, transcript=transcript)
    variants = VARIANTS[:2]
    proof = s.prove(variants, [5, 6])
    s.accepted(proof, variants)
    s.rejected(flip(proof, len(proof) - 40), variants)  # a byte of the tail
    s.close()


# ---------------------------------------------------------------------------------------------- 6. k = 14, the split domain
@pytest.mark.parametrize("maker", ["wide", "rlc"])
def test_k14_on_the_split_domain(ctx, zg, orc, maker):
    """the throughput form at k = 14 with a degree-6 gate: the 4n + n parts, where the fold of the circuits' quotients meets
    what the shuffle pass left on each part; ZG_SPLIT_DOMAIN = 0 -- the single coset -- gives the same bytes"""
    make = (lambda: shuffle_circuits.wide(14, high_gate=True)) if maker == "wide" else phases_circuits.rlc_k14
    orc.load().orc_set_threads(16)
    pc = make()
    variants, seeds = VARIANTS[:2], [41, 42]
    s = Setup(orc, zg, ctx, pc, 2, seed=0x5EED)
    assert s.prover.quotient_terms()["active"]
    s.prover.set_overlap(False)
    proof = s.prove(variants, seeds)
    s.accepted(proof, variants)
    s.close()
    zg.tuning_set("ZG_SPLIT_DOMAIN", 0)
    try:
        s2 = Setup(orc, zg, ctx, pc, 2, seed=0x5EED)
        s2.prover.set_overlap(False)
        assert s2.prove(variants, seeds) == proof
        s2.close()
    finally:
        zg.tuning_set("ZG_SPLIT_DOMAIN", -1)


# ---------------------------------------------------------------------------------------------- 7. plain circuits
def toy_family(count, k=5):
    """`count` toy circuits of one key (tests/test_gpu_multi.py's family): seeds that draw no zero in a1, so the copy
    constraints -- and sigma -- are the same for all of them while witness and instance differ"""
    out, seed = [], 0
    while len(out) < count:
        seed += 1
        rng = random.Random(seed)
        rows = (1 << k) - 8
        if all(rng.randrange(16) for _ in range(rows)):
            cs, asg, ilen = toy_circuit(k, seed=seed)
            assert rows == cs.usable_rows() - 2 and all(asg.get(ADVICE, 1, r) for r in range(rows))
            out.append((cs, asg, ilen))
        assert seed < 5000
    return out


def test_nothing_changed_for_a_plain_circuit(ctx, zg, orc):
    family = toy_family(3)
    cs, asg, ilen = family[0]
    img = cs.to_c()
    params = orc.params_new(cs.k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x1234567)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    for _, other, _ in family[1:]:
        assert np.array_equal(other.fixed_values(), fixed) and np.array_equal(other.sigma_values(), sigma)
    prover = zg.Prover(ctx, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr)
    fc, sc = prover.vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr)
    prover.set_batch(3)
    adv = [a.advice_values() for _, a, _ in family]
    inst = [a.instance_values(ilen) for _, a, _ in family]
    seeds = [31, 32, 33]
    want = prover.prove_multi(adv, inst, seeds)  # (a first proof makes tables: not part of the comparison below)
    assert proof_ref.verify(proof_ref.Vk(cs, params, fixed, sigma, vk_repr), inst, want).verdict == 1
    ctx.profile(True)
    try:
        ctx.profile_collect()
        got = prover.prove_circuits(adv, inst, seeds)
        new_profile = ctx.profile_collect()
        assert prover.prove_multi(adv, inst, seeds) == want
        old_profile = ctx.profile_collect()
    finally:
        ctx.profile(False)
    assert got == want
    launches = lambda prof: {k: v[0] for k, v in prof.items()}  # noqa: E731
    assert launches(new_profile) == launches(old_profile) and len(new_profile) > 5
    assert "challenge_fill" not in new_profile
    assert prover.prove_circuits(adv, inst, seeds, device=False) == want
    slots = [prover.advice_slot(c) for c in range(3)]  # (they hold the columns of the proof before)
    assert prover.prove_circuits(slots, inst, seeds, device=True) == want
    bad = flip(want, 64 * (3 * (cs.n_advice + 3 * len(cs.lookups) + proof_ref.n_sets(cs)) + 1 + cs.degree() - 1) + 31)
    wrong = swapped(inst)
    for proofs, insts in (([want, bad, want], [inst] * 3), ([want, want], [inst, wrong])):
        assert verifier.verify_circuits(proofs, insts, 13, 3) == verifier.verify_multi(proofs, insts, 13, 3)
    assert verifier.verify_circuits([want, bad, want], [inst] * 3, 13, 3) == [1, 0, 1]
    verifier.close()
    prover.close()


# ---------------------------------------------------------------------------------------------- 8. a batch of verdicts
@pytest.mark.parametrize("maker", ["three", "rlc"])
def test_a_batch_of_verdicts(ctx, zg, orc, maker):
    pc = shuffle_circuits.three() if maker == "three" else phases_circuits.rlc()
    s = Setup(orc, zg, ctx, pc, 2)
    orders = [[0, 1], [1, 2], [2, 0]]
    proofs = [s.prove(v, [51 + 2 * i, 52 + 2 * i]) for i, v in enumerate(orders)]
    for p, v in zip(proofs, orders):
        assert s.ref(p, v).verdict == 1
    _, last_ev, _ = offsets(pc.cs, 2)
    proofs[1] = flip(proofs[1], last_ev + 31)
    assert s.ref(proofs[1], orders[1]).verdict == 0
    got = s.verifier.verify_circuits(proofs, [s.insts(v) for v in orders], 13, 2)
    assert got[0] == 1 and got[1] <= 0 and got[2] == 1
    s.close()


# ---------------------------------------------------------------------------------------------- 9. arguments
def test_arguments_and_refusals_leave_the_prover_usable(ctx, zg, orc):
    pc = phases_circuits.rlc()
    s = Setup(orc, zg, ctx, pc, 2)
    variants, seeds = [0, 1], [9, 10]
    proof = s.prove(variants, seeds)
    s.accepted(proof, variants)
    insts = s.insts(variants)
    synth = pc.synthesize([0, 1, 2])
    # circuits = 0, circuits above the prover's slots
    for count in (0, 3):
        out, st = s.prover.prove_circuits_phased(synth, [pc.instance(0)] * count, list(range(count)), raise_on_error=False)
        assert (out, st) == (b"", ZG_ERR_INVALID_ARG), count
    # a plain entry on a circuit with a later-phase column
    adv = [pc.full_advice([5], v) for v in variants]
    assert "zg_prover_prove_circuits_phased" in refused(zg, lambda: s.prover.prove_circuits(adv, insts, seeds), ZG_ERR_INVALID_ARG)
    assert "zg_prover_prove_circuits_phased" in refused(zg, lambda: s.prover.prove_circuits(adv[:1], insts[:1], seeds[:1]), ZG_ERR_INVALID_ARG)
    # a callback that gives up in phase 1
    calls = []

    def stops_in_phase_1(phase, ch):
        calls.append((phase, ch.shape[0]))
        if phase == 1:
            raise RuntimeError("no witness")
        return pc.synthesize(variants)(phase, ch)

    out, st = s.prover.prove_circuits_phased(stops_in_phase_1, insts, seeds, raise_on_error=False)
    assert (out, st) == (b"", ZG_ERR_INVALID_ARG) and calls == [(0, 2), (1, 2)]
    # ... and after all of it the prover makes the proof it made before
    assert s.prove(variants, seeds) == proof
    # 65 circuits: the slots exist (they serve batches), one proof of them is refused before anything is launched
    s.prover.set_batch(65)
    out, st = s.prover.prove_circuits_phased(pc.synthesize([0] * 65), [pc.instance(0)] * 65, list(range(65)), raise_on_error=False)
    assert (out, st) == (b"", ZG_ERR_UNSUPPORTED) and "65 circuits" in zg.load().zg_last_error().decode()
    assert s.prove(variants, seeds) == proof
    s.close()
    # a lookup failure in one circuit of a circuit with a lookup and a shuffle fails the proof
    wide = shuffle_circuits.wide(5, high_gate=True)
    assert wide.cs.lookups and wide.cs.shuffles
    w = Setup(orc, zg, ctx, wide, 2)
    good = w.prove(variants, seeds)
    w.accepted(good, variants)
    for count in (0, 3):  # the plain entry's count: none, more than the prover's two slots
        refused(zg, lambda: w.prover.prove_circuits([w.advice(0)] * count, [wide.instance(0)] * count, list(range(count))), ZG_ERR_INVALID_ARG)
    broken = w.advice(1).copy()
    t_col = wide.cs.n_advice - 1  # the lookup's input column, the last one made
    broken[t_col, 2] = orc.fr_from_int(1000)  # leaves the table 0 .. 7 on a row where q is set
    for overlap in (True, False):
        w.prover.set_overlap(overlap)
        assert "circuit 1" in refused(zg, lambda: w.prover.prove_circuits([w.advice(0), broken], w.insts(variants), seeds), ZG_ERR_CONSTRAINT)
        assert w.prove(variants, seeds) == good
    w.close()
