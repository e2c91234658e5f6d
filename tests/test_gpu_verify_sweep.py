"""The batch verifier's rejections, swept (csrc/verify.hip, csrc/proof_layout.h): EVERY element of a proof changed one at a
time (tests/proof_mutants.py), every instance cell, every commitment of the verifier's key, for every multi-open argument,
transcript, and feature of a circuit -- lookups, several permutation sets, shuffles, challenges, advice phases, several
circuits per proof -- and past the two strides of the kernels: more than 128 proofs in a call (verify_fold) and more
than 128 terms per proof (verify_terms).  All at k = 5.

The judge is tests/proof_ref.py, verify_proof on Python integers.  Every test first asserts the condition on its own
inputs -- the reference accepts the good proof and REJECTS (0: well formed, wrong) each well-formed mutant -- and only
then compares the device's verdict class, 1 / 0 / malformed, position by position.  A verifier that reads an element
but leaves it out of a query, takes another circuit's copy of it, or weights two queries alike accepts one of these.

Tolerances: none -- verdict classes."""
import copy
import ctypes
import time

import numpy as np
import pytest
import torch  # noqa: F401 -- before the first HIP call of the process (tests/conftest.py)

import phases_circuits
import proof_mutants
import proof_ref
import shuffle_circuits
from circuit import R
from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu

GWC, SHPLONK, EVM, BLAKE2B = 0, 1, 0, 1
KEYS = (0xFEED, 0xBEEF)  # two batch keys: other weights r_b, the same verdicts


def cls(v):
    return 1 if v == 1 else 0 if v == 0 else -1


class Plain:
    """harness circuits of ONE key -- (cs, asg, instance rows) per witness variant -- with the face of phases_circuits.Phased"""

    def __init__(self, name, variants):
        self.name, self._variants = name, variants
        self.cs, self.asg, self.ilen = variants[0]
        self.advice_phase, self.challenge_phase, self.n_phases = [0] * self.cs.n_advice, [], 1
        for _, asg, _ in variants[1:]:
            assert np.array_equal(asg.fixed_values(), self.asg.fixed_values()) and np.array_equal(asg.sigma_values(), self.asg.sigma_values())

    def fixed_values(self):
        return self.asg.fixed_values()

    def sigma_values(self):
        return self.asg.sigma_values()

    def instance(self, variant=0):
        return self._variants[variant][1].instance_values(self.ilen)

    def full_advice(self, challenges, variant=0):
        return self._variants[variant][1].advice_values()


def toy():
    """the toy circuit with a degree-5 gate of its own: a lookup, and five permutation columns in chunks of three -- two
    sets, so z_0 is also opened at the last row"""
    pc = Plain("toy", [toy_circuit(5, force_degree=5)])
    assert proof_ref.n_sets(pc.cs) >= 2 and pc.cs.lookups and pc.cs.n_instance == 1
    return pc


def wide_lookup():
    """three witnesses of the width-2 lookup circuit: two instance columns of two rows each"""
    pc = Plain("wide_lookup", [variant_circuit("wide_lookup", 5, seed) for seed in (3, 4, 5)])
    assert (pc.cs.n_instance, pc.ilen) == (2, 2)
    return pc


# name -> (maker, circuits per proof, multi-open, transcript): each multi-open with each transcript, each feature once
CONFIGS = {
    "toy": (toy, 1, GWC, EVM),
    "three": (shuffle_circuits.three, 2, SHPLONK, BLAKE2B),
    "three_phase": (phases_circuits.three_phase, 2, GWC, BLAKE2B),
    "with_challenge_phased": (lambda: shuffle_circuits.with_challenge(5, True), 3, SHPLONK, EVM),
    "rotated": (shuffle_circuits.rotated, 2, GWC, EVM),
}


class Setup:
    """prover + verifier (told the circuit's shuffles and phases, the multi-open and the transcript) + the reference's key"""

    def __init__(self, orc, zg, ctx, pc, slots, scheme=GWC, transcript=EVM, seed=0xABCDEF, vk=0x1234567):
        self.pc, self.cs, self.zg, self.orc, self.ctx = pc, pc.cs, zg, orc, ctx
        self.scheme, self.transcript = scheme, transcript
        self.img = pc.cs.to_c()
        self.params = orc.params_new(pc.cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        fixed, sigma = pc.fixed_values(), pc.sigma_values()
        self.shuffles = getattr(self.img, "shuffles", None)
        self.prover = zg.Prover(ctx, self.img, fixed, sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr, shuffles=self.shuffles)
        self._told(self.prover)
        self.prover.set_batch(slots)
        self.fc, self.sc = self.prover.vk_commitments()
        self.verifier = self.make_verifier(self.fc, self.sc, self.params.g_np()[0])
        self.vk = proof_ref.Vk(pc.cs, self.params, fixed, sigma, self.vk_repr)
        self._advice = {}

    def _told(self, obj):
        if self.scheme != GWC:
            obj.set_multiopen(self.scheme)
        if self.transcript != EVM:
            obj.set_transcript(self.transcript)
        if self.pc.n_phases > 1 or self.pc.challenge_phase:
            obj.set_phases(self.pc.advice_phase, self.pc.challenge_phase)

    def make_verifier(self, fc, sc, g0):
        v = self.zg.Verifier(self.ctx, self.img, fc, sc, g0, np.array(self.params.g2, np.uint64), np.array(self.params.s_g2, np.uint64),
                             self.vk_repr, shuffles=self.shuffles)
        self._told(v)
        return v

    def insts(self, variants):
        return [self.pc.instance(v) for v in variants]

    def prove(self, variants, seeds) -> bytes:
        """ONE proof of len(variants) circuits, through the entry the circuit needs"""
        if self.pc.n_phases > 1:
            proof, st = self.prover.prove_circuits_phased(self.pc.synthesize(variants), self.insts(variants), seeds)
            assert st == 0
            return proof
        for v in variants:
            if v not in self._advice:
                self._advice[v] = self.pc.full_advice([0] * len(self.pc.challenge_phase), v)
        return self.prover.prove_circuits([self._advice[v] for v in variants], self.insts(variants), seeds)

    def ref(self, proof, insts, vk=None) -> int:
        return proof_ref.verify(vk or self.vk, insts, proof, advice_phase=self.pc.advice_phase, challenge_phase=self.pc.challenge_phase,
                                scheme=self.scheme, transcript=self.transcript).verdict

    def dev(self, proofs, insts, key, verifier=None) -> list:
        """the device's verdict classes; insts: per proof the list of its circuits' instance arrays"""
        v = verifier or self.verifier
        N = len(insts[0])
        got = v.verify(proofs, [i[0] for i in insts], key) if N == 1 else v.verify_circuits(proofs, insts, key, N)
        return [cls(g) for g in got]

    def spans(self, N):
        return proof_mutants.spans(self.cs, N, self.scheme, self.transcript, self.pc.advice_phase)

    def close(self):
        self.verifier.close()
        self.prover.close()


def make(orc, zg, ctx, name, N=None):
    maker, n, scheme, transcript = CONFIGS[name]
    N = N or n
    s = Setup(orc, zg, ctx, maker(), N, scheme, transcript)
    variants = list(range(N))
    proof = s.prove(variants, [61 + c for c in range(N)])
    insts = s.insts(variants)
    assert len(proof) == proof_ref.proof_len(s.cs, N, scheme, transcript)
    assert s.ref(proof, insts) == 1, "the input: the reference does not accept the good proof"
    return s, proof, insts


def sweep(s, good, insts, mutants, well_formed):
    """ONE call over the good proof first, in the middle and last and every mutant between; the reference's class of
    every entry first (the condition on the input), then the device's under two batch keys.  well_formed: how many of
    the mutants, the first ones, must be rejected by the algebra."""
    want = []
    for i, m in enumerate(mutants):
        v = s.ref(m.proof, insts)
        assert v == 0 if i < well_formed else v in (0, -1), "the input: the reference gives %d for %s" % (v, m.label)
        want.append(v)
    if len(mutants) > well_formed:
        assert {0, -1} <= set(want[well_formed:]), "the input: the encoding mutants miss a class"
    half = len(mutants) // 2
    labels = ["good (first)"] + [m.label for m in mutants[:half]] + ["good (middle)"] + [m.label for m in mutants[half:]] + ["good (last)"]
    proofs = [good] + [m.proof for m in mutants[:half]] + [good] + [m.proof for m in mutants[half:]] + [good]
    expect = [1] + want[:half] + [1] + want[half:] + [1]
    for key in KEYS:
        got = s.dev(proofs, [insts] * len(proofs), key)
        wrong = [(label, g, w) for label, g, w in zip(labels, got, expect) if g != w]
        assert not wrong, "key %#x: (element, device, reference) %s" % (key, wrong)
    return want


# ------------------------------------------------------------------------------------------ a. every element, every form
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_every_element_binds(ctx, zg, orc, name):
    s, good, insts = make(orc, zg, ctx, name)
    sp = s.spans(len(insts))
    mutants = list(proof_mutants.well_formed_mutants(good, sp))
    assert sorted({m.span for m in mutants}) == list(range(len(sp)))  # no element left out
    well_formed = len(mutants)
    mutants += list(proof_mutants.encoding_mutants(good, sp))
    t0 = time.perf_counter()
    sweep(s, good, insts, mutants, well_formed)
    print("%s: %d elements, %d + %d mutants, %.1f s" % (name, len(sp), well_formed, len(mutants) - well_formed, time.perf_counter() - t0))
    s.close()


# ------------------------------------------------------------------------------------------ b. instances
def plus_one(orc, inst, col, row):
    out = inst.copy()
    out[col, row] = orc.fr_from_int((orc.fr_to_int(inst[col, row]) + 1) % R)
    return out


@pytest.mark.parametrize("name", ["toy", "three_phase", "wide_lookup"])
def test_every_instance_cell_and_order_binds(ctx, zg, orc, name):
    """inst[count][NC][I][ilen]: each cell of each circuit + 1, and circuits c and c + 1 exchanged, the proof unchanged.
    wide_lookup (GWC, EVM, three circuits of two instance columns with two rows) is here for the indexing: the
    configurations of the element sweep have one instance cell per circuit."""
    if name == "wide_lookup":
        s = Setup(orc, zg, ctx, wide_lookup(), 3)
        insts = s.insts([0, 1, 2])
        good = s.prove([0, 1, 2], [71, 72, 73])
        assert s.ref(good, insts) == 1
    else:
        s, good, insts = make(orc, zg, ctx, name)
    N = len(insts)
    cases = [("good", insts)]
    for c in range(N):
        for col in range(insts[c].shape[0]):
            for row in range(insts[c].shape[1]):
                cases.append(("circuit %d column %d row %d + 1" % (c, col, row), insts[:c] + [plus_one(orc, insts[c], col, row)] + insts[c + 1:]))
    for c in range(N - 1):
        assert insts[c].tobytes() != insts[c + 1].tobytes(), "the input: circuits %d and %d have the same instance" % (c, c + 1)
        cases.append(("circuits %d and %d exchanged" % (c, c + 1), insts[:c] + [insts[c + 1], insts[c]] + insts[c + 2:]))
    cases.append(("good", insts))
    assert len(cases) == 2 + N * s.cs.n_instance * insts[0].shape[1] + N - 1
    want = [s.ref(good, i) for _, i in cases]
    assert want == [1] + [0] * (len(cases) - 2) + [1], "the input: %s" % list(zip([n for n, _ in cases], want))
    for key in KEYS:
        got = s.dev([good] * len(cases), [i for _, i in cases], key)
        assert got == want, (key, [(n, g) for (n, _), g, w in zip(cases, got, want) if g != w])
    s.close()


# ------------------------------------------------------------------------------------------ c. the key's commitments
def key_mutants(s):
    """(label, fixed_c, sigma_c, g0 of the device's verifier, the reference's Vk): each fixed and each sigma commitment in
    turn replaced by another commitment of the key -- the next one, fixed then sigma, cyclically, that differs from it --
    and g[0] by g[1]"""
    F = s.fc.shape[0]
    dev_pool = [np.array(p) for p in s.fc] + [np.array(p) for p in s.sc]
    ref_pool = list(s.vk.fixed_c) + list(s.vk.sigma_c)
    g = s.params.g_np()
    assert len(dev_pool) == len(ref_pool) == s.cs.n_fixed + len(s.cs.perm_columns)
    for t in range(len(dev_pool)):
        r = next(j % len(dev_pool) for j in range(t + 1, t + len(dev_pool)) if dev_pool[j % len(dev_pool)].tobytes() != dev_pool[t].tobytes())
        dev, ref = list(dev_pool), list(ref_pool)
        dev[t], ref[t] = dev_pool[r], ref_pool[r]
        name = lambda i: "fixed %d" % i if i < F else "sigma %d" % (i - F)  # noqa: E731
        vk = copy.copy(s.vk)
        vk.fixed_c, vk.sigma_c = ref[:F], ref[F:]
        yield ("%s replaced by %s" % (name(t), name(r)), np.array(dev[:F]).reshape(F, 8), np.array(dev[F:]).reshape(len(dev) - F, 8), g[0], vk)
    vk = copy.copy(s.vk)
    vk.g0 = np.zeros(12, np.uint64)
    g1 = np.ascontiguousarray(g[1])
    orc_lib = s.orc.load()
    orc_lib.orc_g1_from_affine(ctypes.c_void_p(vk.g0.ctypes.data), ctypes.c_void_p(g1.ctypes.data))
    assert g[0].tobytes() != g[1].tobytes()
    yield ("g[0] replaced by g[1]", s.fc, s.sc, g[1], vk)


def key_sweep(s, good, insts):
    count = 0
    for label, fc, sc, g0, vk in key_mutants(s):
        assert s.ref(good, insts, vk) == 0, "the input: the reference does not reject the good proof with " + label
        verifier = s.make_verifier(fc, sc, g0)
        try:
            for key in KEYS:
                assert s.dev([good, good], [insts] * 2, key, verifier) == [0, 0], (label, key)
        finally:
            verifier.close()
        count += 1
    assert count == s.cs.n_fixed + len(s.cs.perm_columns) + 1  # no column left out
    assert s.dev([good], [insts], KEYS[0]) == [1]


@pytest.mark.parametrize("name", ["toy", "three"])
def test_every_commitment_of_the_key_binds(ctx, zg, orc, name):
    s, good, insts = make(orc, zg, ctx, name)
    key_sweep(s, good, insts)
    s.close()


# ------------------------------------------------------------------------------------------ d. more than 128 proofs
BAD_AT = (0, 127, 128, 129, 255, 256, 259)


def test_more_than_128_proofs(ctx, zg, orc):
    """260 proofs in one call, verify_fold's lanes each fold more than one proof (b += TERMS_WG): four good toy proofs
    repeated, well-formed mutants of seven different elements at 0, 127, 128, 129, 255, 256 and 259.  The reference is
    asked for the seven mutants and one good proof.  The call, the bisection's host pairings included, is timed and
    printed; measured on an MI355X: 0.34 to 0.39 s per call of 260 proofs with the seven wrong ones, 0.22 s with
    five, 0.10 s with one, so all seven positions stay."""
    maker, _, scheme, transcript = CONFIGS["toy"]
    s = Setup(orc, zg, ctx, maker(), 1, scheme, transcript)
    insts = s.insts([0])
    goods = [s.prove([0], [seed]) for seed in (81, 82, 83, 84)]
    assert len(set(goods)) == 4 and s.ref(goods[0], insts) == 1
    sp = s.spans(1)
    proofs, labels = [goods[b % 4] for b in range(260)], {}
    for i, b in enumerate(BAD_AT):
        mutants = list(proof_mutants.well_formed_mutants(proofs[b], sp))
        m = mutants[(i * len(mutants)) // len(BAD_AT)]  # (seven elements spread over the proof: points, scalars, a W)
        assert s.ref(m.proof, insts) == 0, "the input: the reference does not reject " + m.label
        proofs[b], labels[b] = m.proof, m.label
    assert len(set(labels.values())) == len(BAD_AT)
    # all seven; then only those from 128 on, then the last alone: with a wrong proof among the first 128 the bisection's
    # host sums find every other one too, whatever the fold of the proofs behind them returned
    for wrong_at in (BAD_AT, BAD_AT[2:], BAD_AT[-1:]):
        batch = [proofs[b] if b in wrong_at else goods[b % 4] for b in range(260)]
        want = [0 if b in wrong_at else 1 for b in range(260)]
        for key in KEYS:
            t0 = time.perf_counter()
            got = s.dev(batch, [insts] * 260, key)
            print("260 proofs, %d wrong, key %#x: %.3f s" % (len(wrong_at), key, time.perf_counter() - t0))
            assert got == want, (key, [(b, labels.get(b, "good"), g) for b, (g, w) in enumerate(zip(got, want)) if g != w])
    s.close()


# ------------------------------------------------------------------------------------------ e. more than 128 terms
def n_terms(cs, N, scheme):
    """the terms of a proof's two sums: its points, the left side's points once more (every W; SHPLONK: one), the key's
    fixed and sigma commitments and g[0]"""
    points, _ = proof_ref.counts(cs, N, scheme)
    return points + (1 if scheme == SHPLONK else proof_ref.n_point_sets(cs)) + cs.n_fixed + len(cs.perm_columns) + 1


def test_more_than_128_terms(ctx, zg, orc):
    """One proof of so many circuits of shuffle_circuits.three that verify_terms' lanes each take more than one term
    (t += TERMS_WG), GWC and EVM: the terms past the first 128 are the left side's copies of the tail points and the key's
    commitments.  The reference's cost grows with the circuits, so three groups are swept here: the LAST circuit's
    elements (the highest circuit index in every table), the tail points and the key's commitments.
    The elements of the circuits before the last, and the random, h, fixed, random and sigma elements that the circuits
    share, are left to test_every_element_binds, where every element of proofs of two and three circuits is changed."""
    cs = shuffle_circuits.three().cs
    N = next(n for n in range(1, 65) if n_terms(cs, n, GWC) > 128)
    assert n_terms(cs, N, GWC) > 128 >= n_terms(cs, N - 1, GWC) and N > 1
    s = Setup(orc, zg, ctx, shuffle_circuits.three(), N)
    variants = list(range(N))
    insts = s.insts(variants)
    good = s.prove(variants, [91 + c for c in range(N)])
    assert s.ref(good, insts) == 1
    sp = s.spans(N)
    mine = [i for i, x in enumerate(sp) if (" c%d " % (N - 1)) in x.label or x.label.startswith("W ")]
    per_circuit = (len(sp) - len([x for x in sp if " c" not in x.label])) // N
    assert len(mine) == per_circuit + proof_ref.n_point_sets(cs)
    mutants = [m for m in proof_mutants.well_formed_mutants(good, sp) if m.span in mine]
    assert sorted({m.span for m in mutants}) == mine
    sweep(s, good, insts, mutants, len(mutants))
    key_sweep(s, good, insts)
    s.close()
