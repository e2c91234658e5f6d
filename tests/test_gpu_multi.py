"""One proof of several circuit instances (zg_prover_prove_multi: create_proof's `circuits` slice) and its verification on
the device (zg_verifier_verify_multi).  The judge of every multi-circuit proof is tests/proof_ref.py, a Python-integer
verify_proof for N circuits that shares nothing with the library; at N = 1 the bytes are the oracle's.

All witnesses of one proof belong to ONE key: the families below are built from seeds whose copy constraints do not
depend on the values, and every test asserts that their fixed and sigma columns are equal."""
import random

import numpy as np
import pytest

import proof_ref
from circuit import ADVICE
from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu

R = proof_ref.R


def cls(v):
    return 1 if v == 1 else 0 if v == 0 else -1


def be(x: int) -> bytes:
    return x.to_bytes(32, "big")


def toy_family(count, k=5, **kw):
    """`count` toy circuits of one key: toy_circuit copies the rows where a1 = 0 onto each other, so the seeds are chosen
    among those that draw no zero -- then the copies, and with them sigma, are the same for all of them, while the
    witness and the instance (the chain's product) differ."""
    out, seed = [], 0
    while len(out) < count:
        seed += 1
        rng = random.Random(seed)
        rows = (1 << k) - 8  # usable - 2 with the toy circuit's six blinding rows (asserted below)
        if all(rng.randrange(16) for _ in range(rows)):
            cs, asg, ilen = toy_circuit(k, seed=seed, **kw)
            assert rows == cs.usable_rows() - 2 and all(asg.get(ADVICE, 1, r) for r in range(rows))
            out.append((cs, asg, ilen))
        assert seed < 5000
    return out


def variant_family(kind, count, k=5):
    return [variant_circuit(kind, k=k, seed=3 + s) for s in range(count)]


class Setup:
    """One key (prover, device verifier, reference vk) and the witnesses of a family of circuits on it."""

    def __init__(self, orc, zg, ctx, family, seed=0xABCDEF, vk=0x1234567):
        cs, asg, ilen = family[0]
        self.cs, self.ilen = cs, ilen
        self.img = cs.to_c()
        self.params = orc.params_new(cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        fixed, sigma = asg.fixed_values(), asg.sigma_values()
        for _, other, _ in family[1:]:  # one key for all of them
            assert np.array_equal(other.fixed_values(), fixed) and np.array_equal(other.sigma_values(), sigma)
        self.pk = orc.ProvingKey(self.img, fixed, sigma, self.params, self.vk_repr)
        self.prover = zg.Prover(ctx, self.img, fixed, sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr)
        fc, sc = self.prover.vk_commitments()
        self.verifier = zg.Verifier(ctx, self.img, fc, sc, self.params.g_np()[0], np.array(self.params.g2, np.uint64),
                                    np.array(self.params.s_g2, np.uint64), self.vk_repr)
        self.ref = proof_ref.Vk(cs, self.params, fixed, sigma, self.vk_repr)
        self.adv = [a.advice_values() for _, a, _ in family]
        self.inst = [a.instance_values(ilen) for _, a, _ in family]
        self.prover.set_batch(max(len(family), 1))

    def prove(self, idx, seeds, overlap):
        self.prover.set_overlap(overlap)
        return self.prover.prove_multi([self.adv[i] for i in idx], [self.inst[i] for i in idx], seeds)

    def both_forms(self, idx, seeds):
        a, b = self.prove(idx, seeds, True), self.prove(idx, seeds, False)
        assert a == b and len(a) > 0
        return a

    def verdicts(self, proof, insts, circuits=None, key=3):
        """(device verdict, reference verdict) of one multi proof"""
        circuits = len(insts) if circuits is None else circuits
        return self.verifier.verify_multi([proof], [insts], key, circuits)[0], proof_ref.verify(self.ref, insts, proof).verdict

    def close(self):
        self.verifier.close()
        self.prover.close()


def test_one_circuit_is_the_single_proof(ctx, zg, orc):
    s = Setup(orc, zg, ctx, toy_family(1))
    want = orc.create_proof(s.pk, s.adv[0], s.inst[0], 7)[1]
    for overlap in (True, False):
        s.prover.set_overlap(overlap)
        assert s.prover.prove_multi([s.adv[0]], [s.inst[0]], [7]) == s.prover.prove(s.adv[0], s.inst[0], 7) == want
    assert s.verifier.verify_multi([want], [[s.inst[0]]], 5, 1) == s.verifier.verify([want], [s.inst[0]], 5) == [1]
    s.close()


@pytest.mark.parametrize("N", [2, 3, 5])
def test_n_circuits_verify(ctx, zg, orc, N):
    s = Setup(orc, zg, ctx, toy_family(N))
    assert len({i.tobytes() for i in s.inst}) == N  # different instances (and witnesses)
    proof = s.both_forms(list(range(N)), [11 + c for c in range(N)])
    assert len(proof) == proof_ref.proof_len(s.cs, N=N)
    assert proof_ref.verify(s.ref, s.inst, proof).verdict == 1
    assert s.verifier.verify_multi([proof], [s.inst], 9, N) == [1]
    s.close()


CHUNK = 128  # combine_pairs_kernel takes a point set's list in chunks of HC9_MAX = 128 terms, the short chunk first


def short_first_chunk_N(cs) -> tuple:
    """(N, length): the N in 1..64 whose longest point-set list is nearest above a multiple of 128 (the smallest such N)"""
    longest = {N: max(proof_ref.point_set_lengths(cs, N).values()) for N in range(1, 65)}
    N = min((L % CHUNK, N) for N, L in longest.items() if L > CHUNK and L % CHUNK)[1]
    return N, longest[N]


@pytest.mark.parametrize("N", [4, 7, 15, 64])
def test_lazy_sum_kernels_at_their_edges(ctx, zg, orc, N):
    """fold_slots_kernel sums the circuits' quotients three terms at a time: N = 4 leaves its loop a tail of one, N = 7 two
    rounds and a tail of one, N = 64 is FOLD_MAX_SLOTS (21 rounds and a tail of one, every weight slot in use).
    combine_pairs_kernel: the toy circuit's longest list (rotation 0) holds 8 N + 10 pairs; N = 15 gives 130 = 2 + 128, the
    N in 1..64 nearest above a multiple of 128 -- a first chunk of two terms, then a whole chunk chained by v^128; N = 64
    gives 522 = 10 + 4 * 128."""
    s = Setup(orc, zg, ctx, toy_family(N))
    assert short_first_chunk_N(s.cs) == (15, 130)
    assert max(proof_ref.point_set_lengths(s.cs, N).values()) == 8 * N + 10
    proof = s.both_forms(list(range(N)), [71 + c for c in range(N)])
    assert len(proof) == proof_ref.proof_len(s.cs, N=N)
    assert s.verdicts(proof, s.inst) == (1, 1)
    if N > 4:  # the last circuit's quotient is in the sum: its instance exchanged with another's is rejected by both
        assert s.inst[N - 1].tobytes() != s.inst[0].tobytes()
        assert s.verdicts(proof, [s.inst[N - 1]] + s.inst[1:N - 1] + [s.inst[0]]) == (0, 0)
    s.close()


def test_sixty_five_circuits_are_refused(ctx, zg, orc):
    """FOLD_MAX_SLOTS + 1: zg_prover_set_batch allows 65 slots (they serve batches of proofs), one proof of 65 circuits is
    ZG_ERR_UNSUPPORTED -- the status poly_fold_slots has for it, raised by zg_prover_prove_multi before anything is launched --
    and the prover goes on to prove 64."""
    s = Setup(orc, zg, ctx, toy_family(65))
    assert s.prover.batch == 65
    s.prover.set_overlap(True)
    with pytest.raises(zg.ZgError) as e:
        s.prover.prove_multi(s.adv, s.inst, list(range(65)))
    assert e.value.status == -4 and "65 circuits" in str(e.value)  # ZG_ERR_UNSUPPORTED
    proof = s.prover.prove_multi(s.adv[:64], s.inst[:64], list(range(64)))
    assert s.verifier.verify_multi([proof], [s.inst[:64]], 5, 64) == [1]
    s.close()


def test_structure_of_a_three_circuit_proof(ctx, zg, orc):
    """Circuit-major order and per-circuit keys, without any verifier: circuit c's advice commitments are those of its own
    single proof under key c; the random polynomial's commitment is the single proof's under key 0."""
    s = Setup(orc, zg, ctx, toy_family(3))
    seeds = [21, 22, 23]
    proof = s.both_forms([0, 1, 2], seeds)
    A, NL, S = s.cs.n_advice, len(s.cs.lookups), proof_ref.n_sets(s.cs)
    singles = [s.prover.prove(s.adv[c], s.inst[c], seeds[c]) for c in range(3)]
    for c in range(3):
        assert proof[64 * A * c:64 * A * (c + 1)] == singles[c][:64 * A], c
    at_multi, at_single = 64 * 3 * (A + 3 * NL + S), 64 * (A + 3 * NL + S)
    assert proof[at_multi:at_multi + 64] == singles[0][at_single:at_single + 64]
    assert proof[at_multi:at_multi + 64] != singles[1][at_single:at_single + 64]
    s.close()


SHAPES = {
    "no_lookup": lambda: variant_family("no_lookup", 3),   # the random polynomial rides with the products
    "gates_only": lambda: variant_family("gates_only", 3),
    "wide_lookup": lambda: variant_family("wide_lookup", 3),  # two instance columns
    "toy_two_sets": lambda: toy_family(3, k=6),
    "toy_degree_6": lambda: toy_family(3, k=6, force_degree=6),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_circuit_shapes(ctx, zg, orc, shape):
    s = Setup(orc, zg, ctx, SHAPES[shape]())
    if shape.startswith("toy"):
        assert proof_ref.n_sets(s.cs) > 1
    proof = s.both_forms([0, 1, 2], [31, 32, 33])
    assert len(proof) == proof_ref.proof_len(s.cs, N=3)
    assert s.verdicts(proof, s.inst) == (1, 1)
    s.close()


def test_rejections(ctx, zg, orc):
    s = Setup(orc, zg, ctx, toy_family(3))
    seeds = [41, 42, 43]
    good = s.both_forms([0, 1, 2], seeds)
    assert s.verdicts(good, s.inst) == (1, 1)
    assert s.inst[0].tobytes() != s.inst[1].tobytes()
    bad1 = [i.copy() for i in s.inst]
    bad1[1][0, 0] = orc.fr_from_int(orc.fr_to_int(bad1[1][0, 0]) + 1)
    unsat = s.adv[2].copy()
    unsat[2, 3] = orc.fr_from_int(99)
    s.prover.set_overlap(True)
    unsat_proof = s.prover.prove_multi([s.adv[0], s.adv[1], unsat], s.inst, seeds)
    cs = s.cs
    A, NL, S = cs.n_advice, len(cs.lookups), proof_ref.n_sets(cs)
    AQ = len(cs.advice_queries)
    s0 = 64 * (3 * (A + 3 * NL + S) + 1 + cs.degree() - 1) + 32 * (2 * AQ)  # the last circuit's first advice evaluation
    sc0 = int.from_bytes(good[s0:s0 + 32], "big")
    g0 = s.params.g_np()[0]
    g0b = be(orc.fq_to_int(g0[0:4])) + be(orc.fq_to_int(g0[4:8]))
    cases = {
        "an instance value of circuit 1 changed": (good, bad1, 3),
        "instances of circuits 0 and 1 exchanged": (good, [s.inst[1], s.inst[0], s.inst[2]], 3),
        "unsatisfied witness in the last circuit": (unsat_proof, s.inst, 3),
        "an advice evaluation of the last circuit + 1": (good[:s0] + be((sc0 + 1) % R) + good[s0 + 32:], s.inst, 3),
        "verified as 2 circuits": (good, s.inst[:2], 2),
        "verified as 4 circuits": (good, s.inst + [s.inst[0]], 4),
        "truncated by 32 bytes": (good[:-32], s.inst, 3),
        "extended by 32 bytes": (good + bytes(32), s.inst, 3),
        "last W replaced by g0": (good[:-64] + g0b, s.inst, 3),
    }
    for name, (proof, insts, circuits) in cases.items():
        got, want = s.verdicts(proof, insts, circuits)
        assert cls(got) == want, (name, got, want)
        assert got != 1, name
    # a batch of three multi-proofs, the middle one bad
    other = s.both_forms([2, 0, 1], [51, 52, 53])
    tampered = cases["an advice evaluation of the last circuit + 1"][0]
    assert s.verifier.verify_multi([good, tampered, other], [s.inst, s.inst, [s.inst[2], s.inst[0], s.inst[1]]], 13, 3) == [1, 0, 1]
    s.close()


def test_lookup_failure_in_one_circuit_fails_the_proof(ctx, zg, orc):
    s = Setup(orc, zg, ctx, toy_family(3))
    bad = s.adv[2].copy()
    bad[1, 2] = orc.fr_from_int(1000)  # a1 leaves its table on an enabled row
    for overlap in (True, False):
        s.prover.set_overlap(overlap)
        with pytest.raises(zg.ZgError) as e:
            s.prover.prove_multi([s.adv[0], s.adv[1], bad], s.inst, [1, 2, 3])
        assert e.value.status == -5 and "circuit 2" in str(e.value)  # ZG_ERR_CONSTRAINT
        proof = s.prover.prove_multi(s.adv, s.inst, [1, 2, 3])  # the next call on the prover succeeds
        assert s.verifier.verify_multi([proof], [s.inst], 2, 3) == [1]
    s.close()


def test_arguments(ctx, zg, orc):
    s = Setup(orc, zg, ctx, toy_family(2))
    assert s.prover.proof_size_multi(2) >= proof_ref.proof_len(s.cs, N=2) and s.prover.proof_size_multi(1) == s.prover.proof_cap
    for count in (0, 3):  # max_batch = 2
        with pytest.raises(zg.ZgError) as e:
            s.prover.prove_multi([s.adv[0]] * count, [s.inst[0]] * count, list(range(count)))
        assert e.value.status == -1, count  # ZG_ERR_INVALID_ARG
    s.close()


# ---- the tiny model (k = 14), image bytes -> one proof
@pytest.fixture(scope="module")
def tiny(ctx, zg, orc):
    import witness_tape
    import wnn_circuit
    import wnn_model

    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    wnn = wnn_model.load_checked_in(name)
    real = wnn_model.load_test_image()
    s = Setup(orc, zg, ctx, [wnn_circuit.build(wnn, real, k)[:3]], seed=0x5EED, vk=0xC0FFEE)
    s.wnn, s.real = wnn, real
    s.plan = zg.WitnessPlan(ctx, witness_tape.trace(wnn, k).arrays())
    s.prover.set_batch(32)
    s.prover.set_overlap(False)
    yield s
    s.plan.close()
    s.close()


def test_tiny_model_three_images(tiny, zg):
    s = tiny
    images = [s.real, np.zeros_like(s.real), np.full_like(s.real, 255)]
    proof, outputs = s.prover.prove_images_multi(s.plan, np.stack(images), [61, 62, 63])
    assert len(proof) == proof_ref.proof_len(s.cs, N=3)
    for c, im in enumerate(images):
        assert [zg.fr_to_int(x) for x in outputs[c]] == s.wnn.predict(im), c
    insts = [outputs[c][None, :, :] for c in range(3)]
    assert len({i.tobytes() for i in insts}) > 1
    assert s.verdicts(proof, insts) == (1, 1)
    swapped = [insts[1], insts[0], insts[2]]
    assert insts[0].tobytes() != insts[1].tobytes()
    got, want = s.verdicts(proof, swapped)
    assert cls(got) == want == 0


def test_tiny_model_thirty_two_images(tiny, zg):
    """The list-size limits: 32 circuits put about a thousand polynomials at x."""
    s = tiny
    rng = np.random.default_rng(32)
    images = [s.real] + [rng.integers(0, 256, size=s.real.shape, dtype=s.real.dtype) for _ in range(31)]
    proof, outputs = s.prover.prove_images_multi(s.plan, np.stack(images), list(range(100, 132)))
    assert len(proof) == proof_ref.proof_len(s.cs, N=32)
    insts = [outputs[c][None, :, :] for c in range(32)]
    assert s.verifier.verify_multi([proof], [insts], 17, 32) == [1]
    insts[31], insts[30] = insts[30], insts[31]
    assert insts[30].tobytes() != insts[31].tobytes()
    assert s.verifier.verify_multi([proof], [insts], 17, 32) == [0]
