"""tests/proof_ref.py (the Python-integer verify_proof for N circuits) is not vacuous at N = 1: on proofs the oracle makes
it accepts what orc.verify_proof_pairing accepts and gives its verdict class on the tampered cases of
tests/test_gpu_verify.py::test_rejects_as_the_oracle_does; its proof-length formula is orc.proof_size there.  No device
needed: every proof here is the oracle's."""
import pytest

import proof_ref
from circuits import toy_circuit, variant_circuit

R = proof_ref.R


def cls(v):
    return 1 if v == 1 else 0 if v == 0 else -1


def be(x: int) -> bytes:
    return x.to_bytes(32, "big")


class HostSetup:
    def __init__(self, orc, cs, asg, ilen, seed=0xABCDEF, vk=0x1234567):
        self.cs, self.asg, self.ilen = cs, asg, ilen
        self.img = cs.to_c()
        self.params = orc.params_new(cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        fixed, sigma = asg.fixed_values(), asg.sigma_values()
        self.pk = orc.ProvingKey(self.img, fixed, sigma, self.params, self.vk_repr)
        self.vk = proof_ref.Vk(cs, self.params, fixed, sigma, self.vk_repr)
        self.adv, self.inst = asg.advice_values(), asg.instance_values(ilen)

    def prove(self, orc, adv, inst, seed):
        st, proof, _ = orc.create_proof(self.pk, adv, inst, seed)
        assert st == 0
        return proof


CIRCUITS = [("toy", lambda: toy_circuit(5)), ("toy_d6", lambda: toy_circuit(5, force_degree=6))] + [
    (kind, (lambda kind=kind: variant_circuit(kind, k=5)))
    for kind in ("no_lookup", "gates_only", "wide_lookup", "advice_factor", "merged_selectors")]


@pytest.mark.parametrize("name,make", CIRCUITS, ids=[c[0] for c in CIRCUITS])
def test_accepts_oracle_proofs_and_length_formula(orc, name, make):
    s = HostSetup(orc, *make())
    proof = s.prove(orc, s.adv, s.inst, 1)
    assert orc.verify_proof_pairing(s.pk, s.inst, proof) == 1
    assert proof_ref.verify(s.vk, [s.inst], proof).verdict == 1
    assert proof_ref.proof_len(s.cs, N=1) == len(proof)
    # (orc.proof_size is the bound the oracle allocates: one W per possible rotation; the formula counts the point sets)
    assert proof_ref.proof_len(s.cs, N=1) <= orc.proof_size(s.img)
    c = s.img.c
    max_open = 2 + c.n_advice_queries + c.n_fixed_queries
    assert proof_ref.proof_len(s.cs, N=1) + 64 * (max_open - proof_ref.n_point_sets(s.cs)) == orc.proof_size(s.img)


def test_verdict_classes_on_tampered_proofs(orc):
    s = HostSetup(orc, *toy_circuit(5))
    good = s.prove(orc, s.adv, s.inst, 1)
    c = s.img.c
    sets = proof_ref.n_sets(s.cs)
    s0 = 64 * (c.n_advice + 3 * c.n_lookups + sets + 1 + c.cs_degree - 1)
    g0 = s.params.g_np()[0]
    g0b = be(orc.fq_to_int(g0[0:4])) + be(orc.fq_to_int(g0[4:8]))
    x0 = int.from_bytes(good[0:32], "big")
    sc0 = int.from_bytes(good[s0:s0 + 32], "big")
    bad_inst = s.inst.copy()
    bad_inst[0, 0] = orc.fr_from_int(orc.fr_to_int(bad_inst[0, 0]) + 1)
    unsat = s.adv.copy()
    unsat[2, 3] = orc.fr_from_int(99)
    other = HostSetup(orc, *toy_circuit(5), seed=0x777)
    cases = {
        "good": (good, s.inst),
        "wrong instance": (good, bad_inst),
        "unsatisfied witness": (s.prove(orc, unsat, s.inst, 1), s.inst),
        "advice commitment x + 1": (be(x0 + 1) + good[32:], s.inst),
        "two commitments swapped": (good[64:128] + good[0:64] + good[128:], s.inst),
        "scalar + r": (good[:s0] + be(sc0 + R) + good[s0 + 32:], s.inst),
        "evaluation + 1": (good[:s0] + be((sc0 + 1) % R) + good[s0 + 32:], s.inst),
        "W replaced by g0": (good[:-64] + g0b, s.inst),
        "truncated by 32 bytes": (good[:-32], s.inst),
        "extended by 32 bytes": (good + bytes(32), s.inst),
        "made on another SRS": (other.prove(orc, s.adv, s.inst, 1), s.inst),
    }
    seen = set()
    for name, (proof, inst) in cases.items():
        want = orc.verify_proof_pairing(s.pk, inst, proof)
        got = proof_ref.verify(s.vk, [inst], proof).verdict
        assert got == cls(want), (name, got, want)
        assert (got == 1) == (name == "good"), name
        seen.add(got)
    assert seen == {1, 0, -1}
    # a proof checked against another circuit's key
    alt = HostSetup(orc, *toy_circuit(5, force_degree=6))
    assert proof_ref.verify(alt.vk, [s.inst], good).verdict == cls(orc.verify_proof_pairing(alt.pk, s.inst, good)) != 1


@pytest.mark.parametrize("N", [1, 3, 15, 64])
def test_point_set_lengths_count_the_evaluations(N):
    """Every evaluation of the proof is opened once, and h(x), which the proof does not carry, beside them."""
    for cs in (toy_circuit(5)[0], toy_circuit(6, force_degree=6)[0], variant_circuit("wide_lookup", k=5, seed=3)[0]):
        lengths = proof_ref.point_set_lengths(cs, N)
        A, NL, S, d = cs.n_advice, len(cs.lookups), proof_ref.n_sets(cs), cs.degree()
        points = 64 * (N * (A + 3 * NL + S) + 1 + (d - 1) + proof_ref.n_point_sets(cs))
        assert len(lengths) == proof_ref.n_point_sets(cs)
        assert 32 * (sum(lengths.values()) - 1) == proof_ref.proof_len(cs, N=N) - points
