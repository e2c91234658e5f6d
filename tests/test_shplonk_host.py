"""tests/proof_ref.py's SHPLONK side (the Python-integer prover tail and verifier) is not vacuous: its
rotation sets on a hand-written list, its prover's proofs accepted by its verifier on circuits with one to four opening
points, the prefix shared with the oracle's GWC proof, the length formula, every verdict class, and the two schemes
refusing each other's proofs.  No device: the prover tail runs over tests/arith_level.py's host backend.

A proof of two circuits needs a prover of two circuits, which exists on the device only: tests/golden/shplonk_n2.json is
such a proof, recorded from zg_prover_prove_multi (tests/test_gpu_shplonk.py holds the device to the same bytes), and the
reference verifier judges it here."""
import json
import os

import pytest

import arith_level
import poly_ref as pr
import proof_ref
from circuit import FIXED, Assignment, ConstraintSystem
from circuits import toy_circuit, variant_circuit
from test_gpu_multi import toy_family

R, SHPLONK = proof_ref.R, proof_ref.SHPLONK


def shplonk(vk, instances, proof) -> int:
    return proof_ref.verify(vk, instances, proof, scheme=SHPLONK).verdict


CIRCUITS = {
    "toy": lambda: toy_circuit(k=5),
    "two_lookups": lambda: toy_circuit(k=5, two_lookups=True),
    "gates_only": lambda: variant_circuit("gates_only", k=5),
    "no_lookup": lambda: variant_circuit("no_lookup", k=5),
    "wide_lookup": lambda: variant_circuit("wide_lookup", k=5),
}


GOLDEN_N2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shplonk_n2.json")


def many_queries_circuit(k, subsets):
    """One advice column per entry of `subsets`, queried at exactly those rotations, in one gate that the all-zero witness
    satisfies (degree 3): circuits with as many rotation sets or opening points as a test of the limits needs."""
    cs = ConstraintSystem(k)
    q = cs.fixed_column()
    cols = [cs.advice_column() for _ in subsets]
    total = None
    for c, rots in zip(cols, subsets):
        for r in rots:
            total = cs.advice(c, r) if total is None else total + cs.advice(c, r)
    cs.create_gate([cs.fixed(q) * total * cs.advice(cols[0], subsets[0][0])])
    asg = Assignment(cs)
    for r in range(cs.usable_rows() - max(max(rots) for rots in subsets) - 1):
        asg.set(FIXED, q, r, 1)
    return cs, asg, 0


def seventeen_sets_circuit():
    """17 advice columns opened at 17 different subsets of the rotations 0..4: with the fixed column, h and the random
    polynomial (all at x alone, as column 0) 17 rotation sets, one more than HC_MAX_SETS, over 5 points"""
    return many_queries_circuit(5, [[r for r in range(5) if (i + 1) >> r & 1] for i in range(17)])


def seventeen_points_circuit():
    """one column at the rotations 0..16: 17 opening points, one more than PC_MAX_POINTS"""
    return many_queries_circuit(6, [list(range(17))])


class Made:
    """One circuit's key, the oracle's GWC proof and the reference SHPLONK proof for the same inputs and blinding key."""

    def __init__(self, orc, name, seed=11):
        cs, asg, ilen = CIRCUITS[name]()
        self.cs = cs
        img = cs.to_c()
        self.params = orc.params_new(cs.k, 0xABCDEF)
        vk_repr = orc.fr_from_int(0x1234567)
        fixed, sigma = asg.fixed_values(), asg.sigma_values()
        self.pk = orc.ProvingKey(img, fixed, sigma, self.params, vk_repr)
        self.vk = proof_ref.Vk(cs, self.params, fixed, sigma, vk_repr)
        self.adv, self.inst = asg.advice_values(), asg.instance_values(ilen)
        st, self.gwc, tr = orc.create_proof(self.pk, self.adv, self.inst, seed, want_trace=True)
        assert st == 0
        h_ext = tr.array("h_ext", 1 << cs.extended_k())
        challenges = [pr.to_int(tr.fe(name)) for name in ("theta", "beta", "gamma", "y")]
        orc.trace_free(tr)
        be = arith_level.HostBackend(orc, cs, fixed, sigma, self.params, seed, h_ext, challenges)
        self.proof = proof_ref.create_proof(be, self.vk, self.adv, self.inst, scheme=SHPLONK)


_made = {}


@pytest.fixture
def made(orc):
    def get(name):
        if name not in _made:
            _made[name] = Made(orc, name)
        return _made[name]
    return get


def test_intermediate_sets_on_a_hand_written_list():
    x, wx, w3x, winvx = "x", "wx", "w3x", "w-1x"
    queries = [(x, 0), (wx, 0), (x, 1), (winvx, 2), (x, 2), (x, 3), (wx, 3), (w3x, 3), (wx, 4), (x, 4), (x, 5)]
    sets, T = proof_ref.intermediate_sets(queries)
    assert [len(points) for points, _ in sets] == [2, 1, 2, 3]
    assert [keys for _, keys in sets] == [[0, 4], [1, 5], [2], [3]]
    assert [set(points) for points, _ in sets] == [{x, wx}, {x}, {winvx, x}, {x, wx, w3x}]
    assert len(T) == 4 and set(T) == {x, wx, w3x, winvx}


def test_the_circuits_cover_the_shapes_they_are_here_for(made):
    def shape(name):
        m = made(name)
        qs = proof_ref.replay(m.vk, [m.inst], m.proof[:-128]).queries
        return proof_ref.intermediate_sets([(q[0], q[1]) for q in qs])

    sets, T = shape("toy")
    assert proof_ref.n_sets(made("toy").cs) == 2 and max(len(p) for p, _ in sets) == 3  # a permutation z at x, wx, w^last x
    sets, T = shape("two_lookups")
    assert len(T) == 4  # rotation -1 among them
    sets, T = shape("gates_only")
    assert [len(p) for p, _ in sets] == [1, 1] and all(len(T) > len(p) for p, _ in sets)  # T \ S_i non-empty for both


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_reference_prover_to_reference_verifier(orc, made, name):
    m = made(name)
    nsets = proof_ref.n_point_sets(m.cs)
    assert shplonk(m.vk, [m.inst], m.proof) == 1
    assert m.proof[:-128] == m.gwc[:len(m.gwc) - 64 * nsets]
    assert len(m.proof) == proof_ref.proof_len(m.cs, N=1, scheme=SHPLONK) == len(m.gwc) - 64 * (nsets - 2)


def test_the_limit_circuits_are_past_the_limits(orc):
    for make, want_sets, want_points in ((seventeen_sets_circuit, 17, 5), (seventeen_points_circuit, None, 17)):
        cs, asg, _ = make()
        params = orc.params_new(cs.k, 1)
        vk_repr = orc.fr_from_int(5)
        fixed, sigma = asg.fixed_values(), asg.sigma_values()
        pk = orc.ProvingKey(cs.to_c(), fixed, sigma, params, vk_repr)
        st, gwc, _ = orc.create_proof(pk, asg.advice_values(), asg.instance_values(0), 3)
        assert st == 0 and proof_ref.n_point_sets(cs) == want_points
        vk = proof_ref.Vk(cs, params, fixed, sigma, vk_repr)
        qs = proof_ref.replay(vk, [asg.instance_values(0)], gwc[:len(gwc) - 64 * want_points]).queries
        sets, T = proof_ref.intermediate_sets([(q[0], q[1]) for q in qs])
        assert len(T) == want_points and (want_sets is None or len(sets) == want_sets)


def test_a_recorded_proof_of_two_circuits_through_the_n_circuit_verifier(orc):
    """the per-circuit loops of the replay, the (circuit, polynomial) identity of the rotation sets and verify for two circuits"""
    rec = json.load(open(GOLDEN_N2))
    family = toy_family(2)
    cs, asg, ilen = family[0]
    params = orc.params_new(cs.k, rec["params_seed"])
    vk = proof_ref.Vk(cs, params, asg.fixed_values(), asg.sigma_values(), orc.fr_from_int(rec["vk_repr"]))
    inst = [a.instance_values(ilen) for _, a, _ in family]
    proof = bytes.fromhex(rec["proof"])
    assert len(proof) == proof_ref.proof_len(cs, N=2, scheme=SHPLONK)
    qs = proof_ref.replay(vk, inst, proof[:-128]).queries
    sets, T = proof_ref.intermediate_sets([(q[0], q[1]) for q in qs])
    one = proof_ref.intermediate_sets([(q[0], q[1]) for q in qs if q[1][0] != 1])[0]  # without circuit 1's commitments
    assert [p for p, _ in sets] == [p for p, _ in one] and sum(len(k) for _, k in sets) > sum(len(k) for _, k in one)
    assert shplonk(vk, inst, proof) == 1
    assert shplonk(vk, [inst[1], inst[0]], proof) == 0
    g0 = params.g_np()[0]
    g0b = be32(orc.fq_to_int(g0[0:4])) + be32(orc.fq_to_int(g0[4:8]))
    assert shplonk(vk, inst, proof[:-128] + g0b + proof[-64:]) == 0
    assert shplonk(vk, inst, proof + b"\x00") == 0
    assert shplonk(vk, inst, proof[:-32]) == -1
    assert shplonk(vk, inst[:1], proof) != 1  # read as a proof of one circuit


def be32(x: int) -> bytes:
    return x.to_bytes(32, "big")


def test_verdict_classes(orc, made):
    m = made("toy")
    good = m.proof
    g0 = m.params.g_np()[0]
    g0b = be32(orc.fq_to_int(g0[0:4])) + be32(orc.fq_to_int(g0[4:8]))
    c = m.cs.to_c().c
    s0 = 64 * (c.n_advice + 3 * c.n_lookups + proof_ref.n_sets(m.cs) + 1 + c.cs_degree - 1)  # the first evaluation
    sc0 = int.from_bytes(good[s0:s0 + 32], "big")
    h2x = int.from_bytes(good[-64:-32], "big")
    cases = {
        "good": (good, 1),
        "h1 replaced by g0": (good[:-128] + g0b + good[-64:], 0),
        "one evaluation changed": (good[:s0] + be32((sc0 + 1) % R) + good[s0 + 32:], 0),
        "one trailing byte": (good + b"\x00", 0),
        "truncated": (good[:-32], -1),
        "h2 off the curve": (good[:-64] + be32((h2x + 1) % proof_ref.Q) + good[-32:], -1),
    }
    for name, (proof, want) in cases.items():
        assert shplonk(m.vk, [m.inst], proof) == want, name


def test_the_schemes_refuse_each_others_proofs(orc, made):
    for name in ("toy", "gates_only"):
        m = made(name)
        assert proof_ref.verify(m.vk, [m.inst], m.gwc).verdict == 1
        assert shplonk(m.vk, [m.inst], m.gwc) != 1
        assert proof_ref.verify(m.vk, [m.inst], m.proof).verdict != 1
        assert orc.verify_proof_pairing(m.pk, m.inst, m.proof) != 1
