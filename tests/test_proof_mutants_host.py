"""tests/proof_mutants.py against the reference verifier, without a device: over the four recorded proofs of
tests/golden/proof_*.json (one per multi-open and transcript pair) every element is found, every well-formed mutant is
REJECTED by the algebra -- not accepted, not called malformed -- and the encoding mutants fall into both rejecting classes.
The device tests (tests/test_gpu_verify_sweep.py) assert the same of their own inputs before they ask the device.

Tolerances: none -- verdict classes."""
import json
import os

import pytest

import phases_circuits
import proof_mutants
import proof_ref
import shuffle_circuits
from circuit import R
from transcript_ref import READER

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {  # file -> (scheme, transcript, elements: points + scalars of the proof)
    "proof_rlc_gwc_evm": (proof_ref.GWC, proof_ref.EVM, 24),
    "proof_three_phase_shplonk_blake2b": (proof_ref.SHPLONK, proof_ref.BLAKE2B, 29),
    "proof_wide_gwc_blake2b": (proof_ref.GWC, proof_ref.BLAKE2B, 27),
    "proof_with_challenge_shplonk_evm": (proof_ref.SHPLONK, proof_ref.EVM, 17),
}


def recorded(orc, name):
    rec = json.load(open(os.path.join(GOLDEN, name + ".json")))
    module, maker, kw = rec["circuit"]
    pc = getattr({"phases_circuits": phases_circuits, "shuffle_circuits": shuffle_circuits}[module], maker)(**kw)
    params = orc.params_new(pc.cs.k, rec["params_seed"])
    vk = proof_ref.Vk(pc.cs, params, pc.fixed_values(), pc.sigma_values(), orc.fr_from_int(rec["vk_repr"]))
    inst = pc.instance(0)

    def judge(p):
        return proof_ref.verify(vk, [inst], p, advice_phase=rec["advice_phase"], challenge_phase=rec["challenge_phase"],
                                scheme=rec["scheme"], transcript=rec["transcript"]).verdict

    return pc, rec, bytes.fromhex(rec["proof"]), judge


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_element_is_found_and_binds_in_the_reference(orc, name):
    scheme, transcript, elements = CASES[name]
    pc, rec, proof, judge = recorded(orc, name)
    assert (rec["scheme"], rec["transcript"]) == (scheme, transcript)
    sp = proof_mutants.spans(pc.cs, 1, scheme, transcript, pc.advice_phase)
    points, scalars = proof_ref.counts(pc.cs, 1, scheme)
    assert len(sp) == points + scalars == elements
    assert sp[0].offset == 0 and sp[-1].offset + sp[-1].length == len(proof)
    assert all(a.offset + a.length == b.offset for a, b in zip(sp, sp[1:]))
    # the names of the advice commitments are in the order the reference reads them
    assert [s.label for s in sp[:pc.cs.n_advice]] == ["adv c%d col%d" % (c, col) for _, c, col in proof_ref.advice_order(pc.cs, 1, pc.advice_phase)]
    assert judge(proof) == 1

    order = READER[transcript].byteorder
    mutants = list(proof_mutants.well_formed_mutants(proof, sp))
    assert sorted({m.span for m in mutants}) == list(range(len(sp)))  # no element left out
    assert len(mutants) == len(sp) + (points if transcript == proof_ref.BLAKE2B else 0)
    for m in mutants:
        s = sp[m.span]
        assert len(m.proof) == len(proof) and m.proof != proof, m.label
        assert m.proof[:s.offset] == proof[:s.offset] and m.proof[s.offset + s.length:] == proof[s.offset + s.length:], m.label
        if s.kind == proof_mutants.SCALAR:
            old = int.from_bytes(proof[s.offset:s.offset + 32], order)
            assert int.from_bytes(m.proof[s.offset:s.offset + 32], order) == (old + 1) % R, m.label
        assert judge(m.proof) == 0, m.label

    classes = {}
    for m in proof_mutants.encoding_mutants(proof, sp):
        v = judge(m.proof)
        assert v in (0, -1), (m.label, v)
        classes.setdefault(v, []).append(m.label)
    assert sorted(classes) == [-1, 0], classes
    assert "proof: the last byte cut off" in classes[-1] and "proof: one zero byte appended" in classes[0]


def test_spans_of_several_circuits_follow_the_reference_walk():
    """N = 3 of the circuit with every argument: the names come in replay's order and the families cover every label"""
    pc = shuffle_circuits.three()
    cs, N = pc.cs, 3
    for scheme in (proof_ref.GWC, proof_ref.SHPLONK):
        for transcript in (proof_ref.EVM, proof_ref.BLAKE2B):
            sp = proof_mutants.spans(cs, N, scheme, transcript)
            points, scalars = proof_ref.counts(cs, N, scheme)
            assert [s.kind for s in sp].count(proof_mutants.POINT) == points and len(sp) == points + scalars
            assert sp[-1].offset + sp[-1].length == proof_ref.proof_len(cs, N, scheme, transcript)
            assert {proof_mutants.family(s.label) for s in sp} == {name for name, _ in proof_mutants.FAMILIES}
            labels = [s.label for s in sp]
            for c in range(N):  # per circuit: 5 advice, 2 x 2 permuted, 1 pz, 2 lz, 3 sz commitments; 3 x 2 shuffle evaluations
                mine = [l for l in labels if (" c%d " % c) in l]
                assert len(mine) == 5 + 4 + 1 + 2 + 3 + len(cs.advice_queries) + 2 + 10 + 6, (c, mine)
            assert labels.index("sz c0 j2") + 1 == labels.index("sz c1 j0") and labels.index("lz c2 l1") + 1 == labels.index("sz c0 j0")
            assert labels.index("sh ev c1 j2 z(wx)") + 1 == labels.index("sh ev c2 j0 z(x)")
            tail = [l for l in labels if l.startswith("W ")]
            assert len(tail) == (2 if scheme == proof_ref.SHPLONK else proof_ref.n_point_sets(cs)) and labels[-len(tail):] == tail
    phased = shuffle_circuits.with_challenge(5, True)
    sp = proof_mutants.spans(phased.cs, 2, proof_ref.GWC, proof_ref.EVM, phased.advice_phase)
    assert [s.label for s in sp[:8]] == ["adv c%d col%d" % (c, col) for _, c, col in proof_ref.advice_order(phased.cs, 2, phased.advice_phase)]
