"""The phase, challenge and shuffle branches of tests/proof_ref.py without a device.  The oracle knows neither challenges
nor shuffles and no CPU prover makes such proofs, so tests/golden/proof_*.json hold four small proofs (k = 5) recorded from
the device prover (tests/golden/make_proof_golden.py), one per (multi-open, transcript) pair, each with what the comparator
that proof_ref replaced -- phases_ref.verify or shuffle_ref.verify, one copy of the walk per proof form -- returned for it
and for five inputs derived from it.  proof_ref.verify reproduces every recorded field and verdict: the merged walk is
what the copies were.  The circuit is rebuilt from code and the key from orc.params_new."""
import json
import os

import pytest

import phases_circuits
import proof_ref
import shuffle_circuits
from circuit import R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LARGEST_FIXTURE = 58839  # tests/golden/vectors.json
CASES = {  # file -> (scheme, transcript)
    "proof_rlc_gwc_evm": (proof_ref.GWC, proof_ref.EVM),
    "proof_three_phase_shplonk_blake2b": (proof_ref.SHPLONK, proof_ref.BLAKE2B),
    "proof_wide_gwc_blake2b": (proof_ref.GWC, proof_ref.BLAKE2B),
    "proof_with_challenge_shplonk_evm": (proof_ref.SHPLONK, proof_ref.EVM),
}


def flip(proof, at):
    b = bytearray(proof)
    b[at] ^= 1
    return bytes(b)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_reference_reproduces_what_the_replaced_comparators_returned(orc, name):
    path = os.path.join(GOLDEN, name + ".json")
    assert os.path.getsize(path) <= LARGEST_FIXTURE
    rec = json.load(open(path))
    module, maker, kw = rec["circuit"]
    pc = getattr({"phases_circuits": phases_circuits, "shuffle_circuits": shuffle_circuits}[module], maker)(**kw)
    cs, want = pc.cs, rec["expected"]
    assert (rec["scheme"], rec["transcript"]) == CASES[name] and cs.k == 5
    assert (rec["advice_phase"], rec["challenge_phase"]) == (pc.advice_phase, pc.challenge_phase)
    params = orc.params_new(cs.k, rec["params_seed"])
    vk = proof_ref.Vk(cs, params, pc.fixed_values(), pc.sigma_values(), orc.fr_from_int(rec["vk_repr"]))
    inst = pc.instance(0)
    assert [[hex(orc.fr_to_int(v)) for v in col] for col in inst] == rec["instance"]
    proof = bytes.fromhex(rec["proof"])
    assert len(proof) == proof_ref.proof_len(cs, N=1, scheme=rec["scheme"], transcript=rec["transcript"])

    def judge(p, instance=inst):
        return proof_ref.verify(vk, [instance], p, advice_phase=rec["advice_phase"], challenge_phase=rec["challenge_phase"],
                                scheme=rec["scheme"], transcript=rec["transcript"])

    r = judge(proof)
    assert r.verdict == want["verdict"] == 1
    assert {str(j): hex(v) for j, v in r.challenges.items()} == want["challenges"] and len(r.challenges) == len(pc.challenge_phase)
    assert [list(o) for o in r.order] == want["order"] == [list(o) for o in proof_ref.advice_order(cs, 1, pc.advice_phase)]
    if module == "shuffle_circuits":
        assert {k: hex(v) for k, v in r.named.items()} == want["named"]
        got = [[proof_ref.affine(p) for p in c] for c in r.shuffle_z]
        assert [[[hex(orc.fq_to_int(a[0:4])), hex(orc.fq_to_int(a[4:8]))] for a in c] for c in got] == want["shuffle_z"]
        assert len(want["shuffle_z"]) == 1 and len(want["shuffle_z"][0]) == len(cs.shuffles) > 0
    derived = {"bit 0 of byte 5 flipped": judge(flip(proof, 5)).verdict,
               "bit 0 of byte -70 flipped": judge(flip(proof, len(proof) - 70)).verdict,
               "the last byte cut off": judge(proof[:-1]).verdict,
               "one zero byte appended": judge(proof + b"\x00").verdict}
    if cs.n_instance:
        wrong = inst.copy()
        wrong[0, 0] = orc.fr_from_int((orc.fr_to_int(inst[0, 0]) + 1) % R)
        derived["a wrong first instance value"] = judge(proof, wrong).verdict
    assert derived == want["derived"]
    assert derived["the last byte cut off"] == -1 and derived["one zero byte appended"] == 0  # with the 1 above: every class
