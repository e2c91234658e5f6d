"""zg_prover_prove_circuits / _dev / _phased and zg_verifier_verify_circuits without a device: the
layers that name the entries, and the reference verifier on recorded proofs of several circuits.

No CPU prover makes a proof of a circuit with shuffles or challenges, so tests/golden/circuits_proofs.json holds proofs
recorded from the device prover (tools/record_circuits_golden.py), k = 5.  tests/proof_ref.py -- the judge of the GPU tests
in tests/test_gpu_circuits.py -- accepts each of them with the recorded instances and rejects each with one byte flipped.
Two circuits' instances swapped are rejected too, where the circuit has an instance column: of the recorded circuits only
`rlc` has one (it is on file for that), for the others the swap changes nothing and the proof stays accepted."""
import json
import os
import re

import pytest

import phases_circuits
import proof_ref
import shuffle_circuits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "circuits_proofs.json")
ENTRIES = ("zg_prover_prove_circuits", "zg_prover_prove_circuits_dev", "zg_prover_prove_circuits_phased",
           "zg_verifier_verify_circuits")
GWC, SHPLONK, EVM, BLAKE2B = proof_ref.GWC, proof_ref.SHPLONK, proof_ref.EVM, proof_ref.BLAKE2B
RECORDED = [("three", 2, GWC, EVM), ("with_challenge_phased", 2, SHPLONK, BLAKE2B), ("interleaved", 3, GWC, EVM), ("rlc", 2, GWC, EVM)]


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_entries():
    header = read("include", "zg_halo2.h")
    for name in ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        args = decl.group(1)
        assert "size_t circuits" in args and "const zg_fr *const *instance" in args
        if name.startswith("zg_prover"):
            assert "uint8_t *proof," in args and "size_t proof_cap" in args and "size_t *proof_len" in args
        if name.endswith("_phased"):
            assert "zg_phase_fn fn" in args


def test_library_exports_the_entries(zg):
    lib = zg.load()
    for name in ENTRIES:
        assert name in zg.ABI_SYMBOLS and hasattr(lib, name), name
    for method in ("prove_circuits", "prove_circuits_phased"):
        assert callable(getattr(zg.Prover, method))
    assert callable(zg.Verifier.verify_circuits)


def test_generated_rust_block_contains_the_entries():
    rust = read("shim", "halo2_proofs-zg", "src", "zg_sys.rs")
    for name in ENTRIES:
        assert re.search(r"pub fn %s\(" % name, rust), name


def flip(proof, at):
    b = bytearray(proof)
    b[at] ^= 1
    return bytes(b)


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(GOLDEN) < 64 << 10
    return json.load(open(GOLDEN))


def test_the_file_holds_the_proofs_the_tests_name(golden):
    got = []
    for rec in golden["proofs"]:
        module, maker, kw = rec["circuit"]
        pc = getattr({"phases_circuits": phases_circuits, "shuffle_circuits": shuffle_circuits}[module], maker)(**kw)
        got.append((pc.name, rec["circuits"], rec["scheme"], rec["transcript"]))
    assert got == RECORDED
    assert sum(len(rec["proof"]) // 2 for rec in golden["proofs"]) < 16 << 10  # a few KB


@pytest.mark.parametrize("index", range(len(RECORDED)), ids=[r[0] for r in RECORDED])
def test_the_reference_accepts_the_recorded_proofs_and_rejects_tampered_ones(orc, golden, index):
    rec = golden["proofs"][index]
    module, maker, kw = rec["circuit"]
    pc = getattr({"phases_circuits": phases_circuits, "shuffle_circuits": shuffle_circuits}[module], maker)(**kw)
    cs, N = pc.cs, rec["circuits"]
    assert cs.k == 5 and (rec["advice_phase"], rec["challenge_phase"]) == (pc.advice_phase, pc.challenge_phase)
    params = orc.params_new(cs.k, golden["params_seed"])
    vk = proof_ref.Vk(cs, params, pc.fixed_values(), pc.sigma_values(), orc.fr_from_int(golden["vk_repr"]))
    insts = [pc.instance(c) for c in range(N)]  # circuit c has witness variant c
    assert [[[hex(orc.fr_to_int(v)) for v in col] for col in i] for i in insts] == rec["instances"]
    proof = bytes.fromhex(rec["proof"])
    assert len(proof) == proof_ref.proof_len(cs, N=N, scheme=rec["scheme"], transcript=rec["transcript"])

    def judge(p, instances=insts):
        return proof_ref.verify(vk, instances, p, advice_phase=pc.advice_phase, challenge_phase=pc.challenge_phase,
                                scheme=rec["scheme"], transcript=rec["transcript"])

    r = judge(proof)
    assert r.verdict == 1
    assert r.order == proof_ref.advice_order(cs, N, pc.advice_phase) and len(r.challenges) == len(pc.challenge_phase)
    assert len(r.shuffle_z) == N and all(len(z) == len(proof_ref.shuffles_of(cs)) for z in r.shuffle_z)
    # one byte flipped: in the first commitment, in the last evaluation (a shuffle's where the circuit has one), in the tail
    point_bytes = proof_ref.READER[rec["transcript"]].point_bytes
    points, scalars = proof_ref.counts(cs, N, rec["scheme"])
    tail = 2 if rec["scheme"] == SHPLONK else proof_ref.n_point_sets(cs)
    last_eval = point_bytes * (points - tail) + 32 * scalars - 1
    for at in (5, last_eval, len(proof) - 3):
        assert judge(flip(proof, at)).verdict <= 0, at
    assert judge(proof[:-1]).verdict == -1 and judge(proof + b"\x00").verdict == 0
    # two circuits' instances swapped
    swapped = [insts[1], insts[0]] + insts[2:]
    if cs.n_instance:
        assert insts[0].tobytes() != insts[1].tobytes()
        assert judge(proof, swapped).verdict == 0
    else:
        assert all(i.size == 0 for i in insts) and judge(proof, swapped).verdict == 1
    # ... and a proof of N circuits is none of N - 1 or N + 1
    assert judge(proof, insts[:-1]).verdict <= 0 and judge(proof, insts + [insts[0]]).verdict <= 0

