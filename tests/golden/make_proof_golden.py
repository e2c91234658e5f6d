#!/usr/bin/env python3
"""Writes the recorded proofs tests/golden/proof_*.json -- needs a GPU; run from the repo root:
    python tests/golden/make_proof_golden.py [output directory]

One small proof (k = 5) per file from the device prover, for circuits no CPU prover can prove: advice phases with
challenges and shuffles, under both multi-open arguments and both transcripts.  tests/test_proof_golden_host.py rebuilds
each circuit from code, takes the key from orc.params_new and holds the reference verifier (tests/proof_ref.py) to the
file's "expected" block: what the comparators that proof_ref replaced (phases_ref.verify, shuffle_ref.verify) returned for
the proof and for five inputs derived from it.  This script only proves and writes; it keeps a file's "expected" block as
long as the proof's bytes are the ones on file (the prover is deterministic in its seeds)."""
import json
import os
import sys

import torch  # noqa: F401 -- before the library: one HIP runtime in the process (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for sub in ("tests", "harness", "oracle", "0g-halo2_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import orc  # noqa: E402
import phases_circuits  # noqa: E402
import shuffle_circuits  # noqa: E402
import zg_halo2 as zg  # noqa: E402

GWC, SHPLONK, EVM, BLAKE2B = 0, 1, 0, 1
PARAMS_SEED, VK_REPR = 0xABCDEF, 0x1234567

# file name -> (module, maker, arguments, scheme, transcript, blinding seed)
CASES = {
    "proof_rlc_gwc_evm": ("phases_circuits", "rlc", {"k": 5}, GWC, EVM, 51),
    "proof_three_phase_shplonk_blake2b": ("phases_circuits", "three_phase", {"k": 5}, SHPLONK, BLAKE2B, 52),
    "proof_wide_gwc_blake2b": ("shuffle_circuits", "wide", {"k": 5}, GWC, BLAKE2B, 53),
    "proof_with_challenge_shplonk_evm": ("shuffle_circuits", "with_challenge", {"k": 5, "phased": True}, SHPLONK, EVM, 54),
}


def prove(ctx, pc, scheme, transcript, seed) -> bytes:
    img = pc.cs.to_c()
    params = orc.params_new(pc.cs.k, PARAMS_SEED)
    prover = zg.Prover(ctx, img, pc.fixed_values(), pc.sigma_values(), params.g_np(), params.g_lagrange_np(),
                       orc.fr_from_int(VK_REPR), shuffles=getattr(img, "shuffles", None))
    prover.set_multiopen(scheme)
    prover.set_transcript(transcript)
    try:
        if pc.n_phases > 1:
            prover.set_phases(pc.advice_phase, pc.challenge_phase)
            (proof,), st = prover.prove_phased(pc.synthesize([0]), [pc.instance(0)], [seed])
            assert st == 0
            return proof
        return prover.prove(pc.full_advice([0] * len(pc.challenge_phase), 0), pc.instance(0), seed)
    finally:
        prover.close()


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    orc.load()
    zg.load()
    ctx = zg.Ctx(0)
    for name, (module, maker, kw, scheme, transcript, seed) in CASES.items():
        pc = getattr({"phases_circuits": phases_circuits, "shuffle_circuits": shuffle_circuits}[module], maker)(**kw)
        proof = prove(ctx, pc, scheme, transcript, seed)
        inst = pc.instance(0)
        rec = {"what": "%s.%s(%s), variant 0, k = 5" % (module, maker, ", ".join("%s=%r" % kv for kv in kw.items())),
               "circuit": [module, maker, kw], "params_seed": PARAMS_SEED, "vk_repr": VK_REPR, "seed": seed,
               "scheme": scheme, "transcript": transcript,
               "advice_phase": pc.advice_phase, "challenge_phase": pc.challenge_phase,
               "instance": [[hex(orc.fr_to_int(v)) for v in col] for col in inst],
               "proof": proof.hex()}
        path = os.path.join(out_dir, name + ".json")
        if os.path.exists(path):
            old = json.load(open(path))
            if old.get("proof") == rec["proof"] and "expected" in old:
                rec["expected"] = old["expected"]
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print("wrote", path, len(proof), "proof bytes", "" if "expected" in rec else "(no expected block)")
    ctx.close()
