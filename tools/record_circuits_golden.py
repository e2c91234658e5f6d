#!/usr/bin/env python3
"""Writes tests/golden/circuits_proofs.json -- needs a GPU; run from the repo root:
    python tools/record_circuits_golden.py [output file]

Proofs of SEVERAL circuits behind one transcript (zg_prover_prove_circuits*) for circuits with
shuffles, challenges and advice phases, k = 5, recorded from the device prover: no CPU prover makes them.
tests/test_circuits_host.py rebuilds each circuit from code, takes the key from orc.params_new and holds the recorded bytes
to the reference verifier (tests/proof_ref.py).  Circuit c of a proof has witness variant c and blinding seed SEED + c."""
import json
import os
import sys

import torch  # noqa: F401 -- before the library: one HIP runtime in the process (tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "harness", "oracle", "0g-halo2_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import orc  # noqa: E402
import phases_circuits  # noqa: E402
import shuffle_circuits  # noqa: E402
import zg_halo2 as zg  # noqa: E402

GWC, SHPLONK, EVM, BLAKE2B = 0, 1, 0, 1
PARAMS_SEED, VK_REPR, SEED = 0xABCDEF, 0x1234567, 60

# (module, maker, arguments, circuits, scheme, transcript); the last one is there for its instance column
CASES = [
    ("shuffle_circuits", "three", {"k": 5}, 2, GWC, EVM),
    ("shuffle_circuits", "with_challenge", {"k": 5, "phased": True}, 2, SHPLONK, BLAKE2B),
    ("phases_circuits", "interleaved", {"k": 5}, 3, GWC, EVM),
    ("phases_circuits", "rlc", {"k": 5}, 2, GWC, EVM),
]


def prove(ctx, pc, N, scheme, transcript) -> bytes:
    img = pc.cs.to_c()
    params = orc.params_new(pc.cs.k, PARAMS_SEED)
    prover = zg.Prover(ctx, img, pc.fixed_values(), pc.sigma_values(), params.g_np(), params.g_lagrange_np(),
                       orc.fr_from_int(VK_REPR), shuffles=getattr(img, "shuffles", None))
    prover.set_multiopen(scheme)
    prover.set_transcript(transcript)
    prover.set_batch(N)
    variants, seeds = list(range(N)), [SEED + c for c in range(N)]
    insts = [pc.instance(v) for v in variants]
    try:
        if pc.n_phases > 1:
            prover.set_phases(pc.advice_phase, pc.challenge_phase)
            proof, st = prover.prove_circuits_phased(pc.synthesize(variants), insts, seeds)
            assert st == 0
            return proof
        return prover.prove_circuits([pc.full_advice([0] * len(pc.challenge_phase), v) for v in variants], insts, seeds)
    finally:
        prover.close()


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "circuits_proofs.json")
    orc.load()
    zg.load()
    ctx = zg.Ctx(0)
    recs = []
    for module, maker, kw, N, scheme, transcript in CASES:
        pc = getattr({"phases_circuits": phases_circuits, "shuffle_circuits": shuffle_circuits}[module], maker)(**kw)
        proof = prove(ctx, pc, N, scheme, transcript)
        recs.append({"circuit": [module, maker, kw], "circuits": N, "scheme": scheme, "transcript": transcript,
                     "advice_phase": pc.advice_phase, "challenge_phase": pc.challenge_phase,
                     "instances": [[[hex(orc.fr_to_int(v)) for v in col] for col in pc.instance(c)] for c in range(N)],
                     "proof": proof.hex()})
        print("%s.%s N = %d: %d proof bytes" % (module, maker, N, len(proof)))
    ctx.close()
    with open(out, "w") as f:
        json.dump({"what": "zg_prover_prove_circuits*: circuit c has witness variant c and blinding seed %d + c" % SEED,
                   "params_seed": PARAMS_SEED, "vk_repr": VK_REPR, "seed": SEED, "proofs": recs}, f, indent=1)
        f.write("\n")
    print("wrote", out)
