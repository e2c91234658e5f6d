#!/usr/bin/env python3
"""Time ONE proof of N circuits against N proofs of one circuit each, for circuits with shuffles and with advice phases:
    python tools/circuits_time.py [--out PATH]

tests/shuffle_circuits.py wide(14) (one shuffle of width 4, plain entries) and tests/phases_circuits.py rlc_k14() (two phases,
one challenge, the phased entries), k = 14, one prover each in the throughput form, ONE process, one warm-up per shape and
five samples (host clock around the blocking calls) -- tools/multi_time.py's method.  For N in 1, 2, 4, 8, 16, 32,
alternating in the same process:
  prove_circuits(N) / prove_circuits_phased(N)        ms per image, proof bytes per image
  prove_batch(count = N) / prove_phased(count = N)    ms per image, proof bytes per image
  verify_circuits / verify                            ms per image of the proofs just made
Circuit c has witness variant c mod 3.  wide's columns are uploaded once and both forms prove the slots as they stand; rlc's
callback keeps the columns it made per (phase, variant, challenges), so a timed call -- whose challenges are the warm-up's,
the prover is deterministic -- pays the copies into the slots and no Python arithmetic, in both forms alike.  The comparison
is against the batch of the same tree and process.  No bar is set: the figures are recorded with the spread of their five
samples.  Writes profiles/r22/circuits_time.json (or PATH).  Needs a GPU: without one the context's creation raises."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("0g-halo2_amd", "oracle", "harness", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process)

import numpy as np  # noqa: E402
import orc  # noqa: E402
import phases_circuits  # noqa: E402
import shuffle_circuits  # noqa: E402
import zg_halo2 as zg  # noqa: E402
from circuit import to_mont_array  # noqa: E402

REPS = 5
SIZES = (1, 2, 4, 8, 16, 32)
NVAR = 3


def entry(times, per):
    med = statistics.median(times)
    return {"ms_per_image": round(med * 1e3 / per, 4), "median_ms": round(med * 1e3, 3),
            "min_ms": round(min(times) * 1e3, 3), "max_ms": round(max(times) * 1e3, 3),
            "samples_ms": [round(t * 1e3, 3) for t in times]}


def keeping(pc, variants):
    """pc.synthesize(variants) that makes each (phase, variant, challenges) witness once"""
    kept = {}

    def fn(phase, ch):
        out = []
        for b in range(ch.shape[0]):
            ints = tuple(orc.fr_to_int(ch[b, j]) for j in range(ch.shape[1]))
            key = (phase, variants[b], ints)
            if key not in kept:
                kept[key] = {c: to_mont_array(v) for c, v in pc.witness(phase, list(ints), variants[b]).items()}
            out.append(kept[key])
        return out

    return fn


def measure(ctx, pc, res):
    cs = pc.cs
    img = cs.to_c()
    params = orc.params_new(cs.k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    shuffles = getattr(img, "shuffles", None)
    bases = (ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np()))
    prover = zg.Prover(ctx, img, pc.fixed_values(), pc.sigma_values(), bases[0], bases[1], vk_repr, shuffles=shuffles)
    fc, sc = prover.vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr,
                           shuffles=shuffles)
    phased = pc.n_phases > 1
    if phased or pc.challenge_phase:
        prover.set_phases(pc.advice_phase, pc.challenge_phase)
        verifier.set_phases(pc.advice_phase, pc.challenge_phase)
    prover.set_overlap(False)
    prover.set_batch(max(SIZES))
    variants = [c % NVAR for c in range(max(SIZES))]
    insts = [pc.instance(v) for v in variants]
    if not phased:  # the columns into the slots, once
        advice = [pc.full_advice([0] * len(pc.challenge_phase), v) for v in range(NVAR)]
        _, sts = prover.prove_batch([advice[v] for v in variants], insts, list(range(max(SIZES))))
        assert sts == [0] * max(SIZES)
    synth = keeping(pc, variants)
    sizes = {}
    for n in SIZES:
        seeds = list(range(100, 100 + n))
        made = {}

        def one():
            if phased:
                made["one"], st = prover.prove_circuits_phased(synth, insts[:n], seeds)
                assert st == 0
            else:
                made["one"] = prover.prove_circuits(None, insts[:n], seeds, device=True)

        def batch():
            if phased:
                made["batch"], st = prover.prove_phased(synth, insts[:n], seeds)
                assert st == 0
            else:
                made["batch"], sts = prover.prove_batch(None, insts[:n], seeds, device=True)
                assert sts == [0] * n

        one()  # one warm-up per shape
        batch()
        t_one, t_batch = [], []
        for _ in range(REPS):  # alternating
            for fn, acc in ((one, t_one), (batch, t_batch)):
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        e = {"prove_circuits": entry(t_one, n), "prove_batch": entry(t_batch, n),
             "proof_bytes_per_image_circuits": round(len(made["one"]) / n, 1),
             "proof_bytes_per_image_batch": round(sum(len(p) for p in made["batch"]) / n, 1)}
        proof, ps = made["one"], made["batch"]
        assert verifier.verify_circuits([proof], [insts[:n]], 7, n) == [1] and verifier.verify(ps, insts[:n], 7) == [1] * n
        v_one, v_batch = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            verifier.verify_circuits([proof], [insts[:n]], 8, n)
            v_one.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            verifier.verify(ps, insts[:n], 8)
            v_batch.append(time.perf_counter() - t0)
        e["verify_circuits"] = entry(v_one, n)
        e["verify"] = entry(v_batch, n)
        e["circuits_over_batch"] = round(e["prove_circuits"]["ms_per_image"] / e["prove_batch"]["ms_per_image"], 4)
        sizes[str(n)] = e
        print(pc.name, n, json.dumps(e), flush=True)
    res["circuits"][pc.name] = {"entry": "prove_circuits_phased / prove_phased" if phased else "prove_circuits_dev / prove_batch_dev",
                                "advice": cs.n_advice, "shuffles": len(getattr(cs, "shuffles", [])), "degree": cs.degree(),
                                "phases": pc.n_phases, "challenges": len(pc.challenge_phase), "sizes": sizes}
    verifier.close()
    prover.close()
    for b in bases:
        b.free()


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r22", "circuits_time.json")
    orc.load().orc_set_threads(16)
    ctx = zg.Ctx(0)  # (raises without a GPU: the tool measures nothing on a CPU)
    res = {"k": 14, "reps": REPS, "device": torch.cuda.get_device_name(0), "circuits": {}}
    for pc in (shuffle_circuits.wide(14), phases_circuits.rlc_k14()):
        measure(ctx, pc, res)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
