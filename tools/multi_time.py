#!/usr/bin/env python3
"""Time ONE proof of N images against N proofs of one image each:   python tools/multi_time.py [--out PATH] [--short]

Tiny model, k = 14, one prover in the throughput form, ONE process, one warm-up per shape and five samples (host clock
around the blocking calls).  For N in 1, 2, 4, 8, 16, 32, alternating in the same process:
  prove_images_multi(N)      ms per image, proof bytes per image
  prove_images(count = N)    ms per image, proof bytes per image
  verify_multi / verify      ms per image of the proofs just made
The comparison is against prove_images of the same tree and process.  No bar is set: the figures are recorded with the
spread of their five samples.  Writes profiles/r11/multi_time.json (or PATH).  --short: N = 32 of both provers only (the
run rocprofv3 --kernel-trace --stats wraps for the fold and combine kernels' times).  Needs a GPU: without one the
context's creation raises."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("0g-halo2_amd", "oracle", "harness"):
    sys.path.insert(0, os.path.join(ROOT, d))
import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process)

import numpy as np  # noqa: E402
import orc  # noqa: E402
import witness_tape  # noqa: E402
import wnn_circuit  # noqa: E402
import wnn_model  # noqa: E402
import zg_halo2 as zg  # noqa: E402

REPS = 5
SIZES = (1, 2, 4, 8, 16, 32)


def entry(times, per):
    med = statistics.median(times)
    return {"ms_per_image": round(med * 1e3 / per, 4), "median_ms": round(med * 1e3, 3),
            "min_ms": round(min(times) * 1e3, 3), "max_ms": round(max(times) * 1e3, 3),
            "samples_ms": [round(t * 1e3, 3) for t in times]}


def main():
    short = "--short" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r11", "multi_time.json")
    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    wnn = wnn_model.load_checked_in(name)
    real = wnn_model.load_test_image()
    cs, asg, ilen, _ = wnn_circuit.build(wnn, real, k)
    img = cs.to_c()
    params = orc.params_new(k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    ctx = zg.Ctx(0)  # (raises without a GPU: the tool measures nothing on a CPU)
    bases = (ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np()))
    prover = zg.Prover(ctx, img, fixed, sigma, bases[0], bases[1], vk_repr)
    prover.set_overlap(False)
    prover.set_batch(32)
    plan = zg.WitnessPlan(ctx, witness_tape.trace(wnn, k).arrays())
    fc, sc = prover.vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr)
    rng = np.random.default_rng(11)
    images = np.stack([real] + [rng.integers(0, 256, size=real.shape, dtype=real.dtype) for _ in range(31)])
    res = {"model": name, "k": k, "reps": REPS, "device": torch.cuda.get_device_name(0), "sizes": {}}

    for n in ((32,) if short else SIZES):
        seeds = list(range(100, 100 + n))
        made = {}

        def multi():
            made["multi"] = prover.prove_images_multi(plan, images[:n], seeds)

        def batch():
            ps, outs, sts = prover.prove_images(plan, images[:n], seeds)
            assert sts == [0] * n
            made["batch"] = (ps, outs)

        multi()  # one warm-up per shape
        batch()
        t_multi, t_batch = [], []
        for _ in range(REPS):  # alternating
            for fn, acc in ((multi, t_multi), (batch, t_batch)):
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        e = {"prove_images_multi": entry(t_multi, n), "prove_images": entry(t_batch, n),
             "proof_bytes_per_image_multi": round(len(made["multi"][0]) / n, 1),
             "proof_bytes_per_image_batch": round(sum(len(p) for p in made["batch"][0]) / n, 1)}
        if not short:
            proof, outs = made["multi"]
            insts = [o[None, :, :] for o in outs]
            ps, bouts = made["batch"]
            binsts = [o[None, :, :] for o in bouts]
            assert verifier.verify_multi([proof], [insts], 7, n) == [1] and verifier.verify(ps, binsts, 7) == [1] * n
            v_multi, v_batch = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                verifier.verify_multi([proof], [insts], 8, n)
                v_multi.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                verifier.verify(ps, binsts, 8)
                v_batch.append(time.perf_counter() - t0)
            e["verify_multi"] = entry(v_multi, n)
            e["verify"] = entry(v_batch, n)
        e["multi_over_batch"] = round(e["prove_images_multi"]["ms_per_image"] / e["prove_images"]["ms_per_image"], 4)
        res["sizes"][str(n)] = e
        print(n, json.dumps(e), flush=True)

    plan.close()
    verifier.close()
    prover.close()
    ctx.close()
    if not short:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
