#!/usr/bin/env python3
"""Time the SHPLONK multi-open against GWC:   python tools/shplonk_time.py [--out PATH]

Tiny model, k = 14, ONE process, two provers of the same tree on the same base tables -- one per scheme -- and one
verifier switched between the schemes.  Per item a warm-up of each scheme, then REPS rounds that ALTERNATE GWC and SHPLONK;
host clock around the blocking calls (each ends in the proof bytes / the verdicts on the host):
  prove_images, batch 32, throughput form           ms per proof
  a lone proof, latency form (prove_dev of a slot; the bucket form, no digit tables)   ms
  prove_images_multi, N = 32, throughput form        ms per image
  verify, batch 1 and batch 384                      ms per proof
No bar is set: medians with the minimum, maximum and every sample are recorded, and the ratio of the medians.  Writes
profiles/r16/shplonk_time.json (or PATH).  Needs a GPU: without one the context's creation raises."""
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

REPS = 7
SCHEMES = (("gwc", zg.MULTIOPEN_GWC), ("shplonk", zg.MULTIOPEN_SHPLONK))


def entry(times, per):
    med = statistics.median(times)
    return {"ms_per_item": round(med * 1e3 / per, 4), "median_ms": round(med * 1e3, 3), "min_ms": round(min(times) * 1e3, 3),
            "max_ms": round(max(times) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times]}


def alternate(fns, per):
    """fns: {scheme name: callable}; one warm-up each, then REPS alternating rounds"""
    for fn in fns.values():
        fn()
    times = {name: [] for name in fns}
    for _ in range(REPS):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    out = {name: entry(t, per) for name, t in times.items()}
    out["shplonk_over_gwc"] = round(out["shplonk"]["median_ms"] / out["gwc"]["median_ms"], 4)
    return out


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r16", "shplonk_time.json")
    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    wnn = wnn_model.load_checked_in(name)
    real = wnn_model.load_test_image()
    cs, asg, ilen, _ = wnn_circuit.build(wnn, real, k)
    img = cs.to_c()
    params = orc.params_new(k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    ctx = zg.Ctx(0)  # (raises without a GPU: the tool measures nothing on a CPU)
    bases = (ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np()))
    provers = {}
    for sname, scheme in SCHEMES:
        p = zg.Prover(ctx, img, fixed, sigma, bases[0], bases[1], vk_repr)
        p.set_batch(32)
        p.set_multiopen(scheme)
        provers[sname] = p
    plan = zg.WitnessPlan(ctx, witness_tape.trace(wnn, k).arrays())
    fc, sc = provers["gwc"].vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr)
    rng = np.random.default_rng(11)
    images = np.stack([real] + [rng.integers(0, 256, size=real.shape, dtype=real.dtype) for _ in range(31)])
    seeds = list(range(100, 132))
    res = {"model": name, "k": k, "reps": REPS, "device": torch.cuda.get_device_name(0)}
    made = {}

    # ---- throughput form: a batch of 32 single proofs, one proof of 32 circuits
    for p in provers.values():
        p.set_overlap(False)

    def batch(sname):
        ps, outs, sts = provers[sname].prove_images(plan, images, seeds)
        assert sts == [0] * 32
        made[sname] = (ps, outs)

    res["prove_images_batch32"] = alternate({s: (lambda s=s: batch(s)) for s, _ in SCHEMES}, 32)
    res["proof_bytes"] = {s: len(made[s][0][0]) for s, _ in SCHEMES}
    print("prove_images_batch32", json.dumps(res["prove_images_batch32"]), flush=True)

    multi = {}

    def prove_multi(sname):
        multi[sname] = provers[sname].prove_images_multi(plan, images, seeds)

    res["prove_images_multi32"] = alternate({s: (lambda s=s: prove_multi(s)) for s, _ in SCHEMES}, 32)
    res["proof_bytes_multi32"] = {s: len(multi[s][0]) for s, _ in SCHEMES}
    print("prove_images_multi32", json.dumps(res["prove_images_multi32"]), flush=True)

    # ---- verification of what was just made: one proof, and 384 (the 32 proofs twelve times over)
    def verify(sname, count):
        ps, outs = made[sname]
        insts = [o[None, :, :] for o in outs]
        reps = (count + 31) // 32
        verifier.set_multiopen(dict(SCHEMES)[sname])
        assert verifier.verify((ps * reps)[:count], (insts * reps)[:count], 7) == [1] * count

    for count in (1, 384):
        res[f"verify_batch{count}"] = alternate({s: (lambda s=s: verify(s, count)) for s, _ in SCHEMES}, count)
        print(f"verify_batch{count}", json.dumps(res[f"verify_batch{count}"]), flush=True)
    for sname, scheme in SCHEMES:  # one proof of 32 circuits under each scheme's verifier
        verifier.set_multiopen(scheme)
        proof, outs = multi[sname]
        assert verifier.verify_multi([proof], [[o[None, :, :] for o in outs]], 7, 32) == [1]

    # ---- latency form: a lone proof
    # (the advice columns already in the prover's slot, as a caller of the witness kernels has them; no digit tables)
    lone = {}
    for p in provers.values():
        p.set_overlap(True)
        p.prove(adv, inst, 7)

    def prove_lone(sname):
        lone[sname] = provers[sname].prove_dev(provers[sname].advice_slot(0), inst, 7)

    res["lone_proof"] = alternate({s: (lambda s=s: prove_lone(s)) for s, _ in SCHEMES}, 1)
    res["proof_bytes_lone"] = {s: len(lone[s]) for s, _ in SCHEMES}
    print("lone_proof", json.dumps(res["lone_proof"]), flush=True)

    plan.close()
    verifier.close()
    for p in provers.values():
        p.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
