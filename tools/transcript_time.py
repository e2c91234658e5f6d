#!/usr/bin/env python3
"""Time halo2's Blake2b transcript (compressed points) against the EvmTranscript:   python tools/transcript_time.py [--out PATH]

Tiny model, k = 14, ONE process, two provers of the same tree on the same base tables -- one per transcript -- and one
verifier switched between them.  Per item a warm-up of each transcript, then REPS rounds that ALTERNATE EVM and Blake2b;
host clock around the blocking calls (each ends in the proof bytes / the verdicts on the host):
  proof sizes under the four (transcript, multi-open) settings
  prove_images, batch 32, throughput form                     ms per proof
  a lone proof, latency form (prove_dev of a slot)            ms
  verify, batch 32                                            ms per batch, and the kernels' shares of one batch
                                                              (zg_ctx_profile_*: g1_decompress, verify_replay, the rest)
  zg_g1_decompress_dev at n = 2^14 and 2^17                   points per second
No bar is set: medians with the minimum, maximum and every sample are recorded, and the ratio of the medians.  Writes
profiles/r17/transcript_time.json (or PATH).  Needs a GPU: without one the context's creation raises."""
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
TRANSCRIPTS = (("evm", zg.TRANSCRIPT_EVM), ("blake2b", zg.TRANSCRIPT_BLAKE2B))


def entry(times, per):
    med = statistics.median(times)
    return {"ms_per_item": round(med * 1e3 / per, 4), "median_ms": round(med * 1e3, 3), "min_ms": round(min(times) * 1e3, 3),
            "max_ms": round(max(times) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times]}


def alternate(fns, per):
    """fns: {name: callable}; one warm-up each, then REPS alternating rounds"""
    for fn in fns.values():
        fn()
    times = {name: [] for name in fns}
    for _ in range(REPS):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    out = {name: entry(t, per) for name, t in times.items()}
    names = list(fns)
    out["%s_over_%s" % (names[1], names[0])] = round(out[names[1]]["median_ms"] / out[names[0]]["median_ms"], 4)
    return out


def timed(fn, per):
    fn()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return entry(times, per)


def decompress_rates(ctx, real_points):
    """points per second on compressed multiples of real commitments with one invalid lane in 64 (launch + synchronise)"""
    res = {}
    for log_n in (14, 17):
        n = 1 << log_n
        scalars = np.stack([zg.fr_from_int(3 + 5 * i) for i in range(n)])
        pts = ctx.g1_mul_each(np.tile(real_points, ((n + len(real_points) - 1) // len(real_points), 1))[:n], scalars)
        enc = zg.g1_compress(pts)
        enc[63::64, 31] |= 0x40  # bit 6: an invalid encoding per wave
        d_in = torch.from_numpy(enc).cuda()
        d_out = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        d_valid = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def run():
            ctx.g1_decompress_dev(d_in.data_ptr(), n, d_out.data_ptr(), d_valid.data_ptr())
            ctx.sync()

        r = timed(run, 1)
        assert int(d_valid.sum()) == n - n // 64
        assert np.array_equal(zg.g1_compress(d_out.cpu().numpy().view(np.uint64)[:63]), enc[:63])
        r["points_per_s"] = round(n / (r["median_ms"] * 1e-3))
        res["n=2^%d" % log_n] = r
    return res


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r17", "transcript_time.json")
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
    for tname, transcript in TRANSCRIPTS:
        p = zg.Prover(ctx, img, fixed, sigma, bases[0], bases[1], vk_repr)
        p.set_batch(32)
        p.set_transcript(transcript)
        provers[tname] = p
    plan = zg.WitnessPlan(ctx, witness_tape.trace(wnn, k).arrays())
    fc, sc = provers["evm"].vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr)
    rng = np.random.default_rng(11)
    images = np.stack([real] + [rng.integers(0, 256, size=real.shape, dtype=real.dtype) for _ in range(31)])
    seeds = list(range(100, 132))
    res = {"model": name, "k": k, "reps": REPS, "device": torch.cuda.get_device_name(0)}

    # ---- proof sizes: the four settings, each proof accepted by the verifier set the same way
    res["proof_bytes"] = {}
    for tname, transcript in TRANSCRIPTS:
        for sname, scheme in (("gwc", zg.MULTIOPEN_GWC), ("shplonk", zg.MULTIOPEN_SHPLONK)):
            provers[tname].set_multiopen(scheme)
            verifier.set_multiopen(scheme)
            verifier.set_transcript(transcript)
            proof = provers[tname].prove(adv, inst, 7)
            assert verifier.verify([proof], [inst], 3) == [1]
            res["proof_bytes"]["%s+%s" % (tname, sname)] = len(proof)
        provers[tname].set_multiopen(zg.MULTIOPEN_GWC)
    verifier.set_multiopen(zg.MULTIOPEN_GWC)
    print("proof_bytes", json.dumps(res["proof_bytes"]), flush=True)

    # ---- throughput form: a batch of 32 single proofs
    made = {}
    for p in provers.values():
        p.set_overlap(False)

    def batch(tname):
        ps, outs, sts = provers[tname].prove_images(plan, images, seeds)
        assert sts == [0] * 32
        made[tname] = (ps, outs)

    res["prove_images_batch32"] = alternate({t: (lambda t=t: batch(t)) for t, _ in TRANSCRIPTS}, 32)
    print("prove_images_batch32", json.dumps(res["prove_images_batch32"]), flush=True)

    # ---- verification of what was just made
    def verify(tname):
        ps, outs = made[tname]
        verifier.set_transcript(dict(TRANSCRIPTS)[tname])
        assert verifier.verify(ps, [o[None, :, :] for o in outs], 7) == [1] * 32

    res["verify_batch32"] = alternate({t: (lambda t=t: verify(t)) for t, _ in TRANSCRIPTS}, 1)
    print("verify_batch32", json.dumps(res["verify_batch32"]), flush=True)
    res["verify_batch32_kernels_ms"] = {}
    for tname, _ in TRANSCRIPTS:
        ctx.profile(True)
        ctx.profile_collect()
        verify(tname)
        stats = ctx.profile_collect()
        ctx.profile(False)
        res["verify_batch32_kernels_ms"][tname] = {kn: round(v[1], 4) for kn, v in sorted(stats.items())}
    print("verify_batch32_kernels_ms", json.dumps(res["verify_batch32_kernels_ms"]), flush=True)

    # ---- latency form: a lone proof (the advice columns already in the prover's slot; no digit tables)
    lone = {}
    for p in provers.values():
        p.set_overlap(True)
        p.prove(adv, inst, 7)

    def prove_lone(tname):
        lone[tname] = provers[tname].prove_dev(provers[tname].advice_slot(0), inst, 7)

    res["lone_proof"] = alternate({t: (lambda t=t: prove_lone(t)) for t, _ in TRANSCRIPTS}, 1)
    print("lone_proof", json.dumps(res["lone_proof"]), flush=True)

    # ---- the decompression kernel alone
    res["g1_decompress_dev"] = decompress_rates(ctx, np.concatenate([fc, sc])[:8] if len(fc) + len(sc) else params.g_np()[:8])
    print("g1_decompress_dev", json.dumps(res["g1_decompress_dev"]), flush=True)

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
