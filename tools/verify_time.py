#!/usr/bin/env python3
"""Time batched GWC verification on the device against the oracle's CPU verifier:   python tools/verify_time.py [--out PATH]

Makes 384 tiny-model proofs with the throughput form, then times Verifier.verify (transcript replay, scalars and terms
on the GPU, one host pairing check) for batches of 1, 32 and 384, and the oracle's verify_proof_pairing per proof on 16
threads.  Writes profiles/r06/verify_time.json (or PATH)."""
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
import wnn_circuit  # noqa: E402
import wnn_model  # noqa: E402
import zg_halo2 as zg  # noqa: E402


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r06", "verify_time.json")
    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    cs, asg, ilen, _ = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), k)
    img = cs.to_c()
    params = orc.params_new(k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    ctx = zg.Ctx(0)
    prover = zg.Prover(ctx, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr)
    fc, sc = prover.vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64),
                           vk_repr)
    prover.set_batch(64)
    prover.set_overlap(False)
    proofs = []
    for j in range(6):
        ps, _ = prover.prove_batch([adv] * 64, [inst] * 64, list(range(1000 + 64 * j, 1064 + 64 * j)))
        proofs += ps
    res = {"model": name, "k": k, "proof_bytes": len(proofs[0]), "batches": {}}
    for batch in (1, 32, 384):
        sub, insts = proofs[:batch], [inst] * batch
        assert verifier.verify(sub, insts, 1) == [1] * batch  # (warm: buffers, code objects)
        times = []
        for rep in range(5):
            t0 = time.perf_counter()
            v = verifier.verify(sub, insts, 2 + rep)
            times.append(time.perf_counter() - t0)
            assert v == [1] * batch
        med = statistics.median(times)
        res["batches"][str(batch)] = {"median_ms": round(med * 1e3, 3), "ms_per_proof": round(med * 1e3 / batch, 4),
                                      "samples_ms": [round(t * 1e3, 3) for t in times]}
        print(batch, res["batches"][str(batch)], flush=True)
    # the failure path: one bad proof (a W taken from another proof) in 32 and in 384: the batch is bisected
    for batch in (32, 384):
        bad = list(proofs[:batch])
        bad[7] = bad[7][:-64] + bad[8][-64:]
        t0 = time.perf_counter()
        v = verifier.verify(bad, [inst] * batch, 9)
        res[f"batch{batch}_one_bad_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert v[7] == 0 and v.count(1) == batch - 1
        print(f"batch {batch} with one bad proof", res[f"batch{batch}_one_bad_ms"], "ms", flush=True)
    pk = orc.ProvingKey(img, fixed, sigma, params, vk_repr)
    ot = []
    for p in proofs[:3]:
        t0 = time.perf_counter()
        assert orc.verify_proof_pairing(pk, inst, p) == 1
        ot.append(time.perf_counter() - t0)
    res["oracle_verify_proof_pairing_ms"] = {"threads": 16, "median_ms": round(statistics.median(ot) * 1e3, 3),
                                             "samples_ms": [round(t * 1e3, 3) for t in ot]}
    res["bar_ms_per_proof"] = 0.67
    res["device"] = torch.cuda.get_device_name(0)
    verifier.close()
    prover.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
