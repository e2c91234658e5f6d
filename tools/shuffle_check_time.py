#!/usr/bin/env python3
"""Time the witness check of circuits with shuffles against proving and verifying them:
    python tools/shuffle_check_time.py [--out PATH] [--parent-json PATH] [--prove-verify-only] [--short]

`wide(14, high_gate=True)` and `three(14)` of tests/shuffle_circuits.py, ONE process, a warm-up and five samples each (host
clock around blocking calls), at batch 1 and batch 32, the witnesses resident in the prover's slots:
  check_satisfied      zg_prover_check_circuit_dev on the slots as they stand, every witness a shuffle: ms per witness;
  check_one_bad        the same with the BAD variant in slot 0, cap 64 (bitmap and partner rows read back, records ordered);
  prove, verify        zg_prover_prove_batch_dev on the same slots (throughput form) and Verifier.verify: ms per proof.
The one condition (asserted): at batch 32 a satisfied check costs less per witness than prove + verify per proof.
--prove-verify-only measures only the last line (what a build without the check can run: point ZG_HALO2_LIB at it) and
--parent-json PATH takes the condition's prove + verify from such a run's file instead of this process's.
Writes profiles/r20/shuffle_check_time.json (or PATH).  --short: the satisfied check at batch 32 only (the run
rocprofv3 --kernel-trace --stats wraps for the per-kernel split).  Needs a GPU."""
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
import shuffle_circuits  # noqa: E402
import zg_halo2 as zg  # noqa: E402
from circuit import to_mont_array  # noqa: E402

REPS, BATCH, K = 5, 32, 14


def timed(fn, reps=REPS):
    fn()  # warm: buffers, code objects, the key's check data
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def entry(times, per):
    med = statistics.median(times)
    return {"median_ms": round(med * 1e3, 3), "ms_per_item": round(med * 1e3 / per, 4), "samples_ms": [round(t * 1e3, 3) for t in times]}


def columns(pc, variant):
    cols = pc.witness(0, [], variant)
    return np.stack([to_mont_array(cols[c]) for c in range(pc.cs.n_advice)])


def measure(ctx, pc, params, bases, vk_repr, mode):
    img = pc.cs.to_c()
    prover = zg.Prover(ctx, img, pc.fixed_values(), pc.sigma_values(), bases[0], bases[1], vk_repr, shuffles=img.shuffles)
    prover.set_overlap(False)
    prover.set_batch(BATCH)
    good, bad = columns(pc, 0), columns(pc, shuffle_circuits.BAD)
    inst = pc.instance(0)
    insts = [inst] * BATCH
    hip = zg._hip_runtime()

    def put(slot, cols):
        assert hip.hipMemcpy(prover.advice_slot(slot), cols.ctypes.data, cols.nbytes, 1) == 0

    for s in range(BATCH):
        put(s, good)
    clean = ([0, 0, 0, 0], [])
    res = {"circuit": pc.name, "k": pc.cs.k, "advice": pc.cs.n_advice, "shuffle_widths": [len(i) for i, _ in pc.cs.shuffles], "batches": {}}
    for b in ((BATCH,) if mode == "short" else (1, BATCH)):
        e = {}
        if mode != "prove-verify-only":
            def satisfied():
                assert prover.check_circuit(None, insts[:b], device=True) == [clean] * b

            e["check_satisfied"] = entry(timed(satisfied), b)
        if mode == "short":
            res["batches"][str(b)] = e
            continue
        proofs = []

        def prove():
            ps, sts = prover.prove_batch(None, insts[:b], list(range(100, 100 + b)), device=True)
            assert all(s == 0 for s in sts)
            proofs[:] = ps

        e["prove"] = entry(timed(prove), b)
        fc, sc = prover.vk_commitments()
        verifier = zg.Verifier(ctx, img, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr,
                               shuffles=img.shuffles)
        e["verify"] = entry(timed(lambda: verifier.verify(proofs, insts[:b], 7)), b)
        assert verifier.verify(proofs, insts[:b], 8) == [1] * b
        verifier.close()
        e["prove_plus_verify_ms_per_item"] = round(e["prove"]["ms_per_item"] + e["verify"]["ms_per_item"], 4)
        if mode != "prove-verify-only":
            put(0, bad)

            def one_bad():
                reports = prover.check_circuit(None, insts[:b], cap=64, device=True)
                assert reports[0][0][3] >= 1 and len(reports[0][1]) == min(64, sum(reports[0][0])) and reports[1:] == [clean] * (b - 1)
                return reports

            e["check_one_bad"] = entry(timed(one_bad), b)
            e["bad_witness_totals"] = one_bad()[0][0]
            put(0, good)
            e["check_over_prove_plus_verify"] = round(e["check_satisfied"]["ms_per_item"] / e["prove_plus_verify_ms_per_item"], 4)
        res["batches"][str(b)] = e
        print(pc.name, b, json.dumps(e), flush=True)
    prover.close()
    return res


def main():
    mode = "short" if "--short" in sys.argv else "prove-verify-only" if "--prove-verify-only" in sys.argv else "full"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r20", "shuffle_check_time.json")
    parent = sys.argv[sys.argv.index("--parent-json") + 1] if "--parent-json" in sys.argv else None
    orc.load().orc_set_threads(16)
    ctx = zg.Ctx(0)
    params = orc.params_new(K, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    bases = (ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np()))
    res = {"mode": mode, "reps": REPS, "device": torch.cuda.get_device_name(0), "library": zg.load().zg_version().decode(),
           "circuits": {}}
    for pc in (shuffle_circuits.wide(K, high_gate=True), shuffle_circuits.three(K)):
        res["circuits"][pc.name] = measure(ctx, pc, params, bases, vk_repr, mode)
    ctx.close()
    if mode == "full":
        theirs = json.load(open(parent))["circuits"] if parent else res["circuits"]
        res["condition"] = {"prove_plus_verify_from": "the build of %s" % parent if parent else "this process"}
        for name, r in res["circuits"].items():
            chk = r["batches"][str(BATCH)]["check_satisfied"]["ms_per_item"]
            pv = theirs[name]["batches"][str(BATCH)]["prove_plus_verify_ms_per_item"]
            res["condition"][name] = {"check_ms_per_witness_at_32": chk, "prove_plus_verify_ms_per_proof_at_32": pv, "holds": chk < pv}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if mode == "full":
        for name in res["circuits"]:
            assert res["condition"][name]["holds"], "%s: a satisfied check at batch 32 costs no less than prove + verify" % name


if __name__ == "__main__":
    main()
