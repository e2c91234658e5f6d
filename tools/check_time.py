#!/usr/bin/env python3
"""Time the witness check against what a caller pays today for the same yes / no:   python tools/check_time.py [--out PATH] [--short]

Tiny model, k = 14, ONE process, warm-up and five samples each (host clock around blocking calls):
  check_images   ms per witness at batch 1, 32 and on 12 forked provers x 32 (threads, one context each);
  report path    the same batches with one witness that fails on every row (records read back and ordered);
  beside them    prove_images ms per proof and Verifier.verify ms per proof at the same batches.
The one condition (asserted): at batch 32 a satisfied check costs less per witness than prove_images + verify per proof.
Writes profiles/r07/check_time.json (or PATH).  --short: batch 32 of check_images only (the run rocprofv3 --kernel-trace
--stats wraps for the per-kernel split)."""
import json
import os
import statistics
import sys
import threading
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


def together(fns):
    """run the callables on one thread each, all released at once; returns when the last is done"""
    go = threading.Barrier(len(fns) + 1)
    errs = []

    def work(f):
        go.wait()
        try:
            f()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(f,)) for f in fns]
    for t in ts:
        t.start()
    go.wait()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]


def main():
    short = "--short" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r07", "check_time.json")
    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    wnn = wnn_model.load_checked_in(name)
    real = wnn_model.load_test_image()
    cs, asg, ilen, scores = wnn_circuit.build(wnn, real, k)
    img = cs.to_c()
    params = orc.params_new(k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    ctx = zg.Ctx(0)
    bases = (ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np()))
    prover = zg.Prover(ctx, img, fixed, sigma, bases[0], bases[1], vk_repr)
    prover.set_overlap(False)
    prover.set_batch(32)
    arrays = witness_tape.trace(wnn, k).arrays()
    plan = zg.WitnessPlan(ctx, arrays)
    rng = np.random.default_rng(5)
    images = np.stack([real] + [rng.integers(0, 256, size=real.shape, dtype=real.dtype) for _ in range(31)])
    res = {"model": name, "k": k, "reps": REPS, "device": torch.cuda.get_device_name(0), "batches": {}}

    def check_images(p, pl, b):
        reports, _ = p.check_images(pl, images[:b])
        assert all(r == ([0, 0, 0], []) for r in reports)

    if short:
        res["batches"]["32"] = {"check_images": entry(timed(lambda: check_images(prover, plan, 32)), 32)}
        print(json.dumps(res))
        return

    fc, sc = prover.vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr)
    # a witness that fails on every row: every advice cell 2^20 + row + column, resident on the device
    n = 1 << k
    bad = np.stack([zg_fr_column(n, c) for c in range(cs.n_advice)])
    d_bad = torch.from_numpy(bad.view(np.int64)).cuda()

    for b in (1, 32):
        e = {}
        e["check_images"] = entry(timed(lambda: check_images(prover, plan, b)), b)
        _, outputs = prover.check_images(plan, images[:b])
        insts = [o[None, :, :] for o in outputs]
        e["check_only_slots_as_they_stand"] = entry(timed(lambda: prover.check_batch(None, insts, device=True)), b)

        def failing():
            reports = prover.check_batch([d_bad.data_ptr()] + [None] * (b - 1), insts, cap=64, device=True)
            assert sum(reports[0][0]) > n and len(reports[0][1]) == 64 and all(r == ([0, 0, 0], []) for r in reports[1:])
            return reports

        e["check_one_witness_failing_everywhere"] = entry(timed(failing), b)
        e["failing_witness_totals"] = failing()[0][0]
        proofs = []

        def prove():
            ps, outs, sts = prover.prove_images(plan, images[:b], list(range(100, 100 + b)))
            assert sts == [0] * b
            proofs[:] = ps

        e["prove_images"] = entry(timed(prove), b)
        e["verify"] = entry(timed(lambda: verifier.verify(proofs, insts, 7)), b)
        assert verifier.verify(proofs, insts, 8) == [1] * b
        e["prove_plus_verify_ms_per_item"] = round(e["prove_images"]["ms_per_item"] + e["verify"]["ms_per_item"], 4)
        e["check_over_prove_plus_verify"] = round(e["check_images"]["ms_per_item"] / e["prove_plus_verify_ms_per_item"], 4)
        res["batches"][str(b)] = e
        print(b, json.dumps(e), flush=True)

    # twelve forked provers x 32, one context and one plan each (the bench's shape)
    ctxs = [zg.Ctx(0) for _ in range(12)]
    forks = [prover.fork(c) for c in ctxs]
    plans = [zg.WitnessPlan(c, arrays) for c in ctxs]
    for f in forks:
        f.set_overlap(False)
        f.set_batch(32)
    e = {}
    e["check_images"] = entry(timed(lambda: together([lambda f=f, pl=pl: check_images(f, pl, 32) for f, pl in zip(forks, plans)])), 384)
    all_proofs = [None] * 12

    def prove_on(i):
        ps, outs, sts = forks[i].prove_images(plans[i], images, list(range(1000 + 32 * i, 1032 + 32 * i)))
        assert sts == [0] * 32
        all_proofs[i] = (ps, [o[None, :, :] for o in outs])

    e["prove_images"] = entry(timed(lambda: together([lambda i=i: prove_on(i) for i in range(12)])), 384)
    flat = [p for ps, _ in all_proofs for p in ps]
    flat_inst = [o for _, os_ in all_proofs for o in os_]
    e["verify"] = entry(timed(lambda: verifier.verify(flat, flat_inst, 9)), 384)
    e["prove_plus_verify_ms_per_item"] = round(e["prove_images"]["ms_per_item"] + e["verify"]["ms_per_item"], 4)
    e["check_over_prove_plus_verify"] = round(e["check_images"]["ms_per_item"] / e["prove_plus_verify_ms_per_item"], 4)
    res["batches"]["12x32"] = e
    print("12x32", json.dumps(e), flush=True)

    b32 = res["batches"]["32"]
    res["condition"] = {"check_ms_per_witness_at_32": b32["check_images"]["ms_per_item"],
                        "prove_plus_verify_ms_per_proof_at_32": b32["prove_plus_verify_ms_per_item"],
                        "holds": b32["check_images"]["ms_per_item"] < b32["prove_plus_verify_ms_per_item"]}
    for p in plans:
        p.close()
    for f in forks:
        f.close()
    for c in ctxs:
        c.close()
    plan.close()
    verifier.close()
    prover.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    assert res["condition"]["holds"], "a satisfied check at batch 32 costs no less than prove_images + verify"


def zg_fr_column(n, c):
    from circuit import to_mont_array

    return to_mont_array([(1 << 20) + r + c for r in range(n)])


if __name__ == "__main__":
    main()
