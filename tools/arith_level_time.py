#!/usr/bin/env python3
"""What incremental adoption costs:   python tools/arith_level_time.py [--out PATH]

The arithmetic level on device pointers for the tiny model (k = 14, one image), ONE process,
one warm-up and then five samples of each item, the items alternating; host clock around calls that end in a synchronise:
  caller_run_proof     tests/arith_level.py's create_proof over its device backend: halo2's schedule walked by the CALLER
                       (a Python caller: transcript, challenges and query lists as Python integers) over the *_dev entries
  prove_dev            zg_prover_prove_dev of the same advice columns (the prover level), for scale
  evaluate_h / _dev    zg_prover_evaluate_h (host pointers, ~60 MiB over PCIe) against zg_prover_evaluate_h_dev + a synchronise
  permute / _dev       zg_permute_expression_pair (host pointers) against zg_permute_expression_pair_dev on one 2^14-row pair
This is the incremental-adoption path: nothing here enters bench.py's result line, and no threshold is set -- the parent of
this path has no such walk to compare with.  Writes profiles/r14/arith_level_time.json (or PATH)."""
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
import wnn_circuit  # noqa: E402
import wnn_model  # noqa: E402
import zg_halo2 as zg  # noqa: E402

import arith_level  # noqa: E402
import lookup_cases  # noqa: E402
import poly_ref as pr  # noqa: E402

REPS = 5


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r14", "arith_level_time.json")
    orc.load().orc_set_threads(min(16, os.cpu_count() or 1))
    k, name = wnn_model.MNIST_TINY
    cs, asg, ilen, _ = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), k)
    n, en = 1 << k, 1 << cs.extended_k()
    img = cs.to_c()
    params = orc.params_new(k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    seed = 7
    ctx = zg.Ctx(0)
    g, gl = ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np())
    prover = zg.Prover(ctx, img, fixed, sigma, g, gl, vk_repr)
    be = arith_level.DeviceBackend(zg, ctx, prover, cs, fixed, sigma, g, gl, seed)
    d_adv = dev(adv)
    got = {}

    def caller_run():
        got["caller"] = arith_level.create_proof(be, cs, vk_repr, adv, inst)
        ctx.sync()

    def prove_dev():
        got["prover"] = prover.prove_dev(d_adv.data_ptr(), inst, seed)

    # evaluate_h: random coefficient forms (the cost does not depend on the values)
    nl, sets = len(cs.lookups), arith_level.n_sets(cs)
    fams = [orc.fill_fr(100 + i, c * n).reshape(c, n, 4) for i, c in enumerate((cs.n_advice, cs.n_instance, sets, nl, 2 * nl))]
    ch = [orc.fill_fr(200, 4)[i] for i in range(4)]
    d_fams, d_h = [dev(f) for f in fams], dev(np.zeros((en, 4), np.uint64))

    def evalh_host():
        got["h_host"] = prover.evaluate_h(*fams, *ch, en)

    def evalh_dev():
        prover.evaluate_h_dev(*[t.data_ptr() if t.shape[0] else 0 for t in d_fams], *ch, d_h.data_ptr())
        ctx.sync()

    table, inputs = lookup_cases.make("runs", k)
    usable = lookup_cases.usable_rows(k)
    a_in, a_tab = pr.from_ints(inputs + [0] * (n - usable)), pr.from_ints(table + [0] * (n - usable))
    d_in, d_tab, d_a, d_s = dev(a_in), dev(a_tab), dev(np.zeros((n, 4), np.uint64)), dev(np.zeros((n, 4), np.uint64))

    def permute_host():
        got["perm_host"] = ctx.permute_expression_pair(a_in, a_tab, usable)

    def permute_dev():
        ctx.permute_expression_pair_dev(d_in.data_ptr(), d_tab.data_ptr(), k, usable, d_a.data_ptr(), d_s.data_ptr())
        ctx.sync()

    items = [("caller_run_proof", caller_run), ("prove_dev", prove_dev), ("evaluate_h", evalh_host), ("evaluate_h_dev", evalh_dev),
             ("permute_expression_pair", permute_host), ("permute_expression_pair_dev", permute_dev)]
    times = {label: [] for label, _ in items}
    for rep in range(REPS + 1):  # the first round warms: workspace, twiddle tables, code objects
        for label, fn in items:
            t0 = time.perf_counter()
            fn()
            if rep:
                times[label].append(time.perf_counter() - t0)
    assert got["caller"] == got["prover"], "the caller-run proof and the prover level's differ"
    assert np.array_equal(got["h_host"], d_h.cpu().numpy().view(np.uint64))
    assert np.array_equal(got["perm_host"][0], d_a.cpu().numpy().view(np.uint64))
    res = {"purpose": "incremental adoption (INTEGRATION.md 3(a)); not part of the bench line", "model": name, "k": k,
           "ext_k": cs.extended_k(), "reps": REPS, "device": torch.cuda.get_device_name(0), "proof_bytes": len(got["caller"]),
           "items": {label: {"median_ms": round(statistics.median(t) * 1e3, 3), "min_ms": round(min(t) * 1e3, 3),
                             "max_ms": round(max(t) * 1e3, 3), "samples_ms": [round(x * 1e3, 3) for x in t]}
                     for label, t in times.items()}}
    prover.close()
    g.free()
    gl.free()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
