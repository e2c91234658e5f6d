#!/usr/bin/env python3
"""What keygen on the device costs:   python tools/keygen_time.py [--out PATH] [--models tiny,large]

Per model (tiny: k = 14, the checked-in MNIST model; large: k = 17, the synthetic stand-in), ONE process, a warm-up and
three samples each, host clock around blocking calls:
  sigma_values_host    the harness's Assembly::build_pk (Python: cycles -> sigma values), ONE sample -- what the device entry replaces
  permutation_sigma    zg_permutation_sigma from the (column, row) mapping, host arrays in and out
  prover_create        zg_prover_create_shared on registered base tables: upload of fixed / sigma values + everything keygen_pk derives
  export_key_all       zg_prover_export_key of every family (fixed / sigma polys and cosets, l0, l_last, l_active_row) to the host
No condition is asserted: keygen runs once per model.  Writes profiles/r09/keygen_time.json (or PATH)."""
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

REPS = 3


def timed(fn, reps=REPS):
    fn()  # warm: workspace, twiddle tables, code objects
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def entry(times):
    return {"median_ms": round(statistics.median(times) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times]}


def one_model(ctx, label):
    if label == "tiny":
        k, name = wnn_model.MNIST_TINY
        wnn = wnn_model.load_checked_in(name)
    else:
        k, name, wnn = 17, "synthetic large", wnn_model.synthetic_wnn()
    image = wnn_model.load_test_image()
    cs, asg, ilen, _ = wnn_circuit.build(wnn, np.zeros_like(image), k)  # keygen synthesises a zero image
    img = cs.to_c()
    params = orc.params_new(k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    fixed = asg.fixed_values()
    t0 = time.perf_counter()
    sigma_host = asg.sigma_values()
    t_host = time.perf_counter() - t0
    F, P = fixed.shape[0], sigma_host.shape[0]
    next_col, next_row = zg.permutation_mapping(sigma_host, k)
    res = {"model": name, "k": k, "ext_k": cs.extended_k(), "n_fixed": F, "n_perm_columns": P,
           "sigma_values_host": entry([t_host])}
    got = {}

    def sigma_dev():
        got["sigma"] = zg.permutation_sigma(ctx, next_col, next_row, k)

    res["permutation_sigma"] = entry(timed(sigma_dev))
    assert np.array_equal(got["sigma"], sigma_host)
    bases = (ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np()))
    made = []

    def create():
        if made:
            made.pop().close()
        made.append(zg.Prover(ctx, img, fixed, got["sigma"], bases[0], bases[1], vk_repr))

    res["prover_create"] = entry(timed(create))
    prover = made[0]

    def export_all():
        size = 0
        for family, count in ((zg.KEY_FIXED_POLY, F), (zg.KEY_SIGMA_POLY, P), (zg.KEY_FIXED_COSET, F), (zg.KEY_SIGMA_COSET, P),
                              (zg.KEY_L0, 1), (zg.KEY_L_LAST, 1), (zg.KEY_L_ACTIVE_ROW, 1)):
            for c in range(count):
                size += prover.export_key(family, c).nbytes
        got["bytes"] = size

    res["export_key_all"] = entry(timed(export_all))
    res["export_key_all"]["bytes"] = got["bytes"]
    prover.close()
    for b in bases:
        b.free()
    return res


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r09", "keygen_time.json")
    models = sys.argv[sys.argv.index("--models") + 1].split(",") if "--models" in sys.argv else ["tiny", "large"]
    orc.load().orc_set_threads(16)
    ctx = zg.Ctx(0)
    res = {"reps": REPS, "device": torch.cuda.get_device_name(0), "models": {}}
    for label in models:
        res["models"][label] = one_model(ctx, label)
        print(label, json.dumps(res["models"][label]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
