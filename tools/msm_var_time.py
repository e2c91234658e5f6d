#!/usr/bin/env python3
"""What multiplying UNREGISTERED points costs:   python tools/msm_var_time.py [--out PATH] [--ks 14,17] [--reps 7]

Per shape (n = 2^k, batch 1 and 3, uniform scalars), ONE process, a warm-up of each route at that shape, then the two routes
ALTERNATING, `reps` samples each, host clock around calls that end synchronised (both return normalised points):
  msm_var              zg_msm_var_batch on the host arrays
  register_msm_free    zg_bases_register + zg_msm_batch + zg_bases_free on the same host arrays -- the only route for
                       unregistered points without zg_msm_var
and for context
  msm_registered       zg_msm_batch on a set registered beforehand: the cost once tables exist
  kernels_ms           per-kernel device time of ONE profiled zg_msm_var_batch (zg_ctx_profile_*), msm_var_horner among them
Both routes must give the same bytes; no speed condition is asserted.  Writes profiles/r13/msm_var_time.json (or PATH)."""
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
import zg_halo2 as zg  # noqa: E402


def entry(times):
    return {"median_ms": round(statistics.median(times) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times]}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def one_shape(ctx, g, k, batch, reps):
    n = 1 << k
    s = np.stack([orc.fill_fr(1300 + 10 * k + b, n) for b in range(batch)])
    got = {}

    def var():
        got["var"] = ctx.msm_var_batch(g, s)

    def reg():
        bases = ctx.register_bases(g)
        got["reg"] = ctx.msm_batch(bases, s)
        bases.free()

    var()
    reg()  # warm: workspace blocks, code objects
    assert np.array_equal(got["var"], got["reg"]), "the two routes disagree"
    t_var, t_reg = [], []
    for _ in range(reps):
        t_var.append(clock(var))
        t_reg.append(clock(reg))
    bases = ctx.register_bases(g)

    def fixed():
        got["fixed"] = ctx.msm_batch(bases, s)

    fixed()
    t_fixed = [clock(fixed) for _ in range(reps)]
    assert np.array_equal(got["fixed"], got["var"])
    bases.free()
    ctx.profile(True)
    try:
        ctx.profile_collect()
        var()
        stats = ctx.profile_collect()
    finally:
        ctx.profile(False)
    kernels = {name: round(v[1], 4) for name, v in sorted(stats.items()) if name.startswith("msm_var_")}
    res = {"k": k, "batch": batch, "window_bits": "library's choice", "msm_var": entry(t_var), "register_msm_free": entry(t_reg),
           "msm_registered": entry(t_fixed), "kernels_ms": kernels, "kernels_sum_ms": round(sum(kernels.values()), 4)}
    spread = max(max(t_var) - min(t_var), max(t_reg) - min(t_reg))
    res["spread_ms"] = round(spread * 1e3, 3)
    res["register_msm_free_over_msm_var"] = round(statistics.median(t_reg) / statistics.median(t_var), 3)
    return res


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r13", "msm_var_time.json")
    ks = [int(x) for x in sys.argv[sys.argv.index("--ks") + 1].split(",")] if "--ks" in sys.argv else [14, 17]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    ctx = zg.Ctx(0)
    res = {"reps": reps, "device": torch.cuda.get_device_name(0), "shapes": []}
    try:
        res["sclk_mhz"] = torch.cuda.clock_rate()  # the shader clock while idle, where the runtime reports it
    except Exception:  # noqa: BLE001 -- not every build reports it
        pass
    for k in ks:
        g, _ = ctx.params_new(k, orc.fill_fr(0x5EED, 1)[0])
        for batch in (1, 3):
            r = one_shape(ctx, g, k, batch, reps)
            res["shapes"].append(r)
            print(json.dumps(r), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
