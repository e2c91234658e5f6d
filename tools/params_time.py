#!/usr/bin/env python3
"""What an SRS costs on the device:   python tools/params_time.py [--out PATH] [--ks 14,17]

Per k, ONE process, a warm-up and three samples each, host clock around blocking calls:
  params_new            zg_params_new, host arrays out (the existing entry, needs the toxic scalar; here for scale)
  params_lagrange       zg_params_lagrange: g_to_lagrange from g alone, host arrays in and out
  params_lagrange_dev   zg_params_lagrange_dev + zg_ctx_sync: device arrays in and out (the transform itself)
  params_check          zg_params_check with g_lagrange (points, powers relation, Lagrange relation)
  params_check_g_only   zg_params_check with g_lagrange = NULL (points, powers relation)
The transform's output is compared with zg_params_new's g_lagrange and the check must accept; no speed condition is
asserted: each runs once per SRS.  Writes profiles/r10/params_time.json (or PATH)."""
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

REPS = 3


def timed(fn, reps=REPS):
    fn()  # warm: workspace, code objects
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def entry(times):
    return {"median_ms": round(statistics.median(times) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times]}


def one_k(ctx, k):
    n = 1 << k
    s = orc.fill_fr(0x5EED, 1)[0]
    small = orc.params_new(1, 0x5EED)  # g2 / s_g2 do not depend on k
    g2, s_g2 = np.array(small.g2, np.uint64), np.array(small.s_g2, np.uint64)
    got = {}
    res = {"k": k}

    def new():
        got["g"], got["gl"] = ctx.params_new(k, s)

    res["params_new"] = entry(timed(new))
    g, gl = got["g"], got["gl"]

    def lagrange():
        got["lag"] = ctx.params_lagrange(k, g)

    res["params_lagrange"] = entry(timed(lagrange))
    assert np.array_equal(got["lag"], gl)
    d_g = torch.from_numpy(g.view(np.int64).reshape(-1).copy()).cuda()
    d_gl = torch.zeros(n * 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def lagrange_dev():
        ctx.params_lagrange_dev(k, d_g.data_ptr(), d_gl.data_ptr())
        ctx.sync()

    res["params_lagrange_dev"] = entry(timed(lagrange_dev))
    assert np.array_equal(d_gl.cpu().numpy().view(np.uint64).reshape(n, 8), gl)

    def check(with_lagrange):
        got["verdict"] = ctx.params_check(k, g, gl if with_lagrange else None, g2, s_g2, os.urandom(32))

    res["params_check"] = entry(timed(lambda: check(True)))
    assert got["verdict"] == (1, 0)
    res["params_check_g_only"] = entry(timed(lambda: check(False)))
    assert got["verdict"] == (1, 0)
    return res


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r10", "params_time.json")
    ks = [int(x) for x in sys.argv[sys.argv.index("--ks") + 1].split(",")] if "--ks" in sys.argv else [14, 17]
    ctx = zg.Ctx(0)
    res = {"reps": REPS, "device": torch.cuda.get_device_name(0), "k": {}}
    try:
        res["sclk_mhz"] = torch.cuda.clock_rate()  # the shader clock while idle, where the runtime reports it
    except Exception:  # noqa: BLE001 -- not every build reports it
        pass
    for k in ks:
        res["k"][str(k)] = one_k(ctx, k)
        print(k, json.dumps(res["k"][str(k)]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
