#!/usr/bin/env python3
"""What an SRS contribution costs on the device:   python tools/params_update_time.py [--out PATH] [--ks 14,17]

Per k, ONE process, a warm-up and three samples each (tools/params_time.py's scheme), host clock around blocking calls:
  g1_mul_each_dev          zg_g1_mul_each_dev + zg_ctx_sync on 2^k points with full-size scalars; also per point
  srs_kernel               zg_params_new_dev + zg_ctx_sync: the existing kernel, two binary ladders per lane (g and
                           g_lagrange) -- its time / 2^(k+1) is the bar per multiplication
  params_update_dev        zg_params_update_dev + zg_ctx_sync, g only (powers on the device, the multiplications)
  params_update_dev_lagrange   ... with the Lagrange leg (the G1 transform of zg_params_lagrange_dev)
  params_check_update      zg_params_check_update with g_lagrange (zg_params_check + two host pairing products)
The update is compared with zg_params_new of the product scalar and the check must accept.  `meets_bar` says whether the
new kernel takes no more time per multiplication than srs_kernel; nothing is asserted about it.
Writes profiles/r15/params_update_time.json (or PATH)."""
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


def entry(times, per=None):
    e = {"median_ms": round(statistics.median(times) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times]}
    if per:
        e["ns_per_multiplication"] = round(statistics.median(times) * 1e9 / per, 1)
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def one_k(ctx, k):
    n = 1 << k
    s, t = orc.fill_fr(0x5EED, 1)[0], orc.fill_fr(0x7EA, 1)[0]
    st = zg.fr_from_int(zg.fr_to_int(s) * zg.fr_to_int(t))
    g2, s_g2 = zg.params_g2(s)
    res = {"k": k}
    d_g = torch.zeros(n * 8, dtype=torch.int64, device="cuda")
    d_gl = torch.zeros(n * 8, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(n * 8, dtype=torch.int64, device="cuda")
    d_out_l = torch.zeros(n * 8, dtype=torch.int64, device="cuda")
    d_sc = dev(orc.fill_fr(0xABC, n))
    torch.cuda.synchronize()

    def srs():
        ctx.params_new_dev(k, s, d_g.data_ptr(), d_gl.data_ptr())
        ctx.sync()

    res["srs_kernel"] = entry(timed(srs), 2 * n)

    def mul_each():
        ctx.g1_mul_each_dev(d_g.data_ptr(), d_sc.data_ptr(), n, d_out.data_ptr())
        ctx.sync()

    res["g1_mul_each_dev"] = entry(timed(mul_each), n)

    def update(lagrange):
        ctx.params_update_dev(k, t, d_g.data_ptr(), d_out.data_ptr(), d_out_l.data_ptr() if lagrange else 0)
        ctx.sync()

    res["params_update_dev"] = entry(timed(lambda: update(False)))
    res["params_update_dev_lagrange"] = entry(timed(lambda: update(True)))
    want_g, want_gl = ctx.params_new(k, st)
    g_next = d_out.cpu().numpy().view(np.uint64).reshape(n, 8)
    gl_next = d_out_l.cpu().numpy().view(np.uint64).reshape(n, 8)
    assert np.array_equal(g_next, want_g) and np.array_equal(gl_next, want_gl)
    prev = d_g.cpu().numpy().view(np.uint64).reshape(n, 8)[:2].copy()
    # the record and s_g2 of the step, through the host entry at a small k (they do not depend on k)
    _, _, s_g2_next, record = ctx.params_update(1, t, prev, g2, s_g2, lagrange=False)
    got = {}

    def check():
        got["verdict"] = ctx.params_check_update(k, prev, g_next, gl_next, g2, s_g2_next, record, os.urandom(32))

    res["params_check_update"] = entry(timed(check))
    assert got["verdict"] == (1, 0)
    res["meets_bar"] = res["g1_mul_each_dev"]["ns_per_multiplication"] <= res["srs_kernel"]["ns_per_multiplication"]
    return res


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r15", "params_update_time.json")
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
