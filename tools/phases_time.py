#!/usr/bin/env python3
"""What a second advice phase costs:   python tools/phases_time.py [--out PATH] [--bench-line FILE]

The `rlc` circuit of tests/phases_circuits.py at k = 14 with its degree-6 gate (one challenge, the accumulator column in
phase 1), against the SAME circuit with the challenge replaced by a fixed constant and every column in one phase -- built
here and proved by the same library through the same entry (zg_prover_prove_phased): the path the library had before
phases.  ONE process, both provers on the same base tables.  The witnesses are made once (a first run learns each proof's
challenge, which the keys fix) and kept in device buffers; the timed callbacks only copy them into the slots, device to
device, so the figures are the library's: one more MSM launch sequence, one more host round trip, the fill.
Per item a warm-up, then medians of three ALTERNATING rounds; host clock around the blocking calls.
  a lone proof, latency form                 ms
  a batch of 32, throughput form             ms per proof
  challenge_fill                             ms per launch, from the library's profile (a run of its own)
  resident bytes per slot per challenge      by hipMemGetInfo around zg_prover_set_batch, and by formula
--bench-line FILE: a file holding bench.py's JSON line of the same tree and box, recorded beside README's headline.
No bar is set.  Writes profiles/r18/phases_time.json (or PATH).  Needs a GPU."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("0g-halo2_amd", "oracle", "harness", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import torch  # noqa: E402  (before the library: one HIP runtime in the process)

import numpy as np  # noqa: E402
import orc  # noqa: E402
import phases_circuits  # noqa: E402
import zg_halo2 as zg  # noqa: E402
from circuit import to_mont_array  # noqa: E402

REPS, BATCH, K = 3, 32, 14
CONSTANT = 0x1234567
README_HEADLINE_MS, README_SPREAD_MS = 0.669, (0.66, 0.69)


def entry(times, per):
    med = statistics.median(times)
    return {"ms_per_proof": round(med * 1e3 / per, 4), "median_ms": round(med * 1e3, 3), "min_ms": round(min(times) * 1e3, 3),
            "max_ms": round(max(times) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times]}


class Side:
    """one of the two circuits: its prover and, per proof and phase, the witness columns in device memory"""

    def __init__(self, ctx, pc, bases, params, vk_repr):
        self.pc = pc
        self.prover = zg.Prover(ctx, pc.cs.to_c(), pc.fixed_values(), pc.sigma_values(), bases[0], bases[1], vk_repr)
        self.prover.set_phases(pc.advice_phase, pc.challenge_phase)
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.dev = {}  # (proof, phase) -> {column: device tensor of the usable rows}
        self.inst = [pc.instance(b) for b in range(BATCH)]

    def learn(self, count):
        """a first, untimed run with the witness made on the host: leaves every (proof, phase)'s columns on the device"""
        usable = self.pc.usable

        def synth(phase, ch):
            out = []
            for b in range(ch.shape[0]):
                cols = self.pc.witness(phase, [orc.fr_to_int(ch[b, j]) for j in range(ch.shape[1])], b)
                arrs = {c: to_mont_array(v[:usable]) for c, v in cols.items()}
                self.dev[b, phase] = {c: torch.from_numpy(a.view(np.int64).reshape(-1)).cuda() for c, a in arrs.items()}
                out.append(arrs)
            return out

        proofs, st = self.prover.prove_phased(synth, self.inst[:count], list(range(1, count + 1)))
        assert st == 0
        torch.cuda.synchronize()
        return proofs

    def callback(self):
        n, usable = self.pc.n, self.pc.usable

        def cb(_user, phase, cnt, _challenges, d_advice):
            for b in range(cnt):
                for c, t in self.dev[b, phase].items():
                    if self.hip.hipMemcpy(ctypes.c_void_p(d_advice[b] + c * n * 32), ctypes.c_void_p(t.data_ptr()),
                                          ctypes.c_size_t(usable * 32), 3) != 0:
                        return 1
            return 0

        return zg.PHASE_FN(cb)

    def prove(self, count, fn):
        proofs, st = self.prover.prove_phased_c(fn, self.inst[:count], list(range(1, count + 1)))
        assert st == 0
        return proofs


def alternate(sides, count):
    fns = {name: s.callback() for name, s in sides.items()}
    want = {name: s.learn(count) for name, s in sides.items()}
    for name, s in sides.items():
        assert s.prove(count, fns[name]) == want[name], name  # (warm-up; the cached witness is the proof's)
    times = {name: [] for name in sides}
    for _ in range(REPS):
        for name, s in sides.items():
            t0 = time.perf_counter()
            s.prove(count, fns[name])
            times[name].append(time.perf_counter() - t0)
    out = {name: entry(t, count) for name, t in times.items()}
    out["two_phase_over_one_phase"] = round(out["two_phase"]["median_ms"] / out["one_phase"]["median_ms"], 4)
    out["extra_ms_per_proof"] = round(out["two_phase"]["ms_per_proof"] - out["one_phase"]["ms_per_proof"], 4)
    return out


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r18", "phases_time.json")
    orc.load().orc_set_threads(16)
    ctx = zg.Ctx(0)
    params = orc.params_new(K, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    bases = (ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np()))
    sides = {"two_phase": Side(ctx, phases_circuits.rlc(K, high_gate=True), bases, params, vk_repr),
             "one_phase": Side(ctx, phases_circuits.rlc(K, high_gate=True, constant=CONSTANT), bases, params, vk_repr)}
    pc = sides["two_phase"].pc
    res = {"circuit": "rlc, k = 14, cs_degree %d: %d advice, %d fixed, %d gates, 2 equality columns; 1 challenge, accumulator in phase 1"
                      % (pc.cs.degree(), pc.cs.n_advice, pc.cs.n_fixed, len(pc.cs.gates)),
           "baseline": "the same circuit, the challenge replaced by the constant 0x%x, every column in phase 0" % CONSTANT,
           "device": torch.cuda.get_device_name(0), "reps": REPS}
    try:
        res["sclk_mhz"] = torch.cuda.clock_rate()  # the shader clock while idle, where the runtime reports it
    except Exception:  # noqa: BLE001 -- not every build reports it
        pass
    res["lone_latency_form"] = alternate(sides, 1)
    # resident bytes: what growing each prover from 1 to BATCH slots takes, per slot
    free = {}
    for name, s in sides.items():
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        s.prover.set_batch(BATCH)
        s.prover.set_overlap(False)
        free[name] = (before - torch.cuda.mem_get_info()[0]) / (BATCH - 1)
    n = pc.n
    res["resident_bytes_per_slot_per_challenge"] = {
        "measured": round(free["two_phase"] - free["one_phase"]),
        "formula": "(n + n + 8n + 4n + n) * 32: value row, coefficient row, one slab on the single coset and on each split part",
        "formula_bytes": (2 * n + (1 << pc.cs.extended_k()) + 4 * n + n) * 32,
        "slot_bytes": {name: round(v) for name, v in free.items()}}
    res["batch_32_throughput_form"] = alternate(sides, BATCH)
    # the fill kernel by the library's own events, in a run of its own
    ctx.profile(True)
    ctx.profile_collect()
    fn = sides["two_phase"].callback()
    sides["two_phase"].prove(BATCH, fn)
    prof = ctx.profile_collect()
    ctx.profile(False)
    launches, total_ms = prof["challenge_fill"][0], prof["challenge_fill"][1]
    res["challenge_fill"] = {"launches": launches, "ms_per_launch": round(total_ms / launches, 4), "proofs_per_launch": BATCH,
                             "bytes_per_launch": prof["challenge_fill"][2]}
    if "--bench-line" in sys.argv:
        line = json.loads(open(sys.argv[sys.argv.index("--bench-line") + 1]).read().strip().splitlines()[-1])
        res["bench_sanity"] = {"ms_per_proof": line.get("ms_per_proof"), "steps": line.get("steps"), "warmup": line.get("warmup"),
                               "readme_headline_ms": README_HEADLINE_MS, "readme_box_to_box_ms": list(README_SPREAD_MS),
                               "within_spread": README_SPREAD_MS[0] <= line.get("ms_per_proof", 0) <= README_SPREAD_MS[1],
                               "note": "the bench circuit has no challenge: a sanity line, not a criterion"}
    for s in sides.values():
        s.prover.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
