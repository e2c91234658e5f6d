#!/usr/bin/env python3
"""What the native shuffle argument costs against the hand-built one:   python tools/shuffle_time.py [--out PATH]

The `shuffle` circuit of tests/phases_circuits.py at k = 14 -- the statement "b is a permutation of a" built by hand from a
challenge and a second-phase product column z, proved through zg_prover_prove_phased -- against the SAME statement as one
native shuffle argument (zg_prover_create_shuffles: columns a and b, no gate, no challenge, one phase), proved through
zg_prover_prove_batch.  ONE process, both provers on the same base tables.  The hand-built side's witnesses are made once
(a first run learns each proof's challenge) and kept in device buffers, the timed callbacks only copy them into the slots;
the native side's columns are put into its slots once and stay there.  Per item a warm-up, then medians of three
ALTERNATING rounds; host clock around the blocking calls.
  a lone proof, latency form                 ms
  a batch of 32, throughput form             ms per proof
  shuffle_terms, shuffle_h                   ms per launch, from the library's profile (a run of its own)
No bar is set.  Writes profiles/r19/shuffle_time.json (or PATH).  Needs a GPU."""
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
import shuffle_circuits  # noqa: E402
import zg_halo2 as zg  # noqa: E402
from circuit import to_mont_array  # noqa: E402
from phases_time import Side, entry  # noqa: E402

REPS, BATCH, K = 3, 32, 14


class Native:
    """the statement as one shuffle argument; the witness of proof b is the hand-built circuit's phase-0 columns"""

    def __init__(self, ctx, hand, bases, vk_repr):
        cs = shuffle_circuits.ShuffleCS(K)
        a, b = cs.advice_column(), cs.advice_column()
        cs.shuffle([cs.advice(a)], [cs.advice(b)])
        self.cs, self.hand = cs, hand
        img = cs.to_c()
        empty = np.zeros((0, 1 << K, 4), np.uint64)
        self.prover = zg.Prover(ctx, img, empty, empty, bases[0], bases[1], vk_repr, shuffles=img.shuffles)
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.inst = [np.zeros((0, 0, 4), np.uint64)] * BATCH

    def fill(self, count):
        for s in range(count):
            cols = self.hand.witness(0, [], s)
            arr = np.stack([to_mont_array(cols[c]) for c in (0, 1)])
            assert self.hip.hipMemcpy(ctypes.c_void_p(self.prover.advice_slot(s)), ctypes.c_void_p(arr.ctypes.data),
                                      ctypes.c_size_t(arr.nbytes), 1) == 0

    def prove(self, count):
        proofs, st = self.prover.prove_batch(None, self.inst[:count], list(range(1, count + 1)), device=True)
        assert all(s == 0 for s in st)
        return proofs


def alternate(hand, native, count):
    fn = hand.callback()
    want = hand.learn(count)
    assert hand.prove(count, fn) == want
    native.fill(count)
    first = native.prove(count)
    assert native.prove(count) == first
    times = {"hand_built": [], "native": []}
    for _ in range(REPS):
        t0 = time.perf_counter()
        hand.prove(count, fn)
        times["hand_built"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        native.prove(count)
        times["native"].append(time.perf_counter() - t0)
    out = {name: entry(t, count) for name, t in times.items()}
    out["native_over_hand_built"] = round(out["native"]["median_ms"] / out["hand_built"]["median_ms"], 4)
    out["proof_bytes"] = {"hand_built": len(want[0]), "native": len(first[0])}
    return out


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r19", "shuffle_time.json")
    orc.load().orc_set_threads(16)
    ctx = zg.Ctx(0)
    params = orc.params_new(K, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    bases = (ctx.register_bases(params.g_np()), ctx.register_bases(params.g_lagrange_np()))
    hand = Side(ctx, phases_circuits.shuffle(K), bases, params, vk_repr)
    native = Native(ctx, hand.pc, bases, vk_repr)
    res = {"statement": "b is a permutation of a over the usable rows, k = %d" % K,
           "hand_built": "tests/phases_circuits.py shuffle: 3 advice (z in phase 1), 3 fixed, 3 gates of degree <= 3, 1 challenge; zg_prover_prove_phased",
           "native": "2 advice, one zg_shuffle of width 1, cs_degree 3; zg_prover_prove_batch on columns resident in the slots",
           "device": torch.cuda.get_device_name(0), "reps": REPS}
    res["lone_latency_form"] = alternate(hand, native, 1)
    for side in (hand, native):
        side.prover.set_batch(BATCH)
        side.prover.set_overlap(False)
    res["batch_32_throughput_form"] = alternate(hand, native, BATCH)
    ctx.profile(True)
    ctx.profile_collect()
    native.prove(BATCH)
    prof = ctx.profile_collect()
    ctx.profile(False)
    res["kernels"] = {name: {"launches": prof[name][0], "ms_per_launch": round(prof[name][1] / prof[name][0], 4), "proofs_per_launch": BATCH}
                      for name in ("shuffle_terms", "shuffle_h")}
    for side in (hand, native):
        side.prover.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
