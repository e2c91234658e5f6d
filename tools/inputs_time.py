#!/usr/bin/env python3
"""Time input -> proof through the witness program with field operations (zg_prover_prove_inputs):
    python tools/inputs_time.py [--out PATH] [--guard PARENT.so [THIS.so]]

tests/phases_circuits.py rlc and shuffle at k = 5 (two phases, one challenge; shuffle's phase 1 is a chain of products and
inversions), one prover each, ONE process, one warm-up per shape and five samples (host clock around the blocking calls),
alternating, for batches of 1, 4 and 16 inputs:
  prove_inputs                        the recorded program of tests/field_tape.py on the device, every phase
  prove_phased, Python callback       Phased.synthesize: the host pass the entry replaces, Python integers and all
  prove_phased, kept columns          the same callback with every (phase, variant, challenges) witness made once before the
                                      timed calls: the copies into the slots and no Python arithmetic (tools/circuits_time.py)
and per-launch HIP-event times of witness_run_field / witness_finish_phase from the profile of the prove_inputs calls.
The bytes of the three are compared before anything is timed.  No bar is set: facts with the spread of their samples.

--guard: the regression guard of the integer-only path.  tools/witness_time.py tiny (witness_run + witness_finish per
launch, lone and in a batch of 16) in fresh child processes, alternating the parent's build and this one (ZG_HALO2_LIB),
three rounds; the bar is the parent's own spread between its rounds.

Writes profiles/r24/inputs_time.json (or PATH).  Needs a GPU: without one the context's creation raises."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("0g-halo2_amd", "oracle", "harness", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

REPS = 5
SIZES = (1, 4, 16)
NVAR = 3


def entry(times, per):
    med = statistics.median(times)
    return {"ms_per_input": round(med * 1e3 / per, 4), "median_ms": round(med * 1e3, 3), "min_ms": round(min(times) * 1e3, 3),
            "max_ms": round(max(times) * 1e3, 3), "samples_ms": [round(t * 1e3, 3) for t in times]}


def guard(parent, this):
    rows = {"parent": [], "this": []}
    for _ in range(3):
        for which, lib in (("parent", parent), ("this", this)):
            env = dict(os.environ, ZG_HALO2_LIB=os.path.abspath(lib))
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "witness_time.py"), "tiny"], env=env, capture_output=True, text=True,
                               timeout=240, check=True)
            rows[which].append([json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")])
    keys = ("witness_run_us_1", "witness_finish_us_1", "witness_run_us_16", "witness_finish_us_16")
    out = {"tool": "tools/witness_time.py tiny", "rounds": 3, "forms": {}}
    for f, form in enumerate(("ZG_WITNESS_LDS=0", "ZG_WITNESS_LDS default")):
        e = {}
        for key in keys:
            a = [r[f][key] for r in rows["parent"]]
            b = [r[f][key] for r in rows["this"]]
            e[key] = {"parent": a, "this": b, "inside_parent_spread": min(a) <= statistics.median(b) <= max(a)}
        out["forms"][form] = e
    return out


def measure(zg, orc, ctx, name, res):
    import field_tape
    import numpy as np
    from circuit import to_mont_array

    rec = field_tape.recorded(name)
    pc, prog = rec.pc, rec.program
    img = pc.cs.to_c()
    params = orc.params_new(pc.cs.k, 0x5EED)
    prover = zg.Prover(ctx, img, pc.fixed_values(), pc.sigma_values(), params.g_np(), params.g_lagrange_np(), orc.fr_from_int(0xC0FFEE))
    prover.set_phases(pc.advice_phase, pc.challenge_phase)
    prover.set_overlap(False)
    prover.set_batch(max(SIZES))
    plan = zg.WitnessPlan(ctx, prog.arrays())
    variants = [c % NVAR for c in range(max(SIZES))]
    inputs = np.stack([rec.input(v) for v in variants])
    insts = [pc.instance(v) for v in variants]
    kept = {}

    def keeping(phase, ch):
        out = []
        for b in range(ch.shape[0]):
            ints = tuple(orc.fr_to_int(ch[b, j]) for j in range(ch.shape[1]))
            key = (phase, variants[b], ints)
            if key not in kept:
                kept[key] = {c: to_mont_array(v) for c, v in pc.witness(phase, list(ints), variants[b]).items()}
            out.append(kept[key])
        return out

    sizes = {}
    for n in SIZES:
        seeds = list(range(100, 100 + n))
        forms = {"prove_inputs": lambda: prover.prove_inputs(plan, inputs[:n], seeds)[0],
                 "prove_phased_python": lambda: prover.prove_phased(pc.synthesize(variants[:n]), insts[:n], seeds)[0],
                 "prove_phased_kept": lambda: prover.prove_phased(keeping, insts[:n], seeds)[0]}
        made = {f: fn() for f, fn in forms.items()}  # one warm-up per shape
        assert made["prove_inputs"] == made["prove_phased_python"] == made["prove_phased_kept"] and all(made["prove_inputs"])
        times = {f: [] for f in forms}
        for _ in range(REPS):  # alternating
            for f, fn in forms.items():
                t0 = time.perf_counter()
                fn()
                times[f].append(time.perf_counter() - t0)
        e = {f: entry(t, n) for f, t in times.items()}
        ctx.profile(True)
        ctx.profile_collect()
        for _ in range(REPS):
            forms["prove_inputs"]()
        prof = ctx.profile_collect()
        ctx.profile(False)
        e["kernels_us_per_launch"] = {kn: round(prof[kn][1] / prof[kn][0] * 1e3, 1) for kn in ("witness_run_field", "witness_finish_phase") if kn in prof}
        e["kernel_launches_per_call"] = {kn: prof[kn][0] // REPS for kn in ("witness_run_field", "witness_finish_phase") if kn in prof}
        e["inputs_over_python"] = round(e["prove_inputs"]["ms_per_input"] / e["prove_phased_python"]["ms_per_input"], 4)
        e["inputs_over_kept"] = round(e["prove_inputs"]["ms_per_input"] / e["prove_phased_kept"]["ms_per_input"], 4)
        sizes[str(n)] = e
        print(name, n, json.dumps(e), flush=True)
    res["circuits"][name] = {"k": pc.cs.k, "phases": pc.n_phases, "challenges": len(pc.challenge_phase), "plan": plan.info(),
                             "operations": len(prog.tape.ops), "sizes": sizes}
    plan.close()
    prover.close()


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r24", "inputs_time.json")
    res = {"reps": REPS, "circuits": {}}
    if "--guard" in sys.argv:  # (child processes first: this one has not opened the GPU yet)
        i = sys.argv.index("--guard")
        this = sys.argv[i + 2] if len(sys.argv) > i + 2 and not sys.argv[i + 2].startswith("--") else os.path.join(ROOT, "0g-halo2_amd", "libzg_halo2.so")
        res["integer_only_guard"] = guard(sys.argv[i + 1], this)
        print(json.dumps(res["integer_only_guard"]), flush=True)
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)

    import orc
    import zg_halo2 as zg

    orc.load().orc_set_threads(16)
    ctx = zg.Ctx(0)  # (raises without a GPU: the tool measures nothing on a CPU)
    res["device"] = torch.cuda.get_device_name(0)
    for name in ("rlc", "shuffle"):
        measure(zg, orc, ctx, name, res)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
