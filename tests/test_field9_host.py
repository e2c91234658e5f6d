"""The host leg of the field9 probe.  csrc/field9.h up to xyzz9_add / xyzz9_to_xyzz is plain C++ for host and device, so
the records of tests/test_gpu_field9.py that need no DPP run here on the CPU under the same judge (tests/field9_cases.py,
tests/field9_ref.py) -- and once more in a build with -fsanitize=signed-integer-overflow: an int64 column or an int32 limb
sum that overflows at a contract's bound is undefined behaviour here and wraps silently on the device.  Also: the judge
itself has to be able to fail."""
import os
import subprocess

import numpy as np
import pytest

import field9_cases as fc
import field9_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "abi", "field9_probe")


def run_host(exe, tmp_path):
    rows, arr = fc.host_cases()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    arr.tofile(fin)
    r = subprocess.run([exe, "host", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print("records per op: %s" % sorted(fc.counts(rows).items()))
    fails = fc.judge(rows, fc.read_out(fout, len(rows)))
    assert not fails, "%d wrong results, the first:\n%s" % (len(fails), "\n".join(fails[:8]))


def test_every_generated_case_is_covered_by_host_or_lane_ops():
    rows, arr = fc.all_cases()
    assert arr.shape == (len(rows), fc.IN_WORDS) and {r[0] for r in rows} == set(fc.OP.values())
    assert [r[0] for r in rows] == sorted(r[0] for r in rows), "one run of records per op"
    n = fc.counts(rows)
    assert all(n["%s/%s" % (op, f)] > 0 for op in ("mul", "sqr", "mul2_add", "mul2_sub", "mul2_split", "dot", "canon", "iszero", "reduce_pack",
                                                   "mul_small", "fe_mul", "fe_add", "fe_sub") for f in ("Fq", "Fr"))
    assert n["xmadd_pair/Fq"] % 8 == 0
    assert {r[0] for r in fc.host_cases()[0]} == fc.HOST_OPS


def test_host_build_meets_the_contracts(tmp_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    run_host(EXE, tmp_path)


def test_host_build_has_no_signed_overflow_at_the_bounds(tmp_path):
    """a second, stand-alone build of the probe (nothing preloaded, nothing loaded into Python); the first overflow ends it"""
    exe = str(tmp_path / "field9_probe_ubsan")
    subprocess.run(["hipcc", "-O1", "-Xarch_device", "-O0", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host",
                    "-fsanitize=signed-integer-overflow", "-Xarch_host", "-fno-sanitize-recover=all", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi", "field9_probe.hip"), "-o", exe], check=True)
    run_host(exe, tmp_path)


# ---- the judge can fail ------------------------------------------------------------------------------------------------------
def out_record(slots, inf=0, wm=0, zero=0):
    o = [ref.SENTINEL] * (9 * fc.OUT_SLOTS) + [inf, wm, zero, 0]
    for i, s in enumerate(slots):
        o[9 * i:9 * i + 9] = s
    return np.array([o], dtype=np.int64).astype(np.int32)


def test_the_judge_rejects_wrong_results():
    p = ref.Q
    a, b = ref.split(p - 1), ref.split((1 << 256) - 1)
    row = (fc.OP["mul"], 0, 0, [a, b] * 4)
    good = ref.split(ref.mont(ref.val(a) * ref.val(b), p))
    assert fc.judge([row], out_record([good] * 4)) == []
    off_by_p = ref.split(ref.val(good) + p)  # the right residue, the wrong representative
    assert "1*p+0" in fc.judge([row], out_record([off_by_p] * 4))[0]
    moved = list(good)  # the right VALUE, a limb off by one and the next limb making up for it
    moved[3] += 1 << 29
    moved[4] -= 1
    assert ref.val(moved) == ref.val(good)
    assert "same value, other limbs" in fc.judge([row], out_record([moved] * 4))[0]
    # points
    P, S = ref.ec_mul(5, ref.G), ref.ec_mul(7, ref.G)
    pa, pb = fc.limbs_of(fc.xyzz_res(P, 3), [0] * 4), fc.limbs_of(fc.xyzz_res(S, 1), [0] * 4)
    row = (fc.OP["xaddl2"], 0, 0, pa + pb)
    sm = fc.limbs_of(fc.xyzz_res(ref.ec_add(P, S), 11), [1, -1, 0, 2])
    assert fc.judge([row], out_record(sm + sm, wm=0xB4)) == []
    neg = [sm[0], ref.split(-ref.val(sm[1])), sm[2], sm[3]]
    assert "NEGATIVE" in fc.judge([row], out_record(neg + neg, wm=0xB4))[0]
    unwritten = [sm[0], [ref.SENTINEL] * 9, sm[2], sm[3]]
    assert "y was not written" in fc.judge([row], out_record(unwritten + sm, wm=0xB4))[0]
    assert "differs from xyzz9_add" in fc.judge([row], out_record(sm + fc.limbs_of(fc.xyzz_res(ref.ec_add(P, S), 2), [0] * 4), wm=0xB4))[0]
    assert "write masks" in fc.judge([row], out_record(sm + sm, wm=0xB0))[0]
    wrong_zzz = [sm[0], sm[1], sm[2], ref.split(ref.val(sm[3]) + 1)]
    assert "zz^3 != zzz^2" in fc.judge([row], out_record(wrong_zzz + wrong_zzz, wm=0xB4))[0]
    # P + (-P) has to be the all-zero identity, a float quotient one too high leaves a negative value, a zero test that says no
    row = (fc.OP["add"], 0, 0, pa + fc.limbs_of(fc.xyzz_res(ref.ec_neg(P), 2), [0] * 4))
    assert fc.judge([row], out_record([fc.ZERO9] * 4)) == []
    assert "identity" in fc.judge([row], out_record(sm))[0]
    row = (fc.OP["mul_small"], 1, -4096, [ref.split(ref.R - 1)] * 8)
    e = (ref.R - 1) * -4096 % ref.R
    assert fc.judge([row], out_record([ref.split(e + ref.R)] * 8)) == []
    assert len(fc.judge([row], out_record([ref.split(e - ref.R)] * 8))) == 8
    row = (fc.OP["iszero"], 0, 0, [ref.split(3 * p)] * 8)
    assert fc.judge([row], out_record([], zero=0xFF)) == [] and len(fc.judge([row], out_record([], zero=0x7F))) == 1
