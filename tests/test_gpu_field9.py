"""The primitives of csrc/field9.h and the device path of csrc/field.h, one by one, on the GPU against Python integers: the
nine-limb products with their shared reductions, the two float quotient estimates, the zero test, the XYZZ formulas and
their 2- and 4-lane DPP forms -- at the bounds their comments state (a carry across a 29-bit boundary, one below a multiple
of p, equal points under other representatives and scalings, a column at 27 * 2^58), which seeded MSMs, NTTs and proofs do not
reach.  tests/abi/field9_probe.hip runs ONCE for the whole module; the cases and the judge are tests/field9_cases.py and
tests/field9_ref.py.  Every comparison is exact."""
import os
import re
import subprocess

import pytest

import field9_cases as fc

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "abi", "field9_probe")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """(rows, OUT array) of the one device run; a probe that fails or runs out of time fails every test here, once"""
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    d = tmp_path_factory.mktemp("field9")
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    rows = fc.write_in(fin)
    try:
        r = subprocess.run([EXE, "device", fin, fout], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.fail("field9_probe device did not end in 120 s: %s %s" % (e.stdout, e.stderr))
    if r.returncode != 0:
        pytest.fail("field9_probe device exit %d: %s%s" % (r.returncode, r.stdout, r.stderr))
    print("records per op: %s" % sorted(fc.counts(rows).items()))
    return rows, fc.read_out(fout, len(rows))


def judged(probe, ops, lanes="all"):
    rows, out = probe
    n = {k: v for k, v in fc.counts(rows).items() if k.split("/")[0] in ops}
    assert {k.split("/")[0] for k in n} == set(ops), "an op family without records"
    print("records: %s" % sorted(n.items()))
    fails = fc.judge(rows, out, only=lambda name: name in ops, lanes=lanes)
    per_op = {}
    for f in fails:  # counted by op and, for a limb-for-limb difference, by coordinate and amount
        m = re.search(r"(coordinate \d) .*\(by ([^)]*)\)", f.split("\n")[0])
        key = f.split()[0] + (" %s by %s" % m.groups() if m else "")
        per_op[key] = per_op.get(key, 0) + 1
    print("wrong results per op: %s" % sorted(per_op.items()))
    assert not fails, "%d wrong results %s, the first:\n%s" % (len(fails), sorted(per_op.items()), "\n".join(fails[:4]))


def test_unpack_pack_and_norm(probe):
    judged(probe, ("unpack", "pack", "norm"))


def test_products_with_one_reduction(probe):
    """Field9::mul, sqr, mul2<false>, mul2<true>, mulq + sub_fused, Dot9: limb for limb (T + m p) / 2^261"""
    judged(probe, ("mul", "sqr", "mul2_add", "mul2_sub", "mul2_split", "dot"))


def test_canon_and_the_zero_test(probe):
    judged(probe, ("canon", "iszero"))


def test_float_quotient_estimates(probe):
    """f9_reduce_pack around every multiple of p below 2^263; f9_mul_small for every c and around x c = m p"""
    judged(probe, ("reduce_pack", "mul_small"))


def test_the_8x32_device_path(probe):
    """Fr / Fq mul (the generated product-scanning asm), sqr, add, sub, neg, dbl, from_raw, to_raw"""
    judged(probe, ("fe_mul", "fe_sqr", "fe_add", "fe_sub", "fe_neg", "fe_dbl", "fe_from_raw", "fe_to_raw"))


def test_curve_formulas(probe):
    judged(probe, ("madd", "from_pair", "dbl", "add", "to_xyzz"))


XADDS = ("xaddl1", "xaddl2", "xaddl4", "xadd1", "xadd2", "xadd4")


def test_lane_split_additions_store_the_python_point(probe):
    """xaddl<1, 2, 4> and xadd<false>, xadd<true>, xadd4 through xstore: every coordinate written by exactly one lane, a
    valid operand of the next addition, and the Python point"""
    judged(probe, XADDS, lanes="point")


def test_lane_split_additions_equal_xyzz9_add_limb_for_limb(probe):
    """the same stored sums, limb for limb what xyzz9_add returns for the same operands in the same launch: the lanes reduce
    R (Q - X3) and S1 PPP apart and Field9::sub_fused has to settle the q between that and the one reduction of xyzz9_add"""
    judged(probe, XADDS, lanes="limbs")


def test_xmadd_pair_chains_hold_the_python_point(probe):
    """after every step of every chain: both lanes carry the same inf, the reassembled point is a valid operand and the
    Python point, lane B's zzz is lane A's"""
    judged(probe, ("xmadd_pair",), lanes="point")


def test_xmadd_pair_chains_equal_xyzz9_madd_limb_for_limb(probe):
    """after every step x, y, zz, zzz and inf of the pair are those of xyzz9_madd on one lane of the same chain"""
    judged(probe, ("xmadd_pair",), lanes="limbs")
