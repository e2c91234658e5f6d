"""The host half of the SRS contribution entries, without a GPU: zg_params_g2 and zg_g2_mul against the oracle's G2
arithmetic, and the scalar recoding of the per-point multiplication (csrc/g1_mul_digits.h) against Python integers
through its stand-alone probe (tests/abi/g1_mul_probe.hip, built by the package Makefile)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import srs_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "abi", "g1_mul_probe")
R = sc.R
WIDTHS = (2, 3, 4, 5)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def orc_g2_mul(orc, q, t_int):
    out = np.zeros(16, np.uint64)
    q = np.ascontiguousarray(q, dtype=np.uint64)
    orc.load().orc_g2a_mul(_p(out), _p(q), _p(orc.fr_from_int(t_int)))
    return out


def orc_params_g2(orc, s_int):
    prm = orc.params_from_scalar(0, orc.fr_from_int(s_int))
    return np.array(prm.g2, np.uint64), np.array(prm.s_g2, np.uint64)


SCALARS = [1, 2, R - 1, random.Random(7).randrange(R)]


@pytest.mark.parametrize("s", SCALARS, ids=["1", "2", "r-1", "random"])
def test_params_g2_equals_the_oracle(zg, orc, s):
    g2, s_g2 = zg.params_g2(sc.fr_mont(s))
    want_g2, want_s_g2 = orc_params_g2(orc, s)
    assert np.array_equal(g2, want_g2)
    assert np.array_equal(s_g2, want_s_g2)


def test_params_g2_refuses_a_non_canonical_scalar(zg):
    with pytest.raises(zg.ZgError) as e:
        zg.params_g2(sc.fr_raw_limbs(R))
    assert e.value.status == -1


def test_g2_mul_equals_the_oracle(zg, orc):
    g2, _ = orc_params_g2(orc, 1)
    q = orc_g2_mul(orc, g2, 0xABCDEF0123456789)  # not the generator
    for t in (0, 1, 2, R - 1, random.Random(8).randrange(R)):
        got = zg.g2_mul(q, sc.fr_mont(t))
        assert np.array_equal(got, orc_g2_mul(orc, q, t)), hex(t)
        if t == 0:
            assert not got.any()
        if t == 1:
            assert np.array_equal(got, q)
        if t == R - 1:  # the negation: same x, y and its negative sum to q (mod q) limb-wise is not checked; x suffices
            assert np.array_equal(got[:8], q[:8]) and not np.array_equal(got[8:], q[8:])


def test_g2_mul_of_the_identity_is_the_identity(zg):
    ident = np.zeros(16, np.uint64)
    for t in (0, 1, 5, R - 1):
        assert not zg.g2_mul(ident, sc.fr_mont(t)).any()


def test_g2_mul_refuses_bad_points_and_scalars(zg, orc):
    g2, _ = orc_params_g2(orc, 1)
    out_before = np.full(16, 0x5A5A5A5A5A5A5A5A, np.uint64)
    lib = zg.load()

    def status(q, t):
        out = out_before.copy()
        st = lib.zg_g2_mul(_p(np.ascontiguousarray(q)), _p(np.ascontiguousarray(t)), _p(out))
        assert np.array_equal(out, out_before)  # a refused call writes nothing
        return st

    off = g2.copy()
    off[8] ^= np.uint64(1)  # y.c0 changed: off the twist
    assert status(off, sc.fr_mont(3)) == -1
    noncanon = g2.copy()
    noncanon[:4] = np.array(sc.limbs(sc.Q), np.uint64)  # x.c0 = q: not below q
    assert status(noncanon, sc.fr_mont(3)) == -1
    assert status(g2, sc.fr_raw_limbs(R)) == -1
    assert status(g2, sc.fr_raw_limbs((1 << 256) - 1)) == -1
    assert lib.zg_g2_mul(None, _p(sc.fr_mont(3)), _p(out_before.copy())) == -1


# ---- the recoding ----
def recoding_scalars(w):
    out = sc.edge_scalars(w) + [(1 << 254) - 1]  # (the contract is a value below 2^254)
    windows = (255 + w - 1) // w
    for j in range(windows + 1):
        for v in ((1 << (w * j)) - 1, 1 << max(w * j - 1, 0)):
            if v < 1 << 254:
                out.append(v)
    rng = random.Random(1500 + w)
    return out + [rng.randrange(R) for _ in range(200)]


def run_probe(rows, tmp_path):
    assert os.path.exists(PROBE), "run __graft_entry__.build() first"
    fin = tmp_path / "scalars.txt"
    fin.write_text("".join("%d %x\n" % row for row in rows))
    r = subprocess.run([PROBE, str(fin)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    return [[int(t) for t in line.split()] for line in lines]


def test_digits_sum_to_the_scalar(tmp_path):
    rows = [(w, s) for w in WIDTHS for s in recoding_scalars(w)]
    for (w, s), vals in zip(rows, run_probe(rows, tmp_path)):
        windows, top, ds = vals[0], vals[1], vals[2:]
        assert windows == (255 + w - 1) // w and len(ds) == windows, (w, hex(s))
        half = 1 << (w - 1)
        assert all(-half <= d <= half - 1 for d in ds), (w, hex(s), ds)
        assert top in (0, 1) and (top == 0 or w * windows < 256), (w, hex(s))
        # ds[0] is the top window: the order the kernel meets them in
        value = top << (w * windows)
        for j, d in enumerate(reversed(ds)):
            value += d << (w * j)
        assert value == s, (w, hex(s), top, ds)
        assert (windows, top, ds) == sc.digits(s, w)
    assert len(rows) > 4 * 200


def test_the_kernel_width_is_one_the_probe_covers():
    r = subprocess.run([PROBE, "width"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and int(r.stdout) in WIDTHS


def test_the_digit_check_can_fail(tmp_path):
    (vals,) = run_probe([(3, R - 1)], tmp_path)
    windows, top, ds = vals[0], vals[1], vals[2:]
    ds[5] += 1
    assert (top << (3 * windows)) + sum(d << (3 * j) for j, d in enumerate(reversed(ds))) != R - 1


def test_python_curve_reference_agrees_with_the_oracle(orc):
    """the reference of the GPU tests (srs_cases.mul) against the oracle's one-term msm, including the edges"""
    prm = orc.params_new(2)
    g = prm.g_np()
    p = sc.np_to_affine(g[3])
    for k in (0, 1, 2, R - 1, R - 2, (R + 1) // 2, 1 << 253, random.Random(9).randrange(R)):
        want = orc.msm(sc.fr_mont(k).reshape(1, 4), g[3:4])
        got = sc.affine_to_np(sc.mul(p, k))
        if k == 0:
            assert not got.any() and not want[8:].any()
        else:
            assert np.array_equal(got, want[:8]), hex(k)
