"""The scalar recoding of the variable-base MSM (csrc/msm_var_digits.h) on the CPU, against Python integers: a stand-alone
probe with its own main (tests/abi/msm_var_probe.hip), built here into tmp_path -- once plainly, once with
-fsanitize=signed-integer-overflow on the host code (the flags of tests/test_field9_host.py).  Nothing is loaded into
Python and nothing runs on a device."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "abi", "msm_var_probe.hip")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
WIDTHS = range(2, 17)


def windows(c):
    return (255 + c - 1) // c


def scalars_for(c):
    """0, 1, r - 1, 2^253, 2^(cw) - 1 and 2^(cw - 1) for every window w, 200 seeded random values"""
    out = [0, 1, R - 1, 1 << 253]
    for w in range(windows(c) + 1):
        for v in ((1 << (c * w)) - 1, (1 << (c * w - 1)) if c * w >= 1 else 0):
            if v < 1 << 254:  # (the recoding's contract: a scalar is a residue below r < 2^254)
                out.append(v)
    rng = random.Random(1000 + c)
    out += [rng.randrange(R) for _ in range(200)]
    return out


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["hipcc", "-O1", "-Xarch_device", "-O0", "-std=c++17", "--offload-arch=gfx950", *extra, "-Wall", "-Wno-unused-function",
                    SRC, "-o", exe], check=True)
    return exe


def check_digits(exe, tmp_path):
    rows = [(c, s) for c in WIDTHS for s in scalars_for(c)]
    fin = tmp_path / "scalars.txt"
    fin.write_text("".join("%d %x\n" % (c, s) for c, s in rows))
    r = subprocess.run([exe, "digits", str(fin)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    for (c, s), line in zip(rows, lines):
        vals = [int(t) for t in line.split()]
        W, d = vals[0], vals[1:]
        assert W == windows(c) and len(d) == W, (c, hex(s))
        assert sum(dw << (c * w) for w, dw in enumerate(d)) == s, (c, hex(s), d)
        assert all(abs(dw) <= 1 << (c - 1) for dw in d), (c, hex(s), d)
        assert d[-1] >= 0, (c, hex(s), d)
    return len(rows)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("msm_var_probe"), "msm_var_probe", [])


def test_digits_sum_to_the_scalar_for_every_width(probe, tmp_path):
    n = check_digits(probe, tmp_path)
    print("%d (width, scalar) pairs" % n)
    assert n > 15 * 200


def test_digits_have_no_signed_overflow(tmp_path):
    """a second, stand-alone build with the host flags of test_field9_host's sanitizer pass; the first overflow ends it"""
    exe = build(tmp_path, "msm_var_probe_ubsan", ["-Xarch_host", "-fsanitize=signed-integer-overflow", "-Xarch_host", "-fno-sanitize-recover=all"])
    check_digits(exe, tmp_path)


def test_default_width_rule(probe, tmp_path):
    """window_bits = 0: argmin over c of ceil(255 / c) (n + 4 2^(c-1)), restated here; 2 or 3 below n = 32 as halo2's own
    rule; lowered while batch * W * 2^(c-1) exceeds 2^24 bucket sums"""
    def rule(n, batch):
        best = min(WIDTHS, key=lambda c: (windows(c) * (n + 4 * (1 << (c - 1))), c))
        while best > 2 and batch * windows(best) * (1 << (best - 1)) > 1 << 24:
            best -= 1
        return best

    cases = [(n, 1) for n in list(range(1, 70)) + [255, 256, 1000, 4096, 1 << 14, 1 << 17, 1 << 20, (1 << 23) - 1]]
    cases += [(1 << 17, b) for b in (3, 64, 256)] + [((1 << 23) - 1, 256), (1, 256)]
    fin = tmp_path / "sizes.txt"
    fin.write_text("".join("%d %d\n" % nb for nb in cases))
    r = subprocess.run([probe, "width", str(fin)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in r.stdout.split()]
    assert got == [rule(n, b) for n, b in cases]
    assert all(g in (2, 3) for (n, _), g in zip(cases, got) if n < 32)
    assert all(2 <= g <= 16 for g in got)
    assert dict(zip(cases, got))[(1 << 14, 1)] == 10 and dict(zip(cases, got))[(1 << 17, 1)] == 13


def test_the_check_can_fail(probe, tmp_path):
    """a digit changed by one no longer sums to the scalar: the comparison above is not vacuous"""
    fin = tmp_path / "one.txt"
    fin.write_text("5 %x\n" % (R - 1))
    d = [int(t) for t in subprocess.run([probe, "digits", str(fin)], capture_output=True, text=True, check=True).stdout.split()][1:]
    assert sum(dw << (5 * w) for w, dw in enumerate(d)) == R - 1
    d[3] += 1
    assert sum(dw << (5 * w) for w, dw in enumerate(d)) != R - 1
