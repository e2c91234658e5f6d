"""The (tuple, row) order of the witness check's shuffle sort (csrc/check_tuple.h) on the CPU, against Python's sorted() on
the canonical integers: a stand-alone probe with its own main (tests/abi/check_tuple_probe.hip), built here into tmp_path
-- once plainly, once with -fsanitize=undefined on the host code.  Nothing is loaded into Python and nothing runs on a
device."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "abi", "check_tuple_probe.hip")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = (1 << 256) % R


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["hipcc", "-O1", "-Xarch_device", "-O0", "-std=c++17", "--offload-arch=gfx950", *extra, "-Wall", "-Wno-unused-function",
                    SRC, "-o", exe], check=True)
    return exe


def inputs():
    """name -> (usable, rows of tuples)"""
    rng = random.Random(2020)
    out = {}
    # values whose Montgomery order differs from their canonical order
    vals = [rng.randrange(R) for _ in range(64)] + [0, 1, 2, R - 1, R - 2]
    assert sorted(vals) != sorted(vals, key=lambda v: v * MONT % R)
    out["montgomery_order_differs"] = (len(vals) - 3, [(v,) for v in vals])
    # tuples equal up to the last component
    head = (rng.randrange(R), 7, rng.randrange(R))
    rows = [head + (rng.randrange(40),) for _ in range(100)]
    out["equal_up_to_the_last_component"] = (96, rows)
    # values that differ in one 32-bit limb only
    base = rng.randrange(1 << 253)
    rows = [(base ^ (rng.randrange(1, 1 << 32) << (32 * limb)), base) for limb in range(8) for _ in range(6)]
    rows = [(a % R, b) for a, b in rows] + [(base, base)] * 3
    rng.shuffle(rows)
    out["one_limb_differs"] = (len(rows), rows)
    # all-equal tuples: the order is by row; the rows from usable on come last, whatever they hold
    out["all_equal"] = (40, [(5, 5, 5)] * 40 + [(0, 0, 0), (R - 1, 1, 1), (5, 5, 5), (4, 9, 9)])
    # many ties among few values, width 2
    out["ties"] = (250, [(rng.randrange(3), rng.randrange(3)) for _ in range(256)])
    return out


def expected(usable, rows):
    order = [r for _, r in sorted((rows[r], r) for r in range(usable))] + list(range(usable, len(rows)))
    cmps = [(rows[a] > rows[b]) - (rows[a] < rows[b]) for a, b in zip(order[:usable], order[1:usable])]
    return order, cmps


def run(exe, tmp_path):
    for name, (usable, rows) in inputs().items():
        fin = tmp_path / (name + ".txt")
        fin.write_text("%d %d %d\n" % (len(rows), usable, len(rows[0])) + "".join(" ".join("%x" % v for v in t) + "\n" for t in rows))
        r = subprocess.run([exe, str(fin)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-2000:])
        lines = r.stdout.splitlines()
        assert lines[-1].startswith("cmp")
        order, cmps = expected(usable, rows)
        assert [int(x) for x in lines[:-1]] == order, name
        assert [int(x) for x in lines[-1].split()[1:]] == cmps, name
        assert all(c <= 0 for c in cmps)


def test_header_exists():
    assert os.path.exists(os.path.join(ROOT, "0g-halo2_amd", "csrc", "check_tuple.h"))


def test_order_is_sorted_on_canonical_integers_then_row(tmp_path):
    run(build(tmp_path, "check_tuple_probe", []), tmp_path)


def test_order_under_the_undefined_behaviour_sanitizer(tmp_path):
    """a second, stand-alone build with -fsanitize=undefined on the host code; the first finding ends it"""
    run(build(tmp_path, "check_tuple_probe_ubsan", ["-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"]), tmp_path)
