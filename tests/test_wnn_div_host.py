"""csrc/div64.h -- the division by a per-model reciprocal behind the WNN hash (x^3 mod p, the hash indices; csrc/wnn.hip) --
is plain integer code for host and device: here the host build is held against `unsigned __int128` (tests/abi/div64_probe.cpp),
including operands that take each of the algorithm's two correction steps, which seeded GPU inputs need not reach."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_invariant_division_equals_128_bit_integers(tmp_path):
    exe = str(tmp_path / "div64_probe")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "0g-halo2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "abi", "div64_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"checked (\d+) bad (\d+) first_correction (\d+) second_correction (\d+)", r.stdout)
    assert m, r.stdout
    checked, bad, first, second = (int(x) for x in m.groups())
    assert checked == 200 * (2 * 20000 + 25) and bad == 0
    assert first > 0 and second > 0, "a correction step of div_2by1 was never taken: the operands prove nothing about it"
