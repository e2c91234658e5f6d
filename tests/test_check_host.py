"""Host side of the witness check (zg_prover_check_*, csrc/check.hip): the permutation mapping recovered from sigma
values, the new entries and the zg_failure layout, and the tests' own failure enumerator (tests/check_enum.py) pinned
against Assignment.check() so that the GPU tests compare with something that was itself checked on the CPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from check_enum import COPY, GATE, LOOKUP, advice_table_circuit, changed, failures, satisfied_by_check, wrap_circuit
from circuit import ADVICE, INSTANCE
from circuits import toy_circuit, variant_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_model():
    import wnn_circuit
    import wnn_model

    kk, name = wnn_model.MNIST_TINY
    cs, asg, ilen, _ = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), kk)
    return cs, asg, ilen


CIRCUITS = {
    "toy5": lambda: toy_circuit(5),
    "toy10": lambda: toy_circuit(10),
    "no_lookup": lambda: variant_circuit("no_lookup", 6),
    "wide_lookup": lambda: variant_circuit("wide_lookup", 6),
    "tiny": tiny_model,
}


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_permutation_mapping_equals_assembly_mapping(zg, name):
    cs, asg, _ = CIRCUITS[name]()
    next_col, next_row = zg.permutation_mapping(asg.sigma_values(), cs.k)
    want = np.array(asg.mapping, dtype=np.uint32)  # [n_perm][n][2]
    assert next_col.shape == want.shape[:2]
    assert np.array_equal(next_col, want[:, :, 0]) and np.array_equal(next_row, want[:, :, 1])


def test_permutation_mapping_rejects_a_foreign_value(zg):
    cs, asg, _ = toy_circuit(5)
    sigma = asg.sigma_values().copy()
    sigma[2, 7] = zg.fr_from_int(5)  # 5 is no delta^c * omega^r with c < 5 (test_gpu_check.py builds a prover on it)
    with pytest.raises(zg.ZgError) as e:
        zg.permutation_mapping(sigma, cs.k)
    assert e.value.status == -1
    # ... and a label of a column the circuit does not have
    from circuit import DELTA, R

    sigma = asg.sigma_values().copy()
    sigma[0, 0] = zg.fr_from_int(pow(DELTA, len(cs.perm_columns), R))
    with pytest.raises(zg.ZgError):
        zg.permutation_mapping(sigma, cs.k)


def test_new_entries_are_exported_and_declared(zg):
    lib = zg.load()
    for name in ("zg_prover_check_batch", "zg_prover_check_batch_dev", "zg_prover_check_images", "zg_permutation_mapping"):
        assert name in zg.ABI_SYMBOLS and hasattr(lib, name), name
    for method in ("check", "check_batch", "check_images"):
        assert callable(getattr(zg.Prover, method))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_zg_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rs = open(os.path.join(ROOT, "shim", "halo2_proofs-zg", "src", "zg_sys.rs")).read()
    at = rs.index("pub struct zg_failure")
    assert "#[repr(C)]" in rs[rs.rindex("\n", 0, rs.rindex("\n", 0, at)):at]
    assert "pub kind: u32, pub index: u32, pub row: u32, pub other_index: u32, pub other_row: u32" in rs[at:at + 200]


def test_failure_layout_matches_the_c_compiler(zg, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "zg_halo2.h"\n'
        "int main(void) {\n"
        '    printf("%lu %lu %lu %lu %lu %lu %d %d %d\\n", (unsigned long)sizeof(zg_failure), (unsigned long)offsetof(zg_failure, kind),\n'
        "           (unsigned long)offsetof(zg_failure, index), (unsigned long)offsetof(zg_failure, row),\n"
        "           (unsigned long)offsetof(zg_failure, other_index), (unsigned long)offsetof(zg_failure, other_row),\n"
        "           ZG_FAIL_GATE, ZG_FAIL_LOOKUP, ZG_FAIL_COPY);\n"
        "    return 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    f = zg.Failure
    assert ctypes.sizeof(f) == 20
    assert got == [ctypes.sizeof(f), f.kind.offset, f.index.offset, f.row.offset, f.other_index.offset, f.other_row.offset,
                   zg.FAIL_GATE, zg.FAIL_LOOKUP, zg.FAIL_COPY]
    assert (GATE, LOOKUP, COPY) == (zg.FAIL_GATE, zg.FAIL_LOOKUP, zg.FAIL_COPY)


SATISFIED = {
    "toy5": lambda: toy_circuit(5),
    "toy6": lambda: toy_circuit(6),
    "toy10-two": lambda: toy_circuit(10, two_lookups=True),
    "no_lookup": lambda: variant_circuit("no_lookup", 6),
    "gates_only": lambda: variant_circuit("gates_only", 6),
    "wide_lookup": lambda: variant_circuit("wide_lookup", 6),
    "advice_factor": lambda: variant_circuit("advice_factor", 6),
    "merged_selectors": lambda: variant_circuit("merged_selectors", 6),
    "advice_table": advice_table_circuit,
    "wrap": wrap_circuit,
    "tiny": tiny_model,
}


@pytest.mark.parametrize("name", list(SATISFIED))
def test_enumerator_agrees_with_assignment_check_on_satisfied_witnesses(name):
    cs, asg, _ = SATISFIED[name]()
    assert satisfied_by_check(asg)
    assert failures(cs, asg) == ([0, 0, 0], [])


def test_enumerator_lists_what_assignment_check_asserts():
    """Single-cell changes: the enumerator's gate / lookup records are empty exactly when Assignment.check() passes, and
    the records are the ones worked out by hand for these circuits."""
    cs, asg, _ = toy_circuit(6)
    cases = [
        ([(ADVICE, 2, 7, lambda v: v + 1)], [(GATE, 0, 7, 0, 0), (GATE, 1, 7, 0, 0), (COPY, 0, 8, 2, 7), (COPY, 2, 7, 0, 8)]),
        ([(ADVICE, 1, 9, 1 << 20)], [(GATE, 0, 9, 0, 0), (LOOKUP, 0, 9, 0, 0)]),
        ([(INSTANCE, 0, 0, lambda v: v + 1)], [(COPY, 0, 56, 3, 0), (COPY, 3, 0, 2, 55)]),
        ([(ADVICE, 0, 0, lambda v: v + 12345)], [(GATE, 0, 0, 0, 0), (COPY, 0, 0, 4, 0), (COPY, 4, 0, 0, 0)]),
    ]
    for edits, want in cases:
        bad = changed(asg, edits)
        totals, recs = failures(cs, bad)
        assert recs == want and totals == [sum(1 for x in want if x[0] == kd) for kd in (GATE, LOOKUP, COPY)]
        assert satisfied_by_check(bad) == (totals[GATE] + totals[LOOKUP] == 0)
    # every advice cell changed: the every-row-fails witness of the cap tests
    n = 1 << cs.k
    bad = changed(asg, [(ADVICE, c, r, (1 << 20) + r + c) for c in range(3) for r in range(n)])
    totals, recs = failures(cs, bad)
    assert totals == [112, 56, 123] and len(recs) == 291 and recs == sorted(recs)
    # the all-zero witness is NOT such a case: both gates and the lookup hold, one copy pair is left
    zero = changed(asg, [(ADVICE, c, r, 0) for c in range(3) for r in range(n)] + [(INSTANCE, 0, 0, 0)])
    assert failures(cs, zero) == ([0, 0, 2], [(COPY, 0, 0, 4, 0), (COPY, 4, 0, 0, 0)])
    # a pair whose halves both occur in the table, but not together
    cs, asg, _ = variant_circuit("wide_lookup", 6)
    bad = changed(asg, [(ADVICE, 1, 5, 3 * ((asg.get(ADVICE, 0, 5) + 1) % 9) + 1)])
    assert failures(cs, bad) == ([0, 1, 0], [(LOOKUP, 0, 5, 0, 0)]) and not satisfied_by_check(bad)
    # a changed cell on a row where its gate is off is no failure
    for kind, row in (("advice_factor", 6), ("merged_selectors", 12)):
        cs, asg, _ = variant_circuit(kind, 6)
        assert failures(cs, changed(asg, [(ADVICE, 1, row, lambda v: v + 1)])) == ([0, 0, 0], [])
        assert failures(cs, changed(asg, [(ADVICE, 1, 9, lambda v: v + 1)])) == ([1, 0, 0], [(GATE, 0, 9, 0, 0)])
    # the witness-side table and the wrapping rotation
    cs, asg, _ = advice_table_circuit()
    assert failures(cs, changed(asg, [(ADVICE, 0, 4, 99)])) == ([0, 1, 0], [(LOOKUP, 0, 4, 0, 0)])
    cs, asg, _ = wrap_circuit()
    assert failures(cs, changed(asg, [(ADVICE, 1, asg.n - 1, 40)])) == ([1, 0, 0], [(GATE, 0, 0, 0, 0)])
