"""tests/field_tape.py against the circuits it records: the Python-integer interpreter of the witness program with field
operations, challenges and phases must give, for every recorded program, exactly Phased.full_advice -- and its field
operations must be exact on operands anywhere in [0, 2^256).  No device: this keeps a wrong test program from being
mistaken for a wrong kernel in tests/test_gpu_witness_field.py."""
import random

import numpy as np
import pytest

import field_tape
from circuit import R
from field_tape import EDGE, evaluate


@pytest.mark.parametrize("name", sorted(field_tape.RECORDERS))
def test_recorded_program_gives_the_circuits_own_witness(name):
    rec = field_tape.recorded(name)
    pc, prog = rec.pc, rec.program
    rnd = random.Random(sum(name.encode()))
    nch = len(pc.challenge_phase)
    for variant in (0, 1, 2, 5):
        data = rec.input(variant)
        assert data.shape == (prog.input_bytes,)
        for _ in range(2):
            ch = [rnd.randrange(R) for _ in range(nch)]
            assert np.array_equal(prog.columns(data, ch), pc.full_advice(ch, variant)), (name, variant)
            _, inst = prog.column_ints(data, ch)
            want = pc.instance(variant)
            assert len(inst) == (want.shape[1] if want.shape[0] else 0)
            if inst:
                from circuit import to_mont_array

                assert np.array_equal(to_mont_array(inst), want[0])


@pytest.mark.parametrize("name", sorted(field_tape.RECORDERS))
def test_arrays_are_a_well_formed_plan(name):
    """what zg_witness_plan_create_field checks, on the arrays as the builder lays them out"""
    rec = field_tape.recorded(name)
    prog, t = rec.program, rec.program.tape
    a = prog.arrays()
    ops, ls, pls = a["ops"], a["level_start"], a["phase_level_start"]
    assert ls[0] == 0 and ls[-1] == len(ops) and all(ls[i] < ls[i + 1] for i in range(len(ls) - 1))
    assert pls[0] == 0 and pls[-1] == len(ls) - 1 and len(pls) == t.n_phases + 1 and all(pls[i] <= pls[i + 1] for i in range(len(pls) - 1))
    level_of = np.zeros(len(ops), int)
    for lv in range(len(ls) - 1):
        level_of[ls[lv]:ls[lv + 1]] = lv
    phase_of = [max(ph for ph in range(t.n_phases) if pls[ph] <= level_of[i]) for i in range(len(ops))]
    for i, (op, x, y, imm) in enumerate(ops.tolist()):
        nm = field_tape.OPS[op]
        if nm not in field_tape.NO_OPERAND:
            assert level_of[x] < level_of[i]
        if nm in field_tape.TWO_OPERANDS:
            assert level_of[y] < level_of[i]
        if nm == "CHAL":
            assert phase_of[i] > t.challenge_phase[imm]
    for c in range(prog.n_advice):
        for s in a["cell_slot"][c]:
            assert s == field_tape.NO_SLOT or phase_of[s] <= prog.advice_phase[c]
    assert all(phase_of[s] == 0 for s in a["instance_slots"])


def test_field_operations_on_edge_operands():
    for x in EDGE:
        inv = evaluate("INVM", x, 0, 0, [], [], b"", [])
        assert 0 <= inv < R
        if x % R == 0:
            assert inv == 0
        else:
            assert evaluate("MULM", inv, x, 0, [], [], b"", []) == 1
        for y in EDGE:
            s, d, m = (evaluate(nm, x, y, 0, [], [], b"", []) for nm in ("ADDM", "SUBM", "MULM"))
            assert 0 <= s < R and 0 <= d < R and 0 <= m < R
            assert (s - x - y) % R == 0 and (d - x + y) % R == 0 and (m - x * y) % R == 0
    assert evaluate("CHAL", 0, 0, 0, [], [], b"", [R - 1]) == R - 1
    # the edge program: every description once, every value the interpreter's
    prog, out = field_tape.edge_program()
    v = prog.tape.run(b"\0", [R - 1])
    got = dict((d, v[val.idx]) for d, val in out)
    assert len(got) == len(out) == len(EDGE) * (2 + 3 * len(EDGE)) + 3
    assert got["INVM 0"] == 0 and got["INVM 3"] == 0 and got["INVM(x) x 1"] == 1 and got["INVM(x) x 9"] == 1
    assert got["CHAL"] == R - 1 and got["CHAL + 1"] == 0 and got["CHAL^-1"] == R - 1
