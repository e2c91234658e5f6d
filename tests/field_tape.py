"""Witness programs with field operations, challenges and advice phases (zg_witness_plan_create_field, DESIGN.md section
24): a small builder, a Python-integer interpreter of the WHOLE operation set, and one recorded program for each test
circuit of tests/phases_circuits.py (SMALL) and for shuffle_circuits.plain, with the circuit's private data as
little-endian input bytes.

The interpreter is the reference of tests/test_gpu_witness_field.py; tests/test_field_tape_host.py holds it and the
recorded programs against Phased.full_advice, so that a wrong test program is not mistaken for a wrong kernel."""
import numpy as np

from circuit import R, to_mont_array

OPS = ["CONST", "PIXEL", "ADD", "SUB", "MUL", "ADDI", "RSUBI", "MULI", "SHRI", "SHLI", "ANDI", "SHRV", "GTI", "GEI", "EQI", "DIVI",
       "TABLE", "CHAL", "ADDM", "SUBM", "MULM", "INVM"]
OP = {name: i for i, name in enumerate(OPS)}
NO_OPERAND = ("CONST", "PIXEL", "CHAL")
TWO_OPERANDS = ("ADD", "SUB", "MUL", "SHRV", "ADDM", "SUBM", "MULM")
M256 = (1 << 256) - 1
NO_SLOT = 0xFFFFFFFF


def evaluate(name, a, b, imm, consts, table, data, challenges):
    """one operation on Python integers: a, b operand values (any 256-bit integers), the result modulo 2^256"""
    if name == "CONST": return consts[imm]
    if name == "PIXEL": return int(data[imm])
    if name == "ADD": return (a + b) & M256
    if name == "SUB": return (a - b) & M256
    if name == "MUL": return (a * b) & M256
    if name == "ADDI": return (a + imm) & M256
    if name == "RSUBI": return (imm - a) & M256
    if name == "MULI": return (a * imm) & M256
    if name == "SHRI": return a >> imm
    if name == "SHLI": return (a << imm) & M256
    if name == "ANDI": return a & imm
    if name == "SHRV": return a >> b if b < 256 else 0
    if name == "GTI": return int(a > imm)
    if name == "GEI": return int(a >= imm)
    if name == "EQI": return int(a == imm)
    if name == "DIVI": return a // imm
    if name == "TABLE": return table[imm + a] if imm + a < len(table) else 0
    if name == "CHAL": return challenges[imm] % R
    if name == "ADDM": return ((a % R) + (b % R)) % R
    if name == "SUBM": return ((a % R) - (b % R)) % R
    if name == "MULM": return (a % R) * (b % R) % R
    if name == "INVM": return pow(a % R, R - 2, R)  # (0 for a = 0 mod r)
    raise ValueError(name)


class Val:
    """handle of one recorded operation"""

    def __init__(self, tape, idx):
        self.tape, self.idx = tape, idx


class Tape:
    """Operations in recording order; each knows its phase (the largest of its operands', of the phase it was asked into,
    and -- for CHAL j -- challenge_phase[j] + 1) and its level inside the phase.  arrays() sorts them by (phase, level)."""

    def __init__(self, n_phases=1, challenge_phase=()):
        self.n_phases, self.challenge_phase = n_phases, list(challenge_phase)
        self.ops, self.consts, self.table = [], [], [0]  # ops: [name, a idx, b idx, imm, phase, level]

    def emit(self, name, a=None, b=None, imm=0, phase=0):
        deps = [v for v in (a, b) if v is not None]
        assert len(deps) == (0 if name in NO_OPERAND else 2 if name in TWO_OPERANDS else 1), name
        ph = max([phase] + [self.ops[v.idx][4] for v in deps] + ([self.challenge_phase[imm] + 1] if name == "CHAL" else []))
        assert ph < self.n_phases, (name, ph)
        level = max([-1] + [self.ops[v.idx][5] for v in deps if self.ops[v.idx][4] == ph]) + 1
        self.ops.append([name, a.idx if a is not None else 0, b.idx if b is not None else 0, imm, ph, level])
        return Val(self, len(self.ops) - 1)

    def const(self, v, phase=0):
        if v not in self.consts:
            self.consts.append(v)
        return self.emit("CONST", imm=self.consts.index(v), phase=phase)

    def byte(self, i):
        return self.emit("PIXEL", imm=i)

    def le(self, first, nbytes):
        """the little-endian integer in input bytes first .. first + nbytes"""
        v = self.byte(first)
        for j in range(1, nbytes):
            v = self.emit("ADD", v, self.emit("SHLI", self.byte(first + j), imm=8 * j))
        return v

    def chal(self, j):
        return self.emit("CHAL", imm=j)

    def addm(self, a, b): return self.emit("ADDM", a, b)
    def subm(self, a, b): return self.emit("SUBM", a, b)
    def mulm(self, a, b): return self.emit("MULM", a, b)
    def invm(self, a): return self.emit("INVM", a)

    def run(self, data, challenges=()):
        """every operation's value, in recording order, for input bytes `data` and challenges as canonical integers"""
        v = []
        for name, a, b, imm, _, _ in self.ops:
            v.append(evaluate(name, v[a] if name not in NO_OPERAND else 0, v[b] if name in TWO_OPERANDS else 0, imm, self.consts, self.table,
                              data, challenges))
        return v


class Program:
    """tape + which operation every advice cell and every instance row shows"""

    def __init__(self, tape, cells, instance, n_advice, k, input_bytes, advice_phase):
        self.tape, self.cells, self.instance = tape, dict(cells), list(instance)
        self.n_advice, self.k, self.n, self.input_bytes, self.advice_phase = n_advice, k, 1 << k, input_bytes, list(advice_phase)

    def order(self):
        """recording index -> slot: sorted by (phase, level), stable"""
        ops = self.tape.ops
        by = sorted(range(len(ops)), key=lambda i: (ops[i][4], ops[i][5]))
        slot = [0] * len(ops)
        for s, i in enumerate(by):
            slot[i] = s
        return by, slot

    def arrays(self, field=True):
        """what zg.WitnessPlan takes; field=False leaves the phase arrays out (zg_witness_plan_create)"""
        t, ops = self.tape, self.tape.ops
        by, slot = self.order()
        out = np.zeros((len(ops), 4), np.uint64)
        level_start, phase_level_start, prev = [], [], None
        for s, i in enumerate(by):
            name, a, b, imm, ph, lv = ops[i]
            if (ph, lv) != prev:
                while len(phase_level_start) <= ph:
                    phase_level_start.append(len(level_start))
                level_start.append(s)
                prev = (ph, lv)
            out[s] = (OP[name], slot[a] if name not in NO_OPERAND else 0, slot[b] if name in TWO_OPERANDS else 0, imm)
        while len(phase_level_start) <= t.n_phases:
            phase_level_start.append(len(level_start))
        level_start.append(len(ops))
        cell_slot = np.full((self.n_advice, self.n), NO_SLOT, np.uint32)
        for (c, r), v in self.cells.items():
            cell_slot[c, r] = slot[v.idx]
        consts = np.zeros((max(len(t.consts), 1), 4), np.uint64)
        for i, c in enumerate(t.consts):
            consts[i] = [(c >> (64 * w)) & ((1 << 64) - 1) for w in range(4)]
        a = dict(ops=out, level_start=np.array(level_start, np.uint32), consts=consts, table=np.array(t.table, np.uint64), cell_slot=cell_slot,
                 instance_slots=np.array([slot[v.idx] for v in self.instance], np.uint32), image_bytes=self.input_bytes)
        if field:
            a.update(phase_level_start=np.array(phase_level_start, np.uint32), advice_phase=np.array(self.advice_phase, np.uint8),
                     challenge_phase=np.array(t.challenge_phase, np.uint8))
        return a

    def column_ints(self, data, challenges=()):
        """[n_advice][n] canonical integers (an unassigned cell is 0), and the instance values"""
        v = self.tape.run(data, challenges)
        cols = [[0] * self.n for _ in range(self.n_advice)]
        for (c, r), val in self.cells.items():
            cols[c][r] = v[val.idx] % R
        return cols, [v[val.idx] % R for val in self.instance]

    def columns(self, data, challenges=()):
        """uint64[n_advice, n, 4], Montgomery limbs: what Phased.full_advice returns"""
        cols, _ = self.column_ints(data, challenges)
        return np.stack([to_mont_array(col) for col in cols])


# ---------------------------------------------------------------------------------------------- the recorded programs
def _le_bytes(values, nbytes):
    return b"".join(int(v).to_bytes(nbytes, "little") for v in values)


class Recorded:
    """program + the circuit's private data of a witness variant as input bytes"""

    def __init__(self, pc, program, data):
        self.pc, self.program, self._data = pc, program, data

    def input(self, variant=0) -> np.ndarray:
        return np.frombuffer(self._data(variant), np.uint8).copy()


def _phase0(pc, variant):
    return pc.witness(0, [0] * len(pc.challenge_phase), variant)


def rlc(pc):
    m = pc.usable - 1
    t = Tape(2, pc.challenge_phase)
    a = [t.le(3 * r, 3) for r in range(m)]
    cells = {}
    for r in range(m):
        cells[(0, r)] = a[r]
        cells[(1, r)] = t.emit("MUL", a[r], a[r])
    c = t.chal(0)
    acc = a[0]  # acc[1] = acc[0] c + a[0] with acc[0] = 0: the value that does not depend on c, and the public one
    cells[(2, 1)] = acc
    for r in range(1, m):
        acc = t.addm(t.mulm(acc, c), a[r])
        cells[(2, r + 1)] = acc
    return Recorded(pc, Program(t, cells, [a[0]], 3, pc.cs.k, 3 * m, pc.advice_phase), lambda v: _le_bytes(_phase0(pc, v)[0][:m], 3))


def shuffle(pc):
    m = pc.usable - 1
    t = Tape(2, pc.challenge_phase)
    a = [t.le(3 * r, 3) for r in range(m)]
    b = [t.le(3 * (m + r), 3) for r in range(m)]
    cells = {(0, r): a[r] for r in range(m)}
    cells.update({(1, r): b[r] for r in range(m)})
    c = t.chal(0)
    z = t.const(1)
    cells[(2, 0)] = z
    for r in range(m):
        z = t.mulm(t.mulm(z, t.addm(a[r], c)), t.invm(t.addm(b[r], c)))
        cells[(2, r + 1)] = z

    def data(v):
        w = _phase0(pc, v)
        return _le_bytes(w[0][:m], 3) + _le_bytes(w[1][:m], 3)

    return Recorded(pc, Program(t, cells, [], 3, pc.cs.k, 6 * m, pc.advice_phase), data)


def interleaved(pc):
    m = pc.usable - 1
    t = Tape(2, pc.challenge_phase)
    u = [t.le(4 * r, 4) for r in range(m + 1)]
    cells = {(1, r): u[r] for r in range(m + 1)}
    c = t.chal(0)
    s = {r: t.addm(u[r - 1], c) for r in range(1, m + 1)}
    cells.update({(0, r): s[r] for r in s})
    cells.update({(2, r): t.mulm(s[r + 1], u[r]) for r in range(1, m)})
    return Recorded(pc, Program(t, cells, [], 3, pc.cs.k, 4 * (m + 1), pc.advice_phase), lambda v: _le_bytes(_phase0(pc, v)[1][:m + 1], 4))


def three_phase(pc):
    m = pc.usable - 1
    t = Tape(3, pc.challenge_phase)
    a = [t.byte(r) for r in range(m)]
    cells = {(0, r): a[r] for r in range(m)}
    c0, c1, c2 = t.chal(0), t.chal(1), t.chal(2)
    for r in range(m):
        d = t.addm(t.mulm(a[r], c0), c1)
        cells[(1, r)] = d
        cells[(2, r)] = t.mulm(d, c2)
    return Recorded(pc, Program(t, cells, [a[0]], 3, pc.cs.k, m, pc.advice_phase), lambda v: _le_bytes(_phase0(pc, v)[0][:m], 1))


def gates_only_challenge(pc):
    m = pc.usable - 1
    t = Tape(1, pc.challenge_phase)
    a = [t.le(3 * r, 3) for r in range(m)]
    cells = {(0, r): a[r] for r in range(m)}
    cells.update({(1, r): t.emit("MUL", a[r], a[r]) for r in range(m)})
    return Recorded(pc, Program(t, cells, [], 2, pc.cs.k, 3 * m, pc.advice_phase), lambda v: _le_bytes(_phase0(pc, v)[0][:m], 3))


def shuffle_plain(pc):
    """shuffle_circuits.plain: a shuffle ARGUMENT, one phase, no challenge -- the witness is the input itself"""
    u = pc.usable
    t = Tape(1, [])
    cells = {(0, r): t.byte(r) for r in range(u)}
    cells.update({(1, r): t.byte(u + r) for r in range(u)})

    def data(v):
        w = _phase0(pc, v)
        return _le_bytes(w[0][:u], 1) + _le_bytes(w[1][:u], 1)

    return Recorded(pc, Program(t, cells, [], 2, pc.cs.k, 2 * u, pc.advice_phase), data)


RLC_CONSTANT = 7


def rlc_integer(k=5) -> Recorded:
    """phases_circuits.rlc with the challenge replaced by a small constant: one phase, no challenge, and a witness that
    stays far below 2^256 -- an INTEGER-ONLY program (operations 0..16), what zg_witness_plan_create takes as well"""
    import phases_circuits

    pc = phases_circuits.rlc(k, constant=RLC_CONSTANT)
    m = pc.usable - 1
    t = Tape(1, [])
    a = [t.le(3 * r, 3) for r in range(m)]
    cells = {}
    for r in range(m):
        cells[(0, r)] = a[r]
        cells[(1, r)] = t.emit("MUL", a[r], a[r])
    acc = a[0]
    cells[(2, 1)] = acc
    for r in range(1, m):
        acc = t.emit("ADD", t.emit("MULI", acc, imm=RLC_CONSTANT), a[r])
        cells[(2, r + 1)] = acc
    return Recorded(pc, Program(t, cells, [a[0]], 3, pc.cs.k, 3 * m, pc.advice_phase), lambda v: _le_bytes(_phase0(pc, v)[0][:m], 3))


RECORDERS = {"rlc": rlc, "shuffle": shuffle, "interleaved": interleaved, "three_phase": three_phase,
             "gates_only_challenge": gates_only_challenge, "plain": shuffle_plain}


def circuit(name, k=5):
    import phases_circuits
    import shuffle_circuits

    return shuffle_circuits.plain(k) if name == "plain" else phases_circuits.SMALL[name](k)


def recorded(name, k=5) -> Recorded:
    return RECORDERS[name](circuit(name, k))


# ---------------------------------------------------------------------------------------------- operands at the edges
EDGE = [0, 1, R - 1, R, R + 1, 2 * R, 5 * R, 5 * R + 1, 1 << 255, (1 << 256) - 1]


def edge_program(challenge=R - 1):
    """every field operation on every edge operand (pairs for the binary ones), INVM(x) * x beside INVM(x), and CHAL of one
    challenge; one advice column shows every result.  Returns (program, [(description, Val)])."""
    t = Tape(2, [0])
    consts = []
    for v in EDGE:  # (the pool holds the integers as they are: nothing reduces them)
        t.consts.append(v)
        consts.append(t.emit("CONST", imm=len(t.consts) - 1))
    out = []
    for i, x in enumerate(consts):
        inv = t.invm(x)
        out += [(f"INVM {i}", inv), (f"INVM(x) x {i}", t.mulm(inv, x))]
        for j, y in enumerate(consts):
            out += [(f"ADDM {i} {j}", t.addm(x, y)), (f"SUBM {i} {j}", t.subm(x, y)), (f"MULM {i} {j}", t.mulm(x, y))]
    c = t.chal(0)
    out += [("CHAL", c), ("CHAL + 1", t.addm(c, consts[1])), ("CHAL^-1", t.invm(c))]
    k = (len(out) - 1).bit_length()
    prog = Program(t, {(0, r): v for r, (_, v) in enumerate(out)}, [], 1, k, 1, [1])
    return prog, out
