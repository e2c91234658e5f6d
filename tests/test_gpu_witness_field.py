"""The witness program with field operations, challenges and advice phases on the device (zg_witness_plan_create_field,
zg_witness_run_field_dev, zg_prover_prove_inputs / _inputs_circuits, zg_prover_check_inputs).

References, all of them independent of the new kernels: the Python-integer interpreter of tests/field_tape.py (held against
the circuits' own witness by tests/test_field_tape_host.py), zg_prover_prove_phased / _circuits_phased with the Python
callback of tests/phases_circuits.py, and tests/proof_ref.py as the judge of the proofs.  Everything is bit-exact: no
tolerances.  Circuits at k = 5, the operation tests at k = 7."""
import ctypes
import random

import numpy as np
import pytest
import torch  # noqa: F401 -- before the first HIP call of the process (tests/conftest.py)

import field_tape
import proof_ref
from circuit import R
from field_tape import NO_SLOT, OP
from shuffle_circuits import BAD

pytestmark = pytest.mark.gpu

GWC, SHPLONK, EVM, BLAKE2B = 0, 1, 0, 1
INVALID_ARG, UNSUPPORTED = -1, -4
PHASED = ["rlc", "shuffle", "interleaved", "three_phase"]
ALL = PHASED + ["gates_only_challenge", "plain"]
VARIANTS = [0, 1, 2]


def _d2h(ptr: int, nbytes: int) -> np.ndarray:
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.zeros(nbytes // 8, np.uint64)
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0
    return out


def _mont(zg, ints):
    """[count][n_challenges] canonical integers -> uint64[count, n_challenges, 4], or None without challenges"""
    if not ints or not ints[0]:
        return None
    return np.stack([np.stack([zg.fr_from_int(c) for c in row]) for row in ints])


def _run(zg, plan, prog, inputs, challenges):
    """run_field into fresh buffers (stale contents must go): uint64[count, n_advice, n, 4] and the instance values"""
    bufs = [torch.full((prog.n_advice * prog.n * 4,), -1, dtype=torch.int64, device="cuda") for _ in inputs]
    inst = plan.run_field(np.stack(inputs), [b.data_ptr() for b in bufs], _mont(zg, challenges))
    return np.stack([_d2h(b.data_ptr(), prog.n_advice * prog.n * 32).reshape(prog.n_advice, prog.n, 4) for b in bufs]), inst


@pytest.fixture(params=[-1, 0, 3], ids=["lds", "hbm-only", "lds-3KB"])
def lds_form(request, zg):
    """ZG_WITNESS_LDS as tests/test_gpu_witness.py sets it: the default, every operand in HBM, and a 3-KB cell budget"""
    zg.tuning_set("ZG_WITNESS_LDS", request.param)
    yield request.param
    zg.tuning_set("ZG_WITNESS_LDS", -1)


class Setup:
    """prover + verifier (phases and shuffles told) + the reference's key + the recorded program's plan"""

    def __init__(self, orc, zg, ctx, name, batch=3, seed=0xABCDEF, vk=0x1234567):
        self.rec = field_tape.recorded(name)
        self.pc, self.prog = self.rec.pc, self.rec.program
        pc = self.pc
        self.img = pc.cs.to_c()
        self.shuffles = getattr(self.img, "shuffles", None)
        self.params = orc.params_new(pc.cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        fixed, sigma = pc.fixed_values(), pc.sigma_values()
        self.prover = zg.Prover(ctx, self.img, fixed, sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr, shuffles=self.shuffles)
        fc, sc = self.prover.vk_commitments()
        self.verifier = zg.Verifier(ctx, self.img, fc, sc, self.params.g_np()[0], np.array(self.params.g2, np.uint64),
                                    np.array(self.params.s_g2, np.uint64), self.vk_repr, shuffles=self.shuffles)
        for obj in (self.prover, self.verifier):
            obj.set_phases(pc.advice_phase, pc.challenge_phase)
        self.prover.set_batch(batch)
        self.vk = proof_ref.Vk(pc.cs, self.params, fixed, sigma, self.vk_repr)
        self.plan = zg.WitnessPlan(ctx, self.prog.arrays())

    def inputs(self, variants):
        return np.stack([self.rec.input(v) for v in variants])

    def insts(self, variants):
        return [self.pc.instance(v) for v in variants]

    def reference_proofs(self, variants, seeds, prover=None):
        """the host pass the entries replace: prove_phased with the Python callback (prove_batch for a one-phase circuit)"""
        p = prover or self.prover
        if self.pc.n_phases > 1:
            proofs, st = p.prove_phased(self.pc.synthesize(variants), self.insts(variants), seeds)
            assert st == 0
            return proofs
        adv = [self.pc.full_advice([0] * len(self.pc.challenge_phase), v) for v in variants]
        proofs, sts = p.prove_batch(adv, self.insts(variants), seeds)
        assert all(s == 0 for s in sts)
        return proofs

    def ref(self, proof, variant, scheme=GWC, transcript=EVM):
        return proof_ref.verify(self.vk, [self.pc.instance(variant)], proof, advice_phase=self.pc.advice_phase,
                                challenge_phase=self.pc.challenge_phase, scheme=scheme, transcript=transcript)

    def close(self):
        self.plan.close()
        self.verifier.close()
        self.prover.close()


# ---------------------------------------------------------------------------------------------- 1. the operations
def test_each_field_operation_on_edge_operands(ctx, zg):
    prog, out = field_tape.edge_program()
    plan = zg.WitnessPlan(ctx, prog.arrays())
    assert plan.info()["lanes"] > 0
    data = np.zeros(1, np.uint8)
    got, _ = _run(zg, plan, prog, [data], [[R - 1]])
    v = prog.tape.run(data, [R - 1])
    values = {}
    for r, (what, val) in enumerate(out):
        values[what] = zg.fr_to_int(got[0, 0, r])
        assert values[what] == v[val.idx], what
    assert not got[0, 0, len(out):].any()
    E = field_tape.EDGE
    for i, x in enumerate(E):  # (said once more without the interpreter)
        assert values[f"INVM {i}"] == (0 if x % R == 0 else pow(x, -1, R))
        assert values[f"INVM(x) x {i}"] == (0 if x % R == 0 else 1)
        for j, y in enumerate(E):
            assert values[f"MULM {i} {j}"] == (x % R) * (y % R) % R
    assert values["CHAL"] == R - 1 and values["CHAL + 1"] == 0
    plan.close()


# ---------------------------------------------------------------------------------------------- 2. a random DAG
def _random_dag():
    """60 generations of 16 operations over three phases, integer and field operations mixed, operands mostly from the
    generation before and some from far back; nine columns of 2^7 rows, column 3 p + i showing the slots of phase p."""
    rnd = random.Random(2424)
    t = field_tape.Tape(3, [0, 0, 1])

    def raw_const(v, phase=0):
        t.consts.append(v)
        return t.emit("CONST", imm=len(t.consts) - 1, phase=phase)

    t.table = [rnd.getrandbits(64) for _ in range(64)]
    gens = [[t.byte(i) for i in range(8)] + [raw_const(rnd.getrandbits(b)) for b in (1, 20, 63, 64, 65, 128, 200, 254, 256)]
            + [raw_const(v) for v in (0, 1, R - 1, R, R + 1, (1 << 256) - 1)]]
    for g in range(60):
        phase = g // 20
        chals = [j for j, ph in enumerate(t.challenge_phase) if ph < phase]
        cur = []
        for _ in range(16):
            src = gens[-1] if rnd.random() < 0.7 else gens[rnd.randrange(len(gens))]
            a, b = rnd.choice(src), rnd.choice(gens[rnd.randrange(len(gens))])
            kind = rnd.randrange(16)
            if kind == 0: r = t.emit("ADD", a, b, phase=phase)
            elif kind == 1: r = t.emit("SUB", a, b, phase=phase)  # (wraps modulo 2^256 when b > a)
            elif kind == 2: r = t.emit("MUL", a, b, phase=phase)
            elif kind == 3: r = t.emit("ADDI", a, imm=rnd.getrandbits(rnd.choice((3, 30, 64))), phase=phase)
            elif kind == 4: r = t.emit("MULI", a, imm=rnd.getrandbits(rnd.choice((2, 16, 40))), phase=phase)
            elif kind == 5: r = t.emit("SHRI", a, imm=rnd.choice((0, 1, 13, 64, 100, 192, 255)), phase=phase)
            elif kind == 6: r = t.emit("SHLI", a, imm=rnd.choice((0, 1, 5, 40, 70, 190)), phase=phase)
            elif kind == 7: r = t.emit("ANDI", a, imm=rnd.getrandbits(rnd.choice((1, 8, 32, 64))), phase=phase)
            elif kind == 8: r = t.emit("TABLE", t.emit("ANDI", a, imm=127, phase=phase), imm=rnd.randrange(32))  # (both sides of the bound)
            elif kind == 9: r = t.emit("DIVI", a, imm=rnd.getrandbits(rnd.choice((3, 20, 53))) | 1, phase=phase)
            elif kind == 10: r = t.emit("ADDM", a, b, phase=phase)
            elif kind == 11: r = t.emit("SUBM", a, b, phase=phase)
            elif kind in (12, 13): r = t.emit("MULM", a, b, phase=phase)
            elif kind == 14: r = t.emit("INVM", a, phase=phase)
            elif chals: r = t.emit("MULM", a, t.chal(rnd.choice(chals)))
            else: r = t.emit("GTI", a, imm=rnd.getrandbits(20), phase=phase)
            cur.append(r)
        gens.append(cur)
    k, cells, used = 7, {}, [0, 0, 0]
    shown = [v for g in gens for v in g]
    for v in shown:
        ph = t.ops[v.idx][4]
        cells[(3 * ph + used[ph] // 128, used[ph] % 128)] = v
        used[ph] += 1
    assert max(used) <= 3 * 128
    prog = field_tape.Program(t, cells, [gens[0][0], gens[10][3]], 9, k, 8, [0] * 3 + [1] * 3 + [2] * 3)
    return prog, shown


def test_random_dag_over_three_phases(ctx, zg, lds_form):
    prog, shown = _random_dag()
    arrays = prog.arrays()
    assert len(arrays["level_start"]) - 1 >= 40 and all(arrays["phase_level_start"][i] < arrays["phase_level_start"][i + 1] for i in range(3))
    plan = zg.WitnessPlan(ctx, arrays)
    info = plan.info()
    n_field = sum(1 for op in prog.tape.ops if op[0] in field_tape.OPS[17:])
    assert n_field > 200 and (lds_form == 0 or info["wide_values"] >= n_field)  # a field result may exceed 64 bits: [0, r - 1]
    if lds_form == 0:    # every operand in HBM, no allocation made: witness_run_field_kernel
        assert info["lds_bytes"] == 0 and info["values_in_lds"] == 0 and info["hbm_levels"] == info["levels"]
    elif lds_form == -1:  # every value read in its own phase has a cell; the levels that read an earlier phase's slots wait for HBM
        assert 0 < info["lds_bytes"] <= 160 * 1024 and info["values_in_hbm"] == 0 and info["values_in_lds"] > 300
        assert info["wide_cells"] > 0 and info["narrow_cells"] > 0 and 0 < info["hbm_levels"] < info["levels"]
        assert info["narrow_cells"] + info["wide_cells"] < info["values_in_lds"]  # cells are recycled
    else:                 # 3 KB of cells: spills, field results among them
        assert 0 < info["lds_bytes"] and info["values_in_lds"] > 0 and info["values_in_hbm"] > 0
        assert 32 * info["wide_cells"] + 8 * info["narrow_cells"] <= 3 * 1024
    rnd = random.Random(7)
    inputs = [np.zeros(8, np.uint8), np.full(8, 255, np.uint8), np.array([rnd.randrange(256) for _ in range(8)], np.uint8)]
    challenges = [[rnd.randrange(R) for _ in range(3)] for _ in inputs]  # (they differ per input)
    challenges[1][0] = R - 1
    got, inst = _run(zg, plan, prog, inputs, challenges)
    for b, data in enumerate(inputs):
        v = prog.tape.run(data, challenges[b])
        for (c, r), val in prog.cells.items():
            assert zg.fr_to_int(got[b, c, r]) == v[val.idx] % R, f"input {b}: {prog.tape.ops[val.idx][:4]} in phase {prog.tape.ops[val.idx][4]}"
        assert [zg.fr_to_int(x) for x in inst[b]] == [v[val.idx] % R for val in prog.instance]
    free = np.ones((9, 128), bool)
    for (c, r) in prog.cells:
        free[c, r] = False
    assert not got[:, free].any()  # an unassigned cell is zero
    plan.close()


# ---------------------------------------------------------------------------------------------- 3. columns == full_advice
@pytest.mark.parametrize("name", ALL)
def test_run_field_writes_the_circuits_witness(ctx, zg, name):
    rec = field_tape.recorded(name)
    pc, prog = rec.pc, rec.program
    plan = zg.WitnessPlan(ctx, prog.arrays())
    assert (plan.n_advice, plan.k, plan.n_challenges) == (pc.cs.n_advice, pc.cs.k, len(pc.challenge_phase))
    inputs = [rec.input(v) for v in VARIANTS]
    rnd = random.Random(33)
    for _ in range(2):
        challenges = [[rnd.randrange(R) for _ in pc.challenge_phase] for _ in VARIANTS]
        got, inst = _run(zg, plan, prog, inputs, challenges)
        for b, variant in enumerate(VARIANTS):
            assert np.array_equal(got[b], pc.full_advice(challenges[b], variant)), (name, variant)
            if pc.cs.n_instance:
                assert np.array_equal(inst[b], pc.instance(variant)[0])
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. input -> proofs
@pytest.mark.parametrize("name", ALL)
def test_prove_inputs_gives_the_bytes_of_the_host_pass(ctx, zg, orc, name):
    s = Setup(orc, zg, ctx, name)
    seeds = [11, 12, 13]
    want = s.reference_proofs(VARIANTS, seeds)
    got, outputs, sts = s.prover.prove_inputs(s.plan, s.inputs(VARIANTS), seeds)
    assert sts == [0, 0, 0] and got == want
    for b, v in enumerate(VARIANTS):
        assert len(got[b]) == proof_ref.proof_len(s.pc.cs)
        assert s.ref(got[b], v).verdict == 1
        if s.pc.cs.n_instance:
            assert np.array_equal(outputs[b], s.pc.instance(v)[0])
    assert s.verifier.verify(got, s.insts(VARIANTS), 0xFEED) == [1, 1, 1]
    assert s.prover.prove_inputs(s.plan, s.inputs(VARIANTS), seeds)[0] == want  # the same keys, the same bytes
    one, _, _ = s.prover.prove_inputs(s.plan, s.inputs([2]), [13])               # a batch is its single calls
    assert one == want[2:]
    s.close()


@pytest.mark.parametrize("name", ["rlc", "shuffle"])
def test_prove_inputs_under_shplonk_and_blake2b_and_on_a_fork(ctx, zg, orc, name):
    s = Setup(orc, zg, ctx, name)
    for obj in (s.prover, s.verifier):
        obj.set_multiopen(SHPLONK)
        obj.set_transcript(BLAKE2B)
    seeds = [21, 22, 23]
    want = s.reference_proofs(VARIANTS, seeds)
    got, _, sts = s.prover.prove_inputs(s.plan, s.inputs(VARIANTS), seeds)
    assert sts == [0, 0, 0] and got == want
    assert all(s.ref(got[b], v, SHPLONK, BLAKE2B).verdict == 1 for b, v in enumerate(VARIANTS))
    assert s.verifier.verify(got, s.insts(VARIANTS), 1) == [1, 1, 1]
    for overlap in (False, True):  # both scheduling forms
        s.prover.set_overlap(overlap)
        assert s.prover.prove_inputs(s.plan, s.inputs(VARIANTS), seeds)[0] == want
    child_ctx = zg.Ctx(0)
    child = s.prover.fork(child_ctx)  # (the plan stays on the parent's context: another stream)
    assert child.prove_inputs(s.plan, s.inputs(VARIANTS), seeds)[0] == want
    child.close()
    child_ctx.close()
    s.close()


# ---------------------------------------------------------------------------------------------- 5. N inputs, one proof
@pytest.mark.parametrize("name", ["rlc", "shuffle", "three_phase"])
def test_prove_inputs_circuits_gives_the_bytes_of_the_host_pass(ctx, zg, orc, name):
    s = Setup(orc, zg, ctx, name)
    seeds = [31, 32, 33]
    want, st = s.prover.prove_circuits_phased(s.pc.synthesize(VARIANTS), s.insts(VARIANTS), seeds)
    assert st == 0 and len(want) == proof_ref.proof_len(s.pc.cs, 3)
    got, outputs = s.prover.prove_inputs_circuits(s.plan, s.inputs(VARIANTS), seeds)
    assert got == want
    if s.pc.cs.n_instance:
        assert all(np.array_equal(outputs[b], s.pc.instance(v)[0]) for b, v in enumerate(VARIANTS))
    assert s.verifier.verify_circuits([got], [s.insts(VARIANTS)], 0xFEED, 3) == [1]
    one, _ = s.prover.prove_inputs_circuits(s.plan, s.inputs([1]), [7])  # one circuit: the single proof
    assert [one] == s.reference_proofs([1], [7])
    s.close()


# ---------------------------------------------------------------------------------------------- 6. an integer-only plan
def test_integer_only_plan_is_prove_images(ctx, zg, orc):
    rec = field_tape.rlc_integer()
    pc, prog = rec.pc, rec.program
    assert pc.n_phases == 1 and not pc.challenge_phase and all(op[0] in field_tape.OPS[:17] for op in prog.tape.ops)
    img = pc.cs.to_c()
    params = orc.params_new(pc.cs.k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x1234567)
    fixed, sigma = pc.fixed_values(), pc.sigma_values()
    prover = zg.Prover(ctx, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr)
    prover.set_batch(3)
    old = zg.WitnessPlan(ctx, prog.arrays(field=False))  # zg_witness_plan_create
    new = zg.WitnessPlan(ctx, prog.arrays())             # zg_witness_plan_create_field, the same arrays
    assert new.info() == old.info()
    inputs, seeds = np.stack([rec.input(v) for v in VARIANTS]), [41, 42, 43]
    want, want_out, sts = prover.prove_images(old, inputs, seeds)
    assert sts == [0, 0, 0]
    ref, _ = prover.prove_batch([pc.full_advice([], v) for v in VARIANTS], [pc.instance(v) for v in VARIANTS], seeds)
    assert want == ref
    launches = {}
    for plan in (old, new):
        ctx.profile(True)
        try:
            ctx.profile_collect()
            got, out, sts = prover.prove_inputs(plan, inputs, seeds)
            launches[plan] = {k: v[0] for k, v in ctx.profile_collect().items()}
        finally:
            ctx.profile(False)
        assert sts == [0, 0, 0] and got == want and np.array_equal(out, want_out)
    ctx.profile(True)
    try:
        ctx.profile_collect()
        prover.prove_images(old, inputs, seeds)
        images_launches = {k: v[0] for k, v in ctx.profile_collect().items()}
    finally:
        ctx.profile(False)
    assert launches[old] == launches[new] == images_launches and "witness_run_field" not in images_launches
    got, out = prover.prove_inputs_circuits(new, inputs, seeds)
    want_multi, want_multi_out = prover.prove_images_multi(old, inputs, seeds)
    assert got == want_multi and np.array_equal(out, want_multi_out)
    old.close()
    new.close()
    prover.close()


def test_tiny_model_plan_through_the_new_constructor(ctx, zg, orc):
    """zero_g's tiny model: 20 000 operations with table reads, wide and narrow cells and, under a 3-KB budget, spills --
    the same arrays through zg_witness_plan_create_field are laid out as zg_witness_plan_create lays them out in every
    ZG_WITNESS_LDS form, and prove_inputs gives prove_images' bytes from its launches."""
    import witness_tape
    import wnn_circuit
    import wnn_model

    k, name = wnn_model.MNIST_TINY
    wnn = wnn_model.load_checked_in(name)
    real = wnn_model.load_test_image()
    cs, asg, ilen, scores = wnn_circuit.build(wnn, real, k)
    arrays = witness_tape.trace(wnn, k).arrays()
    n_levels = len(arrays["level_start"]) - 1
    as_field = dict(arrays, phase_level_start=np.array([0, n_levels], np.uint32), advice_phase=np.zeros(cs.n_advice, np.uint8),
                    challenge_phase=np.zeros(0, np.uint8))
    plans = {}
    try:
        for knob in (0, 3, -1):
            zg.tuning_set("ZG_WITNESS_LDS", knob)
            for p in plans.values():
                p.close()
            plans = {"old": zg.WitnessPlan(ctx, arrays), "new": zg.WitnessPlan(ctx, as_field)}
            assert plans["new"].info() == plans["old"].info(), knob
            assert (plans["old"].info()["values_in_hbm"] > 0) == (knob == 3) and (plans["old"].info()["lds_bytes"] > 0) == (knob != 0)
    finally:
        zg.tuning_set("ZG_WITNESS_LDS", -1)
    params = orc.params_new(k, 0x5EED)
    prover = zg.Prover(ctx, cs.to_c(), asg.fixed_values(), asg.sigma_values(), params.g_np(), params.g_lagrange_np(), orc.fr_from_int(0xC0FFEE))
    prover.set_batch(2)
    prover.set_overlap(False)
    images = np.stack([real, np.random.default_rng(3).integers(0, 256, size=real.shape, dtype=real.dtype)])
    seeds = [51, 52]
    want, want_out, sts = prover.prove_images(plans["old"], images, seeds)
    assert sts == [0, 0] and [zg.fr_to_int(x) for x in want_out[0]] == scores
    launches = {}
    for which in ("old", "new", "images"):
        ctx.profile(True)
        try:
            ctx.profile_collect()
            got, out, sts = (prover.prove_images(plans["old"], images, seeds) if which == "images" else prover.prove_inputs(plans[which], images, seeds))
            launches[which] = {kn: v[0] for kn, v in ctx.profile_collect().items()}
        finally:
            ctx.profile(False)
        assert sts == [0, 0] and got == want and np.array_equal(out, want_out), which
    assert launches["old"] == launches["new"] == launches["images"] and "witness_run_field" not in launches["new"]
    for p in plans.values():
        p.close()
    prover.close()


# ---------------------------------------------------------------------------------------------- 7. input -> check
def test_check_inputs(ctx, zg, orc):
    s = Setup(orc, zg, ctx, "plain")  # a shuffle ARGUMENT: the check's fourth kind
    reports, _ = s.prover.check_inputs(s.plan, s.inputs(VARIANTS))
    assert [t for t, _ in reports] == [[0, 0, 0, 0]] * 3
    # the input of the spoiled variant: one value of the shuffle column changed
    spoiled = np.stack([s.rec.input(0), s.rec.input(BAD)])
    assert (spoiled[0] != spoiled[1]).sum() == 1
    got, _ = s.prover.check_inputs(s.plan, spoiled, cap=16)
    want = s.prover.check_circuit([s.pc.full_advice([], 0), s.pc.full_advice([], BAD)], s.insts([0, BAD]), None, cap=16)
    assert got == want and got[0][0] == [0, 0, 0, 0] and got[1][0][3] > 0 and got[1][0][:3] == [0, 0, 0]
    s.close()
    # a circuit with phases: the honest inputs pass for ANY challenge values, and a wrong input fails its gates
    s = Setup(orc, zg, ctx, "shuffle")
    rnd = random.Random(77)
    challenges = [[rnd.randrange(R)] for _ in VARIANTS]
    reports, _ = s.prover.check_inputs(s.plan, s.inputs(VARIANTS), _mont(zg, challenges))
    assert [t for t, _ in reports] == [[0, 0, 0, 0]] * 3
    bad = s.inputs(VARIANTS)
    bad[1, 0] ^= 1  # a[0] of input 1: b is no permutation of a any more, the product does not close
    got, _ = s.prover.check_inputs(s.plan, bad, _mont(zg, challenges))
    cols = [s.prog.columns(bad[b], challenges[b]) for b in range(3)]
    want = s.prover.check_circuit(cols, s.insts(VARIANTS), _mont(zg, challenges))
    assert got == want and got[0][0] == got[2][0] == [0, 0, 0, 0] and got[1][0][0] > 0
    s.close()


# ---------------------------------------------------------------------------------------------- 8. refusals
def _refused(zg, fn, status=INVALID_ARG):
    with pytest.raises(zg.ZgError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    return str(e.value)


def test_plan_creation_refuses_what_it_can_see(ctx, zg):
    def arrays(**over):
        # PIXEL 0 | CHAL 0 | ADDM s0 s1 | MULM s2 s1 -- one level each, phase 0 = level 0, phase 1 = levels 1..3; column 0 in phase 0, column 1 in phase 1
        a = dict(ops=np.array([[OP["PIXEL"], 0, 0, 0], [OP["CHAL"], 0, 0, 0], [OP["ADDM"], 0, 1, 0], [OP["MULM"], 2, 1, 0]], np.uint64),
                 level_start=np.array([0, 1, 2, 3, 4], np.uint32), consts=np.zeros((1, 4), np.uint64), table=np.zeros(1, np.uint64),
                 cell_slot=np.array([[0, NO_SLOT], [3, 2]], np.uint32), instance_slots=np.array([0], np.uint32), image_bytes=1,
                 phase_level_start=np.array([0, 1, 4], np.uint32), advice_phase=np.array([0, 1], np.uint8), challenge_phase=np.array([0], np.uint8))
        a.update(over)
        return a

    ok = zg.WitnessPlan(ctx, arrays())
    bufs = torch.zeros(2 * 2 * 4, dtype=torch.int64, device="cuda")
    inst = ok.run_field(np.array([[9]], np.uint8), [bufs.data_ptr()], np.stack([[zg.fr_from_int(5)]]))
    got = _d2h(bufs.data_ptr(), 2 * 2 * 32).reshape(2, 2, 4)
    assert zg.fr_to_int(inst[0, 0]) == 9 and [zg.fr_to_int(x) for x in got.reshape(4, 4)] == [9, 0, 70, 14]
    _refused(zg, lambda: ok.run_field(np.array([[9]], np.uint8), [bufs.data_ptr()], None))  # the plan has a challenge
    _refused(zg, lambda: ok.run(np.array([[9]], np.uint8), [bufs.data_ptr()]))
    ok.close()
    ops = arrays()["ops"]

    def with_op(i, row):
        o = ops.copy()
        o[i] = row
        return o

    bad = [
        dict(ops=with_op(3, [22, 2, 1, 0])),                                   # an unknown opcode
        dict(ops=with_op(1, [OP["CHAL"], 0, 0, 1])),                           # challenge 1 of 1
        dict(challenge_phase=np.array([1], np.uint8)),                         # CHAL in phase 1 of a challenge squeezed behind phase 1
        dict(phase_level_start=np.array([0, 2, 4], np.uint32)),                # ... or standing in phase 0 (level 1 now belongs to it)
        dict(cell_slot=np.array([[2, NO_SLOT], [3, 2]], np.uint32)),           # a phase-0 column showing a phase-1 slot
        dict(instance_slots=np.array([2], np.uint32)),                         # an instance slot outside phase 0
        dict(phase_level_start=np.array([0, 5, 4], np.uint32)),                # phase bounds that descend
        dict(phase_level_start=np.array([0, 1, 3], np.uint32)),                # ... that do not cover the levels
        dict(phase_level_start=np.array([1, 1, 4], np.uint32)),                # ... that do not start at level 0
        dict(phase_level_start=np.array([0, 1, 2, 3, 4], np.uint32)),          # four phases
        dict(advice_phase=np.array([0, 2], np.uint8)),                         # a column in a phase the plan has not
        dict(ops=with_op(2, [OP["ADDM"], 0, 3, 0])),                           # an operand of a later level (b of a field operation)
        dict(ops=with_op(3, [OP["INVM"], 3, 0, 0])),                           # ... its own slot
    ]
    for over in bad:
        _refused(zg, lambda: zg.WitnessPlan(ctx, arrays(**over)))
    # zg_witness_plan_create itself keeps refusing the new opcodes
    plain = {k: v for k, v in arrays(ops=np.array([[OP["PIXEL"], 0, 0, 0], [OP["ADDM"], 0, 0, 0]], np.uint64), level_start=np.array([0, 1, 2], np.uint32),
                                     cell_slot=np.full((2, 2), NO_SLOT, np.uint32)).items() if not k.endswith("phase") and k != "phase_level_start"}
    _refused(zg, lambda: zg.WitnessPlan(ctx, plain))
    one_phase = dict(plain, phase_level_start=np.array([0, 2], np.uint32), advice_phase=np.array([0, 0], np.uint8), challenge_phase=np.zeros(0, np.uint8))
    p = zg.WitnessPlan(ctx, one_phase)  # (the same arrays through the new constructor: a field plan of one phase)
    assert p.info()["lds_bytes"] > 0 and p.info()["wide_values"] == 1  # (the LDS form: ADDM's result is wide)
    p.close()


def test_entries_refuse_and_leave_the_prover_working(ctx, zg, orc):
    s = Setup(orc, zg, ctx, "rlc", batch=2)
    seeds = [9, 10]
    want = s.reference_proofs([0, 1], seeds)
    good = lambda: s.prover.prove_inputs(s.plan, s.inputs([0, 1]), seeds)[0] == want  # noqa: E731
    assert good()
    slot_before = _d2h(s.prover.advice_slot(0), 3 * 32 * 32)
    other = {name: zg.WitnessPlan(ctx, field_tape.recorded(name).program.arrays()) for name in ("interleaved", "three_phase", "gates_only_challenge")}
    k6 = zg.WitnessPlan(ctx, field_tape.recorded("rlc", 6).program.arrays())
    inputs = lambda plan, count: np.zeros((count, plan.image_bytes), np.uint8)  # noqa: E731
    chal = np.zeros((2, 1, 4), np.uint64)
    for plan in list(other.values()) + [k6]:  # other advice phases | more challenges and phases | fewer columns and phases | another k
        for fn in (lambda: s.prover.prove_inputs(plan, inputs(plan, 2), seeds), lambda: s.prover.prove_inputs_circuits(plan, inputs(plan, 2), seeds),
                   lambda: s.prover.check_inputs(plan, inputs(plan, 2), np.zeros((2, plan.n_challenges, 4), np.uint64))):
            _refused(zg, fn)
    assert np.array_equal(_d2h(s.prover.advice_slot(0), 3 * 32 * 32), slot_before)  # nothing was written
    assert good()
    # more inputs than slots; challenges missing; a prover that was never told the phases
    _refused(zg, lambda: s.prover.prove_inputs(s.plan, s.inputs([0, 1, 2]), [1, 2, 3]))
    _refused(zg, lambda: s.prover.prove_inputs_circuits(s.plan, s.inputs([0, 1, 2]), [1, 2, 3]))
    _refused(zg, lambda: s.prover.check_inputs(s.plan, s.inputs([0, 1]), None))
    assert s.prover.check_inputs(s.plan, s.inputs([0, 1]), chal)[0] == [([0, 0, 0, 0], [])] * 2
    assert good()
    # a proof buffer below zg_prover_proof_size on the phased ride; more than 64 inputs in a call
    cap = s.prover.proof_cap
    s.prover.proof_cap = cap - 1
    assert "zg_prover_proof_size" in _refused(zg, lambda: s.prover.prove_inputs(s.plan, s.inputs([0, 1]), seeds))
    s.prover.proof_cap = cap
    s.prover.set_batch(65)
    many = np.repeat(s.inputs([0]), 65, axis=0)
    assert "64 at most" in _refused(zg, lambda: s.prover.prove_inputs(s.plan, many, list(range(65))))
    assert "64 at most" in _refused(zg, lambda: s.prover.check_inputs(s.plan, many, np.zeros((65, 1, 4), np.uint64)))
    s.prover.set_batch(2)
    assert good()
    # (the point-range-shard refusal of the proving entries cannot be reached here: zg_prover_set_shard itself refuses a prover
    #  with challenges or phases -- tests/test_gpu_phases.py pins that -- so the entries' own check only guards that door)
    s.prover.set_phases([0, 0, 0], [0])
    _refused(zg, lambda: s.prover.prove_inputs(s.plan, s.inputs([0, 1]), seeds))
    s.prover.set_phases(s.pc.advice_phase, s.pc.challenge_phase)
    assert good()
    # the old entries keep refusing this circuit, whatever the plan
    assert "challenges or advice phases" in _refused(zg, lambda: s.prover.prove_images(s.plan, s.inputs([0, 1]), seeds), UNSUPPORTED)
    assert "challenges or advice phases" in _refused(zg, lambda: s.prover.check_images(s.plan, s.inputs([0, 1])), UNSUPPORTED)
    assert good() and s.verifier.verify(want, s.insts([0, 1]), 3) == [1, 1]
    for plan in list(other.values()) + [k6]:
        plan.close()
    s.close()
