"""The witness check on the device (zg_prover_check_batch / _dev / _images, csrc/check.hip): Wnn::mock_proof's question
-- is this witness satisfied, and if not, where does it fail -- answered for a batch.  Every expected report comes from
the Python big-integer enumerator of tests/check_enum.py (pinned against Assignment.check() in tests/test_check_host.py),
element for element: totals by kind and records in ascending (kind, index, row) order."""
from ctypes import c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

from check_enum import COPY, GATE, LOOKUP, advice_table_circuit, changed, wrap_circuit
from check_enum import failures as report  # (totals, records) of an assignment, by the enumerator
from circuit import ADVICE, INSTANCE
from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu

CLEAN = ([0, 0, 0], [])


class Setup:
    def __init__(self, orc, zg, ctx, cs, asg, ilen, seed=0xABCDEF, vk=0x1234567, sigma=None, verifier=False):
        self.cs, self.asg, self.ilen = cs, asg, ilen
        self.img = cs.to_c()
        self.params = orc.params_new(cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        self.fixed = asg.fixed_values()
        self.sigma = asg.sigma_values() if sigma is None else sigma
        self.orc = orc
        self._pk = None
        self.prover = zg.Prover(ctx, self.img, self.fixed, self.sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr)
        self.verifier = None
        if verifier:
            fc, sc = self.prover.vk_commitments()
            self.verifier = zg.Verifier(ctx, self.img, fc, sc, self.params.g_np()[0], np.array(self.params.g2, np.uint64),
                                        np.array(self.params.s_g2, np.uint64), self.vk_repr)

    @property
    def pk(self):  # the oracle's key, made when a test compares proof bytes
        if self._pk is None:
            self._pk = self.orc.ProvingKey(self.img, self.fixed, self.sigma, self.params, self.vk_repr)
        return self._pk

    def witness(self, asg=None):
        asg = asg or self.asg
        return asg.advice_values(), asg.instance_values(self.ilen)

    def check(self, asg=None, cap=512):
        return self.prover.check(*self.witness(asg), cap=cap)

    def close(self):
        if self.verifier:
            self.verifier.close()
        self.prover.close()


_TINY = {}


def tiny_parts():
    if not _TINY:
        import wnn_circuit
        import wnn_model

        kk, name = wnn_model.MNIST_TINY
        wnn = wnn_model.load_checked_in(name)
        cs, asg, ilen, scores = wnn_circuit.build(wnn, wnn_model.load_test_image(), kk)
        _TINY.update(k=kk, wnn=wnn, cs=cs, asg=asg, ilen=ilen, scores=scores)
    return _TINY


@pytest.fixture(scope="module")
def tiny(ctx, zg, orc):
    orc.load().orc_set_threads(16)
    t = tiny_parts()
    s = Setup(orc, zg, ctx, t["cs"], t["asg"], t["ilen"], seed=0x5EED, vk=0xC0FFEE, verifier=True)
    yield s
    s.close()


# ---------------------------------------------------------------- 1. satisfied witnesses
@pytest.mark.parametrize("k", [5, 6, 10])
@pytest.mark.parametrize("kw", [{}, {"two_lookups": True}, {"force_degree": 6}], ids=["plain", "two_lookups", "degree6"])
def test_satisfied_toy_witnesses_have_no_failures(ctx, zg, orc, k, kw):
    s = Setup(orc, zg, ctx, *toy_circuit(k, **kw))
    assert s.check() == CLEAN
    s.close()


@pytest.mark.parametrize("kind", ["no_lookup", "gates_only", "wide_lookup", "advice_factor", "merged_selectors"])
def test_satisfied_variant_witnesses_have_no_failures(ctx, zg, orc, kind):
    s = Setup(orc, zg, ctx, *variant_circuit(kind, 6))
    assert s.check() == CLEAN
    s.close()


def test_satisfied_tiny_model_has_no_failures(tiny):
    assert tiny.check() == CLEAN


def test_satisfied_k15_model_has_no_failures(ctx, zg, orc):
    import wnn_circuit
    import wnn_model

    orc.load().orc_set_threads(16)
    kk, name = wnn_model.MNIST_SMALL
    cs, asg, ilen, _ = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), kk)
    s = Setup(orc, zg, ctx, cs, asg, ilen, seed=0x5EED, vk=0xC0FFEE)
    assert s.check() == CLEAN
    s.close()


# ---------------------------------------------------------------- 2. changed witnesses
def _wide_pair(asg):
    return 3 * ((asg.get(ADVICE, 0, 5) + 1) % 9) + 1  # both halves occur in the table, not as a pair


CHANGES = {
    "toy-a2r7": (lambda: toy_circuit(6), lambda a: [(ADVICE, 2, 7, lambda v: v + 1)]),
    "toy-a1r9-big": (lambda: toy_circuit(6), lambda a: [(ADVICE, 1, 9, 1 << 20)]),
    "toy-instance": (lambda: toy_circuit(6), lambda a: [(INSTANCE, 0, 0, lambda v: v + 1)]),
    "toy-fixed-copy": (lambda: toy_circuit(6), lambda a: [(ADVICE, 0, 0, lambda v: v + 12345)]),
    "toy-two-inactive": (lambda: toy_circuit(6, two_lookups=True), lambda a: [(ADVICE, 1, a.cs.usable_rows() - 1, lambda v: v + 1)]),
    "wide-pair": (lambda: variant_circuit("wide_lookup", 6), lambda a: [(ADVICE, 1, 5, _wide_pair(a))]),
    "advice_factor-r9": (lambda: variant_circuit("advice_factor", 6), lambda a: [(ADVICE, 1, 9, lambda v: v + 1)]),
    "advice_factor-off-row": (lambda: variant_circuit("advice_factor", 6), lambda a: [(ADVICE, 1, 6, lambda v: v + 1)]),
    "merged_selectors-r9": (lambda: variant_circuit("merged_selectors", 6), lambda a: [(ADVICE, 1, 9, lambda v: v + 1)]),
    "merged_selectors-off-row": (lambda: variant_circuit("merged_selectors", 6), lambda a: [(ADVICE, 1, 12, lambda v: v + 1)]),
    "no_lookup-copy": (lambda: variant_circuit("no_lookup", 6), lambda a: [(ADVICE, 1, 3, lambda v: v + 2)]),
    "wrap": (wrap_circuit, lambda a: [(ADVICE, 1, a.n - 1, 40)]),
}


@pytest.mark.parametrize("name", list(CHANGES))
def test_changed_witness_reports_equal_the_enumerator(ctx, zg, orc, name):
    make, edits = CHANGES[name]
    cs, asg, ilen = make()
    s = Setup(orc, zg, ctx, cs, asg, ilen)
    assert s.check() == CLEAN
    bad = changed(asg, edits(asg))
    want = report(cs, bad)
    got = s.check(bad)
    print(name, "expected", want, "got", got)
    assert got == want
    if name == "wrap":
        assert want == ([1, 0, 0], [(GATE, 0, 0, 0, 0)])  # the gate on row 0 read row n - 1
    if name.endswith("off-row") or name == "toy-two-inactive":
        assert want == CLEAN  # a changed cell where no constraint looks is no failure
    s.close()


def test_changed_tiny_model_reports_equal_the_enumerator(tiny):
    t = tiny_parts()
    bad = changed(t["asg"], [(ADVICE, 0, 100, lambda v: v + 1)])
    want = report(t["cs"], bad)
    got = tiny.check(bad)
    print("expected", want, "got", got)
    assert sum(want[0]) > 0 and got == want
    assert tiny.check() == CLEAN


# ---------------------------------------------------------------- 3. a table that is part of the witness
def test_lookup_into_an_advice_table_is_made_per_witness(ctx, zg, orc):
    cs, asg, ilen = advice_table_circuit(5)
    usable = cs.usable_rows()
    s = Setup(orc, zg, ctx, cs, asg, ilen)
    # witness B: another table (values 100 .. 104) and inputs that only that table holds
    other = changed(asg, [(ADVICE, 1, r, 100 + r % 5) for r in range(usable)] + [(ADVICE, 0, r, 100 + 2 * r % 5) for r in range(usable)])
    # witness C: A with one input that is in no table; witness D: B's inputs over A's table (all of them missing but 0-rows)
    miss = changed(asg, [(ADVICE, 0, 4, 99)])
    cross = changed(asg, [(ADVICE, 0, r, 100 + 2 * r % 5) for r in range(usable)])
    asgs = [asg, other, miss, cross]
    want = [report(cs, a) for a in asgs]
    assert want[0] == CLEAN and want[1] == CLEAN and want[2] == ([0, 1, 0], [(LOOKUP, 0, 4, 0, 0)]) and want[3][0][LOOKUP] == usable
    s.prover.set_batch(4)
    got = s.prover.check_batch([a.advice_values() for a in asgs], [a.instance_values(ilen) for a in asgs], cap=64)
    assert got == want
    got = s.prover.check_batch([a.advice_values() for a in reversed(asgs)], [a.instance_values(ilen) for a in asgs], cap=64)
    assert got == want[::-1]
    s.close()


# ---------------------------------------------------------------- 4. the cap
def test_cap_cuts_the_ordered_list_and_leaves_the_totals_exact(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(6)
    n = 1 << cs.k
    bad = changed(asg, [(ADVICE, c, r, (1 << 20) + r + c) for c in range(3) for r in range(n)])
    totals, recs = report(cs, bad)
    assert totals == [112, 56, 123] and len(recs) == 291
    s = Setup(orc, zg, ctx, cs, asg, ilen)
    for cap in (3, 130, 0, 291, 400):
        got_totals, got = s.check(bad, cap=cap)
        assert got_totals == totals
        assert len(got) == min(291, cap) and got == recs[:cap]
    s.close()


# ---------------------------------------------------------------- 5. batch independence, device pointers, forks
def test_every_slot_of_a_batch_reports_as_a_lone_check(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(6)
    s = Setup(orc, zg, ctx, cs, asg, ilen)
    asgs = [asg] * 8
    asgs[2] = changed(asg, [(ADVICE, 2, 7, lambda v: v + 1)])
    asgs[5] = changed(asg, [(ADVICE, 1, 9, 1 << 20)])
    want = [report(cs, a) for a in asgs]
    assert want[0] == CLEAN and want[2] != CLEAN and want[5] != CLEAN and want[2] != want[5]
    lone = [s.check(a) for a in asgs]  # (slot 0, batch of one)
    assert lone == want
    s.prover.set_batch(8)
    advs, insts = [a.advice_values() for a in asgs], [a.instance_values(ilen) for a in asgs]
    assert s.prover.check_batch(advs, insts, cap=512) == want
    # the same on the slots as they stand, and named by their device addresses
    assert s.prover.check_batch(None, insts, cap=512, device=True) == want
    assert s.prover.check_batch([s.prover.advice_slot(b) for b in range(8)], insts, cap=512, device=True) == want
    # ... from another slot's columns: slot b takes slot 7 - b's
    back = s.prover.check_batch([s.prover.advice_slot(7 - b) for b in range(4)] + [None] * 4, insts, cap=512, device=True)
    assert back[:4] == [want[0], want[0], want[5], want[0]] and back[4:] == want[4:]
    # a fork shares the key's check data (the mapping, the sorted tables)
    ctx2 = zg.Ctx(0)
    f = s.prover.fork(ctx2)
    f.set_batch(8)
    assert f.check_batch(advs, insts, cap=512) == want
    f.close()
    ctx2.close()
    s.close()


# ---------------------------------------------------------------- 6. the check does not disturb a proof
def _check_then_prove(s, orc, seed):
    adv, inst = s.witness()
    st, want, _ = orc.create_proof(s.pk, adv, inst, seed)
    assert st == 0
    alone = s.prover.prove(adv, inst, seed)
    assert alone == want
    assert s.prover.check(adv, inst) == CLEAN  # (writes the slot, as a proof would; the blinding rows are the witness's own)
    got, sts = s.prover.prove_batch(None, [inst], [seed], device=True)  # the slot as it stands
    assert sts == [0] and got[0] == want
    # ... and the slot a proof left behind (blinding rows drawn) still checks clean, and proves the same again
    assert s.prover.check_batch(None, [inst], device=True)[0] == CLEAN
    got, sts = s.prover.prove_batch(None, [inst], [seed + 1], device=True)
    assert sts == [0] and got[0] == orc.create_proof(s.pk, adv, inst, seed + 1)[1]
    assert s.verifier.verify([want, got[0]], [inst, inst], 17) == [1, 1]


def test_check_then_prove_gives_the_bytes_of_prove_alone_toy(ctx, zg, orc):
    s = Setup(orc, zg, ctx, *toy_circuit(6), verifier=True)
    _check_then_prove(s, orc, 5)
    s.close()


def test_check_then_prove_gives_the_bytes_of_prove_alone_tiny(tiny, orc):
    _check_then_prove(tiny, orc, 7)


# ---------------------------------------------------------------- 7. images
def _images():
    import wnn_model

    real = wnn_model.load_test_image()
    rng = np.random.default_rng(3)
    return [real] + [rng.integers(0, 256, size=real.shape, dtype=real.dtype) for _ in range(2)]


def test_check_images_and_wrong_outputs(ctx, zg, orc, tiny):
    import witness_tape

    t = tiny_parts()
    images = _images()
    plan = zg.WitnessPlan(ctx, witness_tape.trace(t["wnn"], t["k"]).arrays())
    tiny.prover.set_batch(3)
    reports, outputs = tiny.prover.check_images(plan, np.stack(images))
    assert reports == [CLEAN] * 3
    for im, out in zip(images, outputs):
        assert [zg.fr_to_int(x) for x in out] == t["wnn"].predict(im)
    assert [zg.fr_to_int(x) for x in outputs[0]] == t["scores"]
    # image 0 with one claimed output off by one: exactly the copy failures of that instance cell
    j = 3
    wrong = outputs.copy()
    wrong[0, j] = zg.fr_from_int(t["scores"][j] + 1)
    want = report(t["cs"], changed(t["asg"], [(INSTANCE, 0, j, lambda v: v + 1)]))
    assert want[0][GATE] == 0 and want[0][LOOKUP] == 0 and want[0][COPY] > 0
    insts = [w[None, :, :] for w in wrong]
    got = tiny.prover.check_batch(None, insts, device=True)
    print("expected", want, "got", got[0])
    assert got == [want, CLEAN, CLEAN]
    # the verifier only rejects what the check explains
    proofs, sts = tiny.prover.prove_batch(None, insts, [61, 62, 63], device=True)
    assert sts == [0, 0, 0]
    assert tiny.verifier.verify(proofs, insts, 23) == [0, 1, 1]
    plan.close()
    tiny.prover.set_batch(1)


# ---------------------------------------------------------------- 8. what the prover already detects
def test_a_witness_the_prover_refuses_has_lookup_failures(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(6)
    s = Setup(orc, zg, ctx, cs, asg, ilen)
    bad = changed(asg, [(ADVICE, 1, 9, 1 << 20)])
    adv, inst = s.witness(bad)
    _, sts = s.prover.prove_batch([adv], [inst], [1], raise_on_error=False)
    assert sts == [-5]  # ZG_ERR_CONSTRAINT
    totals, recs = s.prover.check(adv, inst)
    assert totals[LOOKUP] > 0 and (LOOKUP, 0, 9, 0, 0) in recs
    s.close()


# ---------------------------------------------------------------- 9. argument errors
def test_argument_errors_are_refused(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(5)
    s = Setup(orc, zg, ctx, cs, asg, ilen)
    adv, inst = s.witness()
    with pytest.raises(zg.ZgError) as e:
        s.prover.check_batch([adv, adv], [inst, inst])  # two witnesses, one slot
    assert e.value.status == -1
    long_inst = np.zeros((1, cs.usable_rows() + 1, 4), np.uint64)
    with pytest.raises(zg.ZgError) as e:
        s.prover.check(adv, long_inst)
    assert e.value.status == -1
    lib = ctx.lib
    adv_ptrs = (c_void_p * 1)(c_void_p(adv.ctypes.data))
    inst_ptrs = (c_void_p * 1)(c_void_p(inst.ctypes.data))
    totals = (c_uint32 * 3)()
    assert lib.zg_prover_check_batch(s.prover.h, c_size_t(1), adv_ptrs, inst_ptrs, c_size_t(ilen), None, c_size_t(4), totals) == -1
    assert lib.zg_prover_check_batch(s.prover.h, c_size_t(1), adv_ptrs, inst_ptrs, c_size_t(ilen), None, c_size_t(0), None) == -1
    assert lib.zg_prover_check_batch(s.prover.h, c_size_t(1), adv_ptrs, None, c_size_t(ilen), None, c_size_t(0), totals) == -1
    assert s.check() == CLEAN  # (nothing was left behind)
    s.close()


def test_a_key_with_a_foreign_sigma_value_cannot_be_checked_but_proves_as_before(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(5)
    sigma = asg.sigma_values().copy()
    sigma[2, 7] = zg.fr_from_int(5)
    s = Setup(orc, zg, ctx, cs, asg, ilen, sigma=sigma)
    adv, inst = s.witness()
    for _ in range(2):  # (the refusal is the key's: it does not depend on who asks first)
        with pytest.raises(zg.ZgError) as e:
            s.prover.check(adv, inst)
        assert e.value.status == -1
    st, want, _ = orc.create_proof(s.pk, adv, inst, 3)
    assert st == 0 and s.prover.prove(adv, inst, 3) == want
    s.close()


# ---------------------------------------------------------------- 10. knob invariance
def test_check_images_does_not_depend_on_the_witness_form(ctx, zg, orc, tiny):
    import witness_tape

    t = tiny_parts()
    images = np.stack(_images())
    arrays = witness_tape.trace(t["wnn"], t["k"]).arrays()
    tiny.prover.set_batch(3)
    seen = []
    try:
        for form in (0, 1):
            zg.tuning_set("ZG_WITNESS_LDS", form)
            plan = zg.WitnessPlan(ctx, arrays)
            reports, outputs = tiny.prover.check_images(plan, images)
            seen.append((reports, outputs.tobytes()))
            plan.close()
    finally:
        zg.tuning_set("ZG_WITNESS_LDS", -1)
        tiny.prover.set_batch(1)
    assert seen[0] == seen[1] and seen[0][0] == [CLEAN] * 3
