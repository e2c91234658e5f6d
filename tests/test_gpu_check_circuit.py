"""zg_prover_check_circuit / _dev on the device: the witness check for circuits with shuffles and
challenges.  Every report -- totals and records -- is compared element for element with tests/check_enum_ext.failures4,
the Python-integer enumeration (held to check_enum and proof_ref by tests/test_check_enum_ext_host.py).  Circuits:
tests/shuffle_circuits.py and tests/phases_circuits.py; witnesses: tests/check_circuit_cases.py.

Tolerances: none -- everything here is exact arithmetic mod r, counts, row numbers or bytes."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401 -- before the first HIP call of the process (tests/conftest.py)

import check_circuit_cases as cases
import phases_circuits
import shuffle_circuits
from check_enum import advice_table_circuit, changed
from check_enum import failures as failures3
from check_enum_ext import columns_of, failures4, instance_of
from circuit import ADVICE, R, to_mont_array
from shuffle_circuits import BAD

pytestmark = pytest.mark.gpu

ZG_ERR_INVALID_ARG = -1
SHUFFLE = 3
CLEAN = ([0, 0, 0, 0], [])
NEW_KERNELS = ("check_challenge_fill", "check_shuffle_eval", "check_shuffle_sort_local", "check_shuffle_sort_global",
               "check_shuffle_compare", "check_shuffle_flag")


def mont(cols):
    return np.stack([to_mont_array(c) for c in cols])


def fr(zg, values):
    return np.stack([zg.fr_from_int(v) for v in values]) if values else np.zeros((0, 4), np.uint64)


class Setup:
    def __init__(self, orc, zg, ctx, pc, batch=1):
        self.pc, self.zg = pc, zg
        self.img = pc.cs.to_c()
        self.params = orc.params_new(pc.cs.k, 0xABCDEF)
        self.prover = zg.Prover(ctx, self.img, pc.fixed_values(), pc.sigma_values(), self.params.g_np(), self.params.g_lagrange_np(),
                                orc.fr_from_int(0x1234567), shuffles=getattr(self.img, "shuffles", None) or None)
        if pc.challenge_phase or pc.n_phases > 1:
            self.prover.set_phases(pc.advice_phase, pc.challenge_phase)
        if batch > 1:
            self.prover.set_batch(batch)

    def inst(self, variant=0):
        return self.pc.instance(variant)

    def want(self, adv, challenges=(), variant=0):
        return failures4(self.pc.cs, self.pc.asg, adv, instance_of(self.pc, variant), list(challenges))

    def check(self, advs, challenges=None, cap=64, variants=None, prover=None, **kw):
        """advs: per witness its columns of integers; challenges: per witness its integers"""
        variants = variants or [0] * len(advs)
        ch = None if challenges is None else np.stack([fr(self.zg, c) for c in challenges])
        return (prover or self.prover).check_circuit([mont(a) for a in advs], [self.inst(v) for v in variants], ch, cap=cap, **kw)

    def close(self):
        self.prover.close()


def capped(report, cap):
    return report[0], report[1][:cap]


# ---------------------------------------------------------------------------------------------- the sort's sizes
@pytest.mark.parametrize("name,k", cases.SIZES)
def test_reports_equal_the_enumerator_at_every_sort_size(ctx, zg, orc, name, k):
    pc = cases.circuit(name, k)
    s = Setup(orc, zg, ctx, pc, batch=2)
    advs = [columns_of(pc, (), 1), columns_of(pc, (), BAD)]
    want = [s.want(a) for a in advs]
    assert want[0] == CLEAN and want[1][0][SHUFFLE] >= 1
    cap = sum(want[1][0]) + 5
    assert s.check(advs, cap=cap) == want
    assert s.check(advs[::-1], cap=cap) == want[::-1]
    s.close()


def test_wide_k14_with_its_high_gate(ctx, zg, orc):
    pc = cases.circuit("wide14")
    s = Setup(orc, zg, ctx, pc, batch=2)
    advs = [columns_of(pc, (), 0), columns_of(pc, (), BAD)]
    want = [s.want(a) for a in advs]
    assert want[0] == CLEAN and want[1] != CLEAN
    assert s.check(advs) == want
    s.close()


# ---------------------------------------------------------------------------------------------- adversarial columns
@pytest.fixture(scope="module")
def plain_cases():
    return cases.plain_cases()


@pytest.mark.parametrize("k", [5, 11])
def test_ties_break_by_row(ctx, zg, orc, plain_cases, k):
    pc = shuffle_circuits.plain(k)
    s = Setup(orc, zg, ctx, pc, batch=2)
    advs = [plain_cases["one_above_k%d" % k][1], plain_cases["one_below_k%d" % k][1]]
    r0 = pc.usable // 2
    want = [([0, 0, 0, 1], [(SHUFFLE, 0, pc.usable - 1, 0, r0)]), ([0, 0, 0, 1], [(SHUFFLE, 0, 0, 0, r0)])]
    assert [s.want(a) for a in advs] == want
    assert s.check(advs) == want
    s.close()


def test_chunk_edge_swap_and_single_limb_differences(ctx, zg, orc, plain_cases):
    pc = shuffle_circuits.plain(11)
    s = Setup(orc, zg, ctx, pc, batch=3)
    advs = [plain_cases[name][1] for name in ("swap_across_chunks", "top_limb", "low_limb")]
    want = [s.want(a) for a in advs]
    assert want[0] == CLEAN and want[1][0][SHUFFLE] >= 1 and want[2][0][SHUFFLE] >= 1 and want[1] != want[2]
    cap = max(sum(w[0]) for w in want) + 1
    assert s.check(advs, cap=cap) == want
    s.close()


@pytest.mark.parametrize("name,k", [("plain", 11), ("three", 5), ("rotated", 10)])
def test_rows_from_usable_on_take_no_part(ctx, zg, orc, name, k):
    pc = cases.circuit(name, k)
    s = Setup(orc, zg, ctx, pc, batch=2)
    clean = [columns_of(pc, (), 0), columns_of(pc, (), BAD)]
    dirty = [cases.garbage(pc, a) for a in clean]
    want = [s.want(a) for a in clean]
    # (rotated's expressions read a neighbour row; its selector is off where that row is no usable one)
    assert [s.want(a) for a in dirty] == want and s.check(dirty) == want
    s.close()


# ---------------------------------------------------------------------------------------------- BAD variants, other_row, caps
def raw_check(zg, prover, adv, inst, cap, fill=0xA5A5A5A5):
    """zg_prover_check_circuit itself with a pre-filled record array: (totals, all `cap` records as tuples)"""
    recs = (zg.Failure * max(1, cap))()
    ctypes.memset(recs, 0xA5, ctypes.sizeof(recs))
    totals = (ctypes.c_uint32 * 4)()
    adv = np.ascontiguousarray(adv, dtype=np.uint64)
    inst = np.ascontiguousarray(inst, dtype=np.uint64)
    ptrs = (ctypes.c_void_p * 1)(adv.ctypes.data)
    iptrs = (ctypes.c_void_p * 1)(inst.ctypes.data)
    ilen = inst.shape[1] if inst.ndim == 3 and inst.shape[0] else 0
    zg._check(prover.ctx.lib.zg_prover_check_circuit(prover.h, ctypes.c_size_t(1), ptrs, iptrs, ctypes.c_size_t(ilen), None,
                                                     recs if cap else None, ctypes.c_size_t(cap), totals))
    return [int(t) for t in totals], [recs[i].as_tuple() for i in range(cap)]


def _caps(s, zg, adv, challenges=None):
    want = s.want(adv, challenges[0] if challenges else ())
    total = sum(want[0])
    assert want[0][SHUFFLE] >= 1 and want[0][:3] == [0, 0, 0]
    assert all(rec[0] == SHUFFLE and rec[3] == 0 and rec[4] < s.pc.usable for rec in want[1])
    for cap in sorted(set(cases.CAPS) | {total, total + 5}):
        assert s.check([adv], challenges, cap=cap)[0] == capped(want, cap), cap
    return want


@pytest.mark.parametrize("name", sorted(shuffle_circuits.SMALL))
def test_bad_variants_report_exact_totals_partners_and_heads(ctx, zg, orc, name):
    pc = shuffle_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    ch = [cases.challenges_for(pc)] if pc.challenge_phase else None
    _caps(s, zg, columns_of(pc, ch[0] if ch else (), BAD), ch)
    s.close()


def test_a_cascade_is_reported_whole_and_entries_past_the_total_are_left_alone(ctx, zg, orc):
    pc, adv = cases.cascade()
    s = Setup(orc, zg, ctx, pc)
    want = _caps(s, zg, adv)
    total = sum(want[0])
    assert total > max(cases.CAPS)
    untouched = (0xA5A5A5A5,) * 5
    for cap in (1, 7, total, total + 5):
        totals, recs = raw_check(zg, s.prover, mont(adv), s.inst(), cap)
        assert totals == want[0] and recs[:total] == want[1][:cap] and all(rec == untouched for rec in recs[total:])
    s.close()


# ---------------------------------------------------------------------------------------------- mixed failures in one batch
def test_every_witness_of_a_mixed_batch_gets_its_own_report(ctx, zg, orc):
    pc, advs = cases.mixed_three()
    s = Setup(orc, zg, ctx, pc, batch=4)
    want = [s.want(a) for a in advs]
    assert want[0] == CLEAN
    assert want[1][0][:3] == [0, 0, 0] and want[1][0][3] > 0
    assert want[2][0][1] > 0 and want[2][0][2] > 0 and want[2][0][3] == 0
    assert all(t > 0 for t in want[3][0][1:])  # (every kind `three` has: it has no gate)
    assert s.check(advs) == want
    assert s.check(advs[::-1]) == want[::-1]
    assert [s.check([a])[0] for a in advs] == want
    s.close()


def test_gate_lookup_and_shuffle_failures_in_one_witness(ctx, zg, orc):
    pc, advs = cases.mixed_wide()
    s = Setup(orc, zg, ctx, pc, batch=2)
    want = [s.want(a) for a in advs]
    assert want[0] == CLEAN and all(want[1][0][kd] > 0 for kd in (0, 1, 3))
    assert s.check(advs) == want
    s.close()


# ---------------------------------------------------------------------------------------------- challenges
@pytest.mark.parametrize("name", ["with_challenge", "with_challenge_phased"])
def test_shuffles_with_a_challenge_per_witness(ctx, zg, orc, name):
    pc = shuffle_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc, batch=3)
    chs = [cases.challenges_for(pc, b) for b in range(3)]
    variants = [0, BAD, 1]
    advs = [columns_of(pc, c, v) for c, v in zip(chs, variants)]
    want = [s.want(a, c) for a, c in zip(advs, chs)]
    assert want[0] == CLEAN and want[2] == CLEAN and want[1][0][SHUFFLE] >= 1
    assert s.check(advs, chs) == want
    got = s.prover.check_phased(pc.synthesize(variants), [s.inst()] * 3, np.stack([fr(zg, c) for c in chs]))
    assert got == want
    s.close()


@pytest.mark.parametrize("name", ["three_phase", "rlc"])
def test_challenges_in_gates_lookup_inputs_and_tables(ctx, zg, orc, name):
    pc = phases_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc, batch=3)
    chs = [cases.challenges_for(pc, b) for b in range(3)]
    variants = [0, 1, 0]
    advs = [columns_of(pc, c, v) for c, v in zip(chs, variants)]
    want = [s.want(a, c, v) for a, c, v in zip(advs, chs, variants)]
    assert want == [CLEAN] * 3
    assert s.check(advs, chs, variants=variants) == want
    got = s.prover.check_phased(pc.synthesize(variants), [s.inst(v) for v in variants], np.stack([fr(zg, c) for c in chs]))
    assert got == want
    # a witness synthesised for other challenge values than the ones passed fails where the enumerator says
    other = [chs[1], chs[2], chs[0]]
    want = [s.want(a, c, v) for a, c, v in zip(advs, other, variants)]
    assert all(sum(w[0]) > 0 for w in want)
    cap = max(sum(w[0]) for w in want)
    assert s.check(advs, other, cap=cap, variants=variants) == want
    s.close()


def test_null_challenges_are_refused_and_the_prover_stays_usable(ctx, zg, orc):
    pc = shuffle_circuits.with_challenge()
    s = Setup(orc, zg, ctx, pc)
    ch = [cases.challenges_for(pc)]
    adv = columns_of(pc, ch[0], 0)
    assert s.check([adv], ch) == [CLEAN]
    with pytest.raises(zg.ZgError) as e:
        s.check([adv], None)
    assert e.value.status == ZG_ERR_INVALID_ARG and "challenges" in str(e.value)
    assert s.check([adv], ch) == [CLEAN]
    s.close()


# ---------------------------------------------------------------------------------------------- nothing older moved
def _launches(ctx, call):
    ctx.profile(True)
    ctx.profile_collect()
    out = call()
    stats = ctx.profile_collect()
    ctx.profile(False)
    return out, {name: v[0] for name, v in stats.items()}


def test_without_shuffles_and_challenges_the_report_and_the_launches_are_check_batch_s(ctx, zg, orc):
    cs, asg, ilen = advice_table_circuit(5)
    params = orc.params_new(cs.k, 0xABCDEF)
    prover = zg.Prover(ctx, cs.to_c(), asg.fixed_values(), asg.sigma_values(), params.g_np(), params.g_lagrange_np(), orc.fr_from_int(0x1234567))
    prover.set_batch(2)
    miss = changed(asg, [(ADVICE, 0, 4, 99), (ADVICE, 0, 0, 5)])
    advs, insts = [a.advice_values() for a in (asg, miss)], [a.instance_values(ilen) for a in (asg, miss)]
    want = [failures3(cs, a) for a in (asg, miss)]
    assert want[0] == ([0, 0, 0], []) and sum(want[1][0]) > 0
    prover.check_batch(advs, insts)  # (the key's check data is made at the first check)
    old, old_launches = _launches(ctx, lambda: prover.check_batch(advs, insts))
    new, new_launches = _launches(ctx, lambda: prover.check_circuit(advs, insts))
    assert old == want and new == [(t + [0], recs) for t, recs in want]
    assert old_launches and new_launches == old_launches
    assert not any(name in new_launches for name in NEW_KERNELS)
    prover.close()


def test_check_then_prove_fork_and_device_pointers(ctx, zg, orc):
    pc = shuffle_circuits.three()
    s = Setup(orc, zg, ctx, pc, batch=2)
    good, bad = columns_of(pc, (), 0), columns_of(pc, (), BAD)
    want = [s.want(good), s.want(bad)]
    inst = s.inst()
    alone = s.prover.prove(mont(good), inst, 5)
    assert s.check([good]) == [CLEAN]  # (writes slot 0, as a proof would)
    got, sts = s.prover.prove_batch(None, [inst], [5], device=True)  # the slot as it stands
    assert sts == [0] and got[0] == alone
    # the slots as they stand, named by their addresses, and on a fork
    assert s.check([good, bad]) == want
    assert s.prover.check_circuit(None, [inst, inst], device=True) == want
    assert s.prover.check_circuit([s.prover.advice_slot(1), s.prover.advice_slot(0)], [inst, inst], device=True) == [want[1], want[1]]
    ctx2 = zg.Ctx(0)
    f = s.prover.fork(ctx2)
    f.set_batch(2)
    assert s.check([good, bad], prover=f) == want
    f.close()
    ctx2.close()
    s.close()
