"""The SHPLONK multi-open on the device (zg_prover_set_multiopen / zg_verifier_set_multiopen).
Bytes are held against the reference prover of tests/proof_ref.py (upstream's order, chained divisions, over the host
backend of tests/arith_level.py) wherever it runs, verdicts against its verifier; tests/test_shplonk_host.py holds the
reference against itself and the oracle on a machine without a GPU."""
import json

import numpy as np
import pytest

import arith_level
import poly_ref as pr
import proof_ref
from circuits import toy_circuit, variant_circuit
from test_gpu_multi import toy_family
from test_shplonk_host import GOLDEN_N2, seventeen_points_circuit, seventeen_sets_circuit, shplonk

pytestmark = pytest.mark.gpu

R, Q = proof_ref.R, proof_ref.Q
GWC, SHPLONK = 0, 1

CIRCUITS = {
    "toy": lambda: toy_circuit(k=5),
    "two_lookups": lambda: toy_circuit(k=5, two_lookups=True),
    "gates_only": lambda: variant_circuit("gates_only", k=5),
    "no_lookup": lambda: variant_circuit("no_lookup", k=5),
    "wide_lookup": lambda: variant_circuit("wide_lookup", k=5),
}


def be32(x: int) -> bytes:
    return x.to_bytes(32, "big")


class Setup:
    """One key: the oracle's, the device prover and verifier (both set to SHPLONK), the reference vk; witnesses of a family."""

    def __init__(self, orc, zg, ctx, family, seed=0xABCDEF, vk=0x1234567):
        cs, asg, ilen = family[0]
        self.orc, self.cs, self.ilen = orc, cs, ilen
        self.img = cs.to_c()
        self.params = orc.params_new(cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        self.fixed, self.sigma = asg.fixed_values(), asg.sigma_values()
        for _, other, _ in family[1:]:
            assert np.array_equal(other.fixed_values(), self.fixed) and np.array_equal(other.sigma_values(), self.sigma)
        self.pk = orc.ProvingKey(self.img, self.fixed, self.sigma, self.params, self.vk_repr)
        self.prover = zg.Prover(ctx, self.img, self.fixed, self.sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr)
        fc, sc = self.prover.vk_commitments()
        self.verifier = zg.Verifier(ctx, self.img, fc, sc, self.params.g_np()[0], np.array(self.params.g2, np.uint64),
                                    np.array(self.params.s_g2, np.uint64), self.vk_repr)
        self.ref = proof_ref.Vk(cs, self.params, self.fixed, self.sigma, self.vk_repr)
        self.adv = [a.advice_values() for _, a, _ in family]
        self.inst = [a.instance_values(ilen) for _, a, _ in family]
        self.prover.set_batch(len(family))
        self.prover.set_multiopen(SHPLONK)
        self.verifier.set_multiopen(SHPLONK)

    def oracle_gwc(self, i, seed):
        st, proof, _ = self.orc.create_proof(self.pk, self.adv[i], self.inst[i], seed)
        assert st == 0
        return proof

    def reference(self, i, seed):
        """the reference prover's SHPLONK proof of witness i"""
        orc = self.orc
        st, _, tr = orc.create_proof(self.pk, self.adv[i], self.inst[i], seed, want_trace=True)
        assert st == 0
        h_ext = tr.array("h_ext", 1 << self.cs.extended_k())
        challenges = [pr.to_int(tr.fe(name)) for name in ("theta", "beta", "gamma", "y")]
        orc.trace_free(tr)
        be = arith_level.HostBackend(orc, self.cs, self.fixed, self.sigma, self.params, seed, h_ext, challenges)
        return proof_ref.create_proof(be, self.ref, self.adv[i], self.inst[i], scheme=SHPLONK)

    def both_forms(self, make):
        self.prover.set_overlap(True)
        a = make()
        self.prover.set_overlap(False)
        b = make()
        assert a == b
        return a

    def close(self):
        self.verifier.close()
        self.prover.close()


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_bytes_are_the_reference_provers_in_both_forms(ctx, zg, orc, name):
    s = Setup(orc, zg, ctx, [CIRCUITS[name]()])
    got = s.both_forms(lambda: s.prover.prove(s.adv[0], s.inst[0], 11))
    assert got == s.reference(0, 11)
    assert len(got) == proof_ref.proof_len(s.cs, N=1, scheme=SHPLONK) <= s.prover.proof_cap
    assert shplonk(s.ref, [s.inst[0]], got) == 1
    assert s.verifier.verify([got], [s.inst[0]], 5) == [1]
    s.close()


@pytest.mark.parametrize("k", [5, 10, 11])
def test_two_lookups_at_the_division_kernels_sizes(ctx, zg, orc, k):
    """k = 5: below one workgroup; k = 10: n = KD_LANES, four 256-row blocks of the latency form; k = 11: strip length 2"""
    s = Setup(orc, zg, ctx, [toy_circuit(k=k, two_lookups=True)])
    got = s.both_forms(lambda: s.prover.prove(s.adv[0], s.inst[0], 12))
    assert got == s.reference(0, 12)
    assert s.verifier.verify([got], [s.inst[0]], 5) == [1]
    s.close()


def test_batch_of_three_witnesses_and_keys(ctx, zg, orc):
    """every proof of a lock-step batch has its own coefficient table: one proof's used for another gives other bytes"""
    s = Setup(orc, zg, ctx, toy_family(3))
    seeds = [21, 22, 23]
    proofs = s.both_forms(lambda: s.prover.prove_batch(s.adv, s.inst, seeds)[0])
    want = [s.reference(i, seeds[i]) for i in range(3)]
    assert proofs == want and len(set(want)) == 3
    assert s.verifier.verify(proofs, s.inst, 7) == [1, 1, 1]
    s.close()


def test_prove_multi(ctx, zg, orc):
    s = Setup(orc, zg, ctx, toy_family(2))
    one = s.both_forms(lambda: s.prover.prove_multi([s.adv[0]], [s.inst[0]], [31]))
    assert one == s.prover.prove(s.adv[0], s.inst[0], 31) == s.reference(0, 31)
    two = s.both_forms(lambda: s.prover.prove_multi(s.adv, s.inst, [31, 32]))
    rec = json.load(open(GOLDEN_N2))  # the proof the host test judges: these bytes
    assert (rec["params_seed"], rec["vk_repr"], rec["seeds"]) == (0xABCDEF, 0x1234567, [31, 32]) and two.hex() == rec["proof"]
    assert len(two) == proof_ref.proof_len(s.cs, N=2, scheme=SHPLONK) <= s.prover.proof_size_multi(2)
    # the prefix is the GWC proof's of the same circuits and keys
    s.prover.set_multiopen(GWC)
    gwc = s.prover.prove_multi(s.adv, s.inst, [31, 32])
    s.prover.set_multiopen(SHPLONK)
    assert two[:-128] == gwc[:len(gwc) - 64 * proof_ref.n_point_sets(s.cs)]
    assert shplonk(s.ref, s.inst, two) == 1
    assert s.verifier.verify_multi([two], [s.inst], 9, 2) == [1]
    swapped = [s.inst[1], s.inst[0]]
    assert shplonk(s.ref, swapped, two) == 0
    assert s.verifier.verify_multi([two], [swapped], 9, 2) == [0]
    s.close()


def test_fork_inherits_and_switching_back_gives_the_oracles_bytes(zg, orc, ctx):
    s = Setup(orc, zg, ctx, [toy_circuit(k=5)])
    want_gwc, want_sh = s.oracle_gwc(0, 41), s.reference(0, 41)
    c2 = zg.Ctx(0)
    try:
        fork = s.prover.fork(c2)
        assert fork.multiopen == SHPLONK
        assert fork.prove(s.adv[0], s.inst[0], 41) == want_sh
        fork.close()
    finally:
        c2.close()
    assert s.prover.prove(s.adv[0], s.inst[0], 41) == want_sh
    s.prover.set_multiopen(GWC)
    assert s.prover.multiopen == GWC and s.prover.proof_cap == orc.proof_size(s.img)
    assert s.prover.prove(s.adv[0], s.inst[0], 41) == want_gwc
    fork = s.prover.fork(ctx)
    assert fork.multiopen == GWC
    fork.close()
    s.prover.set_multiopen(SHPLONK)
    assert s.prover.prove(s.adv[0], s.inst[0], 41) == want_sh
    s.prover.set_batch(3)  # new slots while the prover is set to SHPLONK: its buffers follow them
    assert s.prover.prove_batch([s.adv[0]] * 3, [s.inst[0]] * 3, [41, 42, 41])[0][::2] == [want_sh, want_sh]
    s.close()


def test_caller_side_walk_over_the_device_entries(ctx, zg, orc):
    """create_proof walked by the caller with the SHPLONK tail over zg_fr_lincomb_dev, zg_kate_division_dev and the MSM
    (arith_level.DeviceBackend): a second device route to the prover's bytes."""
    s = Setup(orc, zg, ctx, [toy_circuit(k=5, two_lookups=True)])
    g, gl = ctx.register_bases(s.params.g_np()), ctx.register_bases(s.params.g_lagrange_np())
    try:
        be = arith_level.DeviceBackend(zg, ctx, s.prover, s.cs, s.fixed, s.sigma, g, gl, 13)
        walked = proof_ref.create_proof(be, s.ref, s.adv[0], s.inst[0], scheme=SHPLONK)
        ctx.sync()
    finally:
        g.free()
        gl.free()
    assert walked == s.prover.prove(s.adv[0], s.inst[0], 13)
    s.close()


def test_tiny_model_k14(ctx, zg, orc):
    import wnn_circuit
    import wnn_model

    orc.load().orc_set_threads(16)
    kk, name = wnn_model.MNIST_TINY
    cs, asg, ilen, _ = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), kk)
    s = Setup(orc, zg, ctx, [(cs, asg, ilen)], seed=0x5EED, vk=0xC0FFEE)
    proof = s.prover.prove(s.adv[0], s.inst[0], 7)
    gwc = s.oracle_gwc(0, 7)
    assert len(gwc) == 3840 and len(proof) == 3712 == proof_ref.proof_len(cs, N=1, scheme=SHPLONK)
    assert proof[:-128] == gwc[:len(gwc) - 64 * proof_ref.n_point_sets(cs)]
    assert shplonk(s.ref, [s.inst[0]], proof) == 1
    assert s.verifier.verify([proof], [s.inst[0]], 3) == [1]
    s.close()


def tampered(s, good):
    c = s.img.c
    s0 = 64 * (c.n_advice + 3 * c.n_lookups + proof_ref.n_sets(s.cs) + 1 + c.cs_degree - 1)  # the first evaluation
    sc0 = int.from_bytes(good[s0:s0 + 32], "big")
    g0 = s.params.g_np()[0]
    g0b = be32(s.orc.fq_to_int(g0[0:4])) + be32(s.orc.fq_to_int(g0[4:8]))
    h2x = int.from_bytes(good[-64:-32], "big")
    return {
        "good": (good, 1),
        "h1 replaced by g0": (good[:-128] + g0b + good[-64:], 0),
        "one evaluation changed": (good[:s0] + be32((sc0 + 1) % R) + good[s0 + 32:], 0),
        "one trailing byte": (good + b"\x00", 0),
        "truncated": (good[:-32], -1),
        "h2 off the curve": (good[:-64] + be32((h2x + 1) % Q) + good[-32:], -1),
        "h1 at infinity": (good[:-128] + bytes(64) + good[-64:], -1),
        "h2 not canonical": (good[:-64] + be32(h2x + Q) + good[-32:], -1),
    }


def cls(v):
    return 1 if v == 1 else 0 if v == 0 else -1


def test_verdict_classes_and_the_other_schemes_proofs(ctx, zg, orc):
    s = Setup(orc, zg, ctx, [toy_circuit(k=5)])
    good = s.prover.prove(s.adv[0], s.inst[0], 1)
    for name, (proof, want) in tampered(s, good).items():
        ref = shplonk(s.ref, [s.inst[0]], proof)
        got = s.verifier.verify([proof], [s.inst[0]], 5)[0]
        assert cls(got) == ref == want, name
    gwc = s.oracle_gwc(0, 1)
    assert s.verifier.verify([gwc], [s.inst[0]], 5)[0] != 1
    s.verifier.set_multiopen(GWC)
    assert s.verifier.multiopen == GWC
    assert s.verifier.verify([gwc], [s.inst[0]], 5) == [1]
    assert s.verifier.verify([good], [s.inst[0]], 5)[0] != 1
    s.close()


def test_batch_of_eight_with_one_bad_proof(ctx, zg, orc):
    s = Setup(orc, zg, ctx, [toy_circuit(k=5, two_lookups=True)])
    proofs = [s.prover.prove(s.adv[0], s.inst[0], 50 + b) for b in range(8)]
    bad = bytearray(proofs[5])
    bad[-100] ^= 1  # a bit of h1
    proofs[5] = bytes(bad)
    lone = [s.verifier.verify([p], [s.inst[0]], 8)[0] for p in proofs]
    assert s.verifier.verify(proofs, [s.inst[0]] * 8, 8) == lone
    assert [cls(v) for v in lone] == [shplonk(s.ref, [s.inst[0]], p) for p in proofs]
    assert lone[:5] == [1] * 5 and lone[6:] == [1, 1] and lone[5] != 1
    s.close()


def test_bad_arguments(ctx, zg, orc):
    s = Setup(orc, zg, ctx, [toy_circuit(k=5)])
    for obj in (s.prover, s.verifier):
        for scheme in (2, -1):
            with pytest.raises(zg.ZgError) as e:
                obj.set_multiopen(scheme)
            assert e.value.status == -1  # ZG_ERR_INVALID_ARG
        assert obj.multiopen == SHPLONK  # nothing changed
    # a point-range shard of the SRS: refused at the proof, and the prover makes proofs again once it is whole
    s.prover.set_shard(0, 2, 0, lambda send, recv: None)
    with pytest.raises(zg.ZgError) as e:
        s.prover.prove(s.adv[0], s.inst[0], 3)
    assert e.value.status == -4 and "shard" in str(e.value)  # ZG_ERR_UNSUPPORTED
    s.prover.set_shard(0, 1, 0, None)
    assert s.verifier.verify([s.prover.prove(s.adv[0], s.inst[0], 3)], [s.inst[0]], 5) == [1]
    s.close()


@pytest.mark.parametrize("make,what", [(seventeen_sets_circuit, "rotation sets"), (seventeen_points_circuit, "")])
def test_limits(ctx, zg, orc, make, what):
    """more than HC_MAX_SETS rotation sets / PC_MAX_POINTS opening points: ZG_ERR_UNSUPPORTED from the proof and from the
    verification call, and a circuit inside the limits is served afterwards"""
    s = Setup(orc, zg, ctx, [make()])
    with pytest.raises(zg.ZgError) as e:
        s.prover.prove(s.adv[0], s.inst[0], 3)
    assert e.value.status == -4 and what in str(e.value)  # ZG_ERR_UNSUPPORTED
    with pytest.raises(zg.ZgError) as e:
        s.verifier.verify([s.oracle_gwc(0, 3)], [s.inst[0]], 5)
    assert e.value.status == -4 and what in str(e.value)
    if what:  # within the points' limit GWC serves the circuit
        s.prover.set_multiopen(GWC)
        s.verifier.set_multiopen(GWC)
        assert s.prover.prove(s.adv[0], s.inst[0], 3) == s.oracle_gwc(0, 3)
        assert s.verifier.verify([s.oracle_gwc(0, 3)], [s.inst[0]], 5) == [1]
    s.close()
