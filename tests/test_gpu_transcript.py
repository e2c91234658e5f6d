"""halo2's Blake2b transcript with compressed points on the device (zg_prover_set_transcript / zg_verifier_set_transcript,
zg_g1_compress / zg_g1_decompress).  Proof bytes are held against create_proof walked by the CALLER
over the library's arithmetic-level entries (tests/arith_level.py DeviceBackend) with the Blake2b writer of
tests/transcript_ref.py -- that path takes its challenges as arguments and shares no transcript code with the prover --
verdicts against the reference verifier of tests/proof_ref.py on that transcript, and decompressed
points against Python integers.  tests/test_transcript_host.py holds the host code and the golden proof without a GPU."""
import ctypes
import json

import numpy as np
import pytest

import arith_level
import field9_ref as fref
import proof_ref
import transcript_cases as tc
import transcript_ref as b2
from circuits import toy_circuit, variant_circuit
from test_gpu_multi import toy_family

pytestmark = pytest.mark.gpu

R, Q = proof_ref.R, proof_ref.Q
GWC, SHPLONK = 0, 1
EVM, BLAKE2B = 0, 1

CIRCUITS = {
    "toy": lambda: toy_circuit(k=5),
    "two_lookups": lambda: toy_circuit(k=5, two_lookups=True),
    "gates_only": lambda: variant_circuit("gates_only", k=5),
    "no_lookup": lambda: variant_circuit("no_lookup", k=5),
    "wide_lookup": lambda: variant_circuit("wide_lookup", k=5),
}


class Setup:
    """One key: the device prover and verifier (both set to Blake2b and to `scheme`), the reference vk, the witnesses of a
    family; the bases are registered once, for the prover and for the caller-side walk."""

    def __init__(self, orc, zg, ctx, family, scheme=GWC, seed=0xABCDEF, vk=0x1234567, ilen=None):
        cs, asg, ilen0 = family[0]
        self.orc, self.zg, self.ctx, self.cs, self.scheme = orc, zg, ctx, cs, scheme
        self.ilen = ilen0 if ilen is None else ilen
        self.img = cs.to_c()
        self.params = orc.params_new(cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        self.fixed, self.sigma = asg.fixed_values(), asg.sigma_values()
        for _, other, _ in family[1:]:
            assert np.array_equal(other.fixed_values(), self.fixed) and np.array_equal(other.sigma_values(), self.sigma)
        self.g, self.gl = ctx.register_bases(self.params.g_np()), ctx.register_bases(self.params.g_lagrange_np())
        self.prover = zg.Prover(ctx, self.img, self.fixed, self.sigma, self.g, self.gl, self.vk_repr)
        fc, sc = self.prover.vk_commitments()
        self.verifier = zg.Verifier(ctx, self.img, fc, sc, self.params.g_np()[0], np.array(self.params.g2, np.uint64),
                                    np.array(self.params.s_g2, np.uint64), self.vk_repr)
        self.ref = proof_ref.Vk(cs, self.params, self.fixed, self.sigma, self.vk_repr)
        self.adv = [a.advice_values() for _, a, _ in family]
        self.inst = [a.instance_values(self.ilen) for _, a, _ in family]
        self.prover.set_batch(len(family))
        for obj in (self.prover, self.verifier):
            obj.set_multiopen(scheme)
            obj.set_transcript(BLAKE2B)

    def walked(self, i, seed, writer=None):
        """create_proof walked by the caller over the device entries, Blake2b writer (or, GWC only, the one given)"""
        be = arith_level.DeviceBackend(self.zg, self.ctx, self.prover, self.cs, self.fixed, self.sigma, self.g, self.gl, seed)
        if writer is None:
            out = proof_ref.create_proof(be, self.ref, self.adv[i], self.inst[i], scheme=self.scheme, transcript=BLAKE2B)
        else:
            assert self.scheme == GWC
            out = arith_level.create_proof(be, self.cs, self.vk_repr, self.adv[i], self.inst[i], writer=writer)
        self.ctx.sync()
        return out

    def both_forms(self, make):
        self.prover.set_overlap(True)
        a = make()
        self.prover.set_overlap(False)
        b = make()
        assert a == b
        return a

    def ref_verify(self, insts, proof):
        return proof_ref.verify(self.ref, insts, proof, scheme=self.scheme, transcript=BLAKE2B).verdict

    def close(self):
        self.verifier.close()
        self.prover.close()
        self.g.free()
        self.gl.free()


def cls(v):
    return 1 if v == 1 else 0 if v == 0 else -1


# ---------------------------------------------------------------------------------------------------- proof bytes
@pytest.mark.parametrize("scheme", [GWC, SHPLONK])
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_bytes_are_the_caller_walked_proofs_in_both_forms(ctx, zg, orc, name, scheme):
    s = Setup(orc, zg, ctx, [CIRCUITS[name]()], scheme)
    got = s.both_forms(lambda: s.prover.prove(s.adv[0], s.inst[0], 11))
    assert got == s.walked(0, 11)
    assert len(got) == proof_ref.proof_len(s.cs, N=1, scheme=scheme, transcript=BLAKE2B) <= s.prover.proof_cap
    assert s.ref_verify([s.inst[0]], got) == 1
    assert s.verifier.verify([got], [s.inst[0]], 5) == [1]
    s.close()


def test_batch_of_three_witnesses_and_keys(ctx, zg, orc):
    s = Setup(orc, zg, ctx, toy_family(3))
    seeds = [21, 22, 23]
    proofs = s.both_forms(lambda: s.prover.prove_batch(s.adv, s.inst, seeds)[0])
    assert len(set(proofs)) == 3
    assert proofs == [s.walked(i, seeds[i]) for i in range(3)]
    assert s.verifier.verify(proofs, s.inst, 7) == [1, 1, 1]
    s.close()


def test_prove_multi_is_the_golden_record_and_one_circuit_is_prove(ctx, zg, orc):
    s = Setup(orc, zg, ctx, toy_family(2))
    one = s.both_forms(lambda: s.prover.prove_multi([s.adv[0]], [s.inst[0]], [31]))
    assert one == s.prover.prove(s.adv[0], s.inst[0], 31)
    two = s.both_forms(lambda: s.prover.prove_multi(s.adv, s.inst, [31, 32]))
    rec = json.load(open(tc.GOLDEN_B2_N2))  # the proof the host test judges: these bytes
    assert (rec["params_seed"], rec["vk_repr"], rec["seeds"]) == (0xABCDEF, 0x1234567, [31, 32]) and two.hex() == rec["proof"]
    assert len(two) == proof_ref.proof_len(s.cs, N=2, transcript=BLAKE2B) <= s.prover.proof_size_multi(2) < proof_ref.proof_len(s.cs, N=2)
    assert s.verifier.verify_multi([two], [s.inst], 9, 2) == [1]
    assert s.verifier.verify_multi([two], [[s.inst[1], s.inst[0]]], 9, 2) == [0]
    s.close()


def test_switching_back_gives_the_evm_bytes_and_a_fork_inherits(ctx, zg, orc):
    s = Setup(orc, zg, ctx, [toy_circuit(k=5)])
    pk = orc.ProvingKey(s.img, s.fixed, s.sigma, s.params, s.vk_repr)
    st, want_evm, _ = orc.create_proof(pk, s.adv[0], s.inst[0], 41)
    assert st == 0
    want_b2 = s.prover.prove(s.adv[0], s.inst[0], 41)
    assert s.prover.transcript == BLAKE2B and s.prover.proof_cap < orc.proof_size(s.img)
    c2 = zg.Ctx(0)
    try:
        fork = s.prover.fork(c2)
        assert fork.transcript == BLAKE2B
        assert fork.prove(s.adv[0], s.inst[0], 41) == want_b2
        fork.close()
    finally:
        c2.close()
    s.prover.set_transcript(EVM)
    assert s.prover.transcript == EVM and s.prover.proof_cap == orc.proof_size(s.img)
    assert s.prover.prove(s.adv[0], s.inst[0], 41) == want_evm
    fork = s.prover.fork(ctx)
    assert fork.transcript == EVM
    fork.close()
    s.prover.set_transcript(BLAKE2B)
    assert s.prover.prove(s.adv[0], s.inst[0], 41) == want_b2
    # each verifier refuses the other transcript's proof
    assert s.verifier.verify([want_b2], [s.inst[0]], 5) == [1]
    assert s.verifier.verify([want_evm], [s.inst[0]], 5)[0] != 1
    s.verifier.set_transcript(EVM)
    assert s.verifier.transcript == EVM
    assert s.verifier.verify([want_evm], [s.inst[0]], 5) == [1]
    assert s.verifier.verify([want_b2], [s.inst[0]], 5)[0] != 1
    s.close()


class CountingTranscript(b2.Blake2bWriter):
    """the writer, counting what it absorbs: the total at every finalisation"""

    def __init__(self, keccak=None):
        super().__init__(keccak)
        self.absorbed, self.at_squeeze = 0, []
        CountingTranscript.last = self

    def common_scalar(self, v):
        super().common_scalar(v)
        self.absorbed += 33

    def write_point(self, pt):
        super().write_point(pt)
        self.absorbed += 65

    def squeeze(self):
        self.absorbed += 1
        self.at_squeeze.append(self.absorbed)
        return super().squeeze()


def test_block_edges_a_squeeze_at_a_full_block_and_one_byte_later(ctx, zg, orc):
    """the toy circuit (3 advice columns, 1 lookup, 1 instance column) with 24 instance values: the beta squeeze finalises
    at 9 whole blocks, the gamma squeeze one byte later"""
    s = Setup(orc, zg, ctx, [toy_circuit(k=5)], ilen=24)
    assert (s.cs.n_advice, len(s.cs.lookups), s.cs.n_instance, s.inst[0].shape[1]) == (3, 1, 1, 24)
    walked = s.walked(0, 17, writer=CountingTranscript)
    totals = CountingTranscript.last.at_squeeze
    assert totals[:3] == [33 * 25 + 65 * 3 + 1, 33 * 25 + 65 * 3 + 1 + 65 * 2 + 1, 33 * 25 + 65 * 3 + 1 + 65 * 2 + 2]
    assert totals[1] == 1152 == 9 * 128 and totals[2] % 128 == 1
    assert {0, 1} <= {t % 128 for t in totals}
    got = s.both_forms(lambda: s.prover.prove(s.adv[0], s.inst[0], 17))
    assert got == walked
    assert s.ref_verify([s.inst[0]], got) == 1
    assert s.verifier.verify([got], [s.inst[0]], 5) == [1]
    s.close()


# ---------------------------------------------------------------------------------------------------- verdicts
def tampered(s, good):
    """name -> (proof, instance, expected class)"""
    points, _ = proof_ref.counts(s.cs, N=1, scheme=s.scheme)
    tail = 2 if s.scheme == SHPLONK else proof_ref.n_point_sets(s.cs)
    s0 = 32 * (points - tail)  # the first evaluation
    sc0 = int.from_bytes(good[s0:s0 + 32], "little")
    inst = s.inst[0]

    def first(enc):
        return enc + good[32:]

    bit6 = bytearray(good[:32])
    bit6[31] |= 0x40
    sign = bytearray(good[:32])
    sign[31] ^= 0x80
    wrong = inst.copy()
    wrong[0, 0] = s.orc.fr_from_int((s.orc.fr_to_int(inst[0, 0]) + 1) % R)
    return {
        "good": (good, inst, 1),
        "the sign bit of one commitment flipped": (first(bytes(sign)), inst, 0),
        "one evaluation changed": (good[:s0] + b2.le32((sc0 + 1) % R) + good[s0 + 32:], inst, 0),
        "a wrong instance": (good, wrong, 0),
        "one trailing byte": (good + b"\x00", inst, 0),
        "one byte short": (good[:-1], inst, -1),
        "x = q": (first(b2.le32(Q)), inst, -1),
        "x = 2^255 - 1 with the sign bit on top": (first(b"\xff" * 32), inst, -1),
        "bit 6 set": (first(bytes(bit6)), inst, -1),
        "an x without a point": (first(b2.le32(tc.smallest_x(False))), inst, -1),
        "an all-zero commitment": (first(bytes(32)), inst, -1),
        "the last commitment all zero": (good[:-32] + bytes(32), inst, -1),
        "a scalar not below r": (good[:s0] + b2.le32(sc0 + R) + good[s0 + 32:], inst, -1),
        "malformed wins over trailing": (first(bytes(32)) + b"\x00", inst, -1),
    }


@pytest.mark.parametrize("scheme", [GWC, SHPLONK])
def test_verdict_classes_inside_a_batch_of_good_proofs(ctx, zg, orc, scheme):
    s = Setup(orc, zg, ctx, [toy_circuit(k=5)], scheme)
    good = [s.prover.prove(s.adv[0], s.inst[0], seed) for seed in (1, 2, 3)]
    for name, (proof, inst, want) in tampered(s, good[1]).items():
        ref = s.ref_verify([inst], proof)
        got = s.verifier.verify([good[0], proof, good[2]], [s.inst[0], inst, s.inst[0]], 5)
        assert cls(got[1]) == ref == want, name
        assert got[0] == got[2] == 1, name
        assert s.verifier.verify([proof], [inst], 6)[0] == got[1], name  # the verdict a lone verification gives
    s.close()


# ---------------------------------------------------------------------------------------------------- zg_g1_decompress
def encodings(n):
    """the edge encodings mixed among compressed multiples of the generator, both signs, repeated entries"""
    edges = list(tc.edge_encodings().values())
    out, P = [], None
    for i in range(n):
        P = fref.ec_add(P, fref.G)
        if i % 7 == 3:
            out.append(edges[(i // 7) % len(edges)])
        elif i % 11 == 5:
            out.append(out[i - 2])
        else:
            out.append(b2.compress(*(fref.ec_neg(P) if i % 3 == 1 else P)))
    return out


def check_decompressed(zg, enc, points, valid):
    assert points.shape == (len(enc), 8) and valid.shape == (len(enc),)
    bad = []
    for i, e in enumerate(enc):
        want = b2.decompress(e)
        got = (zg.fq_to_int(points[i, 0:4]), zg.fq_to_int(points[i, 4:8]))
        if (int(valid[i]), got) != ((0, (0, 0)) if want is None else (1, want)):
            bad.append((i, e.hex(), int(valid[i]), got, want))
    assert not bad, "%d of %d wrong, the first: %s" % (len(bad), len(enc), bad[0])
    ok = np.flatnonzero(valid)
    assert 0 < len(ok) < len(enc) or len(enc) < 4
    back = zg.g1_compress(points[ok])  # the round trip
    assert [bytes(b) for b in back] == [enc[i] for i in ok]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_g1_decompress_host_and_device_forms(ctx, zg, n):
    import torch

    enc = encodings(n)
    arr = np.frombuffer(b"".join(enc), np.uint8).reshape(n, 32)
    points, valid = ctx.g1_decompress(arr)
    check_decompressed(zg, enc, points, valid)
    d_points, d_valid = ctx.g1_decompress(torch.from_numpy(arr.copy()).cuda())
    assert np.array_equal(d_points.cpu().numpy().view(np.uint64), points) and np.array_equal(d_valid.cpu().numpy(), valid)
    if n == 257:  # an invalid lane leaves its neighbours right: the same array with one more lane spoiled
        spoiled = list(enc)
        spoiled[64] = tc.signed(Q, 1)
        p2, v2 = ctx.g1_decompress(np.frombuffer(b"".join(spoiled), np.uint8).reshape(n, 32))
        keep = np.arange(n) != 64
        assert v2[64] == 0 and not p2[64].any() and np.array_equal(p2[keep], points[keep]) and np.array_equal(v2[keep], valid[keep])


def test_arguments(ctx, zg, orc):
    s = Setup(orc, zg, ctx, [toy_circuit(k=5)])
    for obj in (s.prover, s.verifier):
        for value in (2, -1):
            with pytest.raises(zg.ZgError) as e:
                obj.set_transcript(value)
            assert e.value.status == -1  # ZG_ERR_INVALID_ARG
        assert obj.transcript == BLAKE2B  # nothing changed
    s.close()
    lib, one = ctx.lib, ctypes.c_void_p(64)  # (never dereferenced: the checks come first)
    assert lib.zg_g1_decompress(ctx.h, None, ctypes.c_size_t(0), None, None) == 0
    assert lib.zg_g1_decompress_dev(ctx.h, None, ctypes.c_size_t(0), None, None) == 0
    assert lib.zg_g1_compress(None, ctypes.c_size_t(0), None) == 0
    assert lib.zg_g1_decompress(ctx.h, None, ctypes.c_size_t(1), one, one) == -1
    assert lib.zg_g1_decompress_dev(ctx.h, one, ctypes.c_size_t(1), None, one) == -1
    assert lib.zg_g1_decompress_dev(ctx.h, one, ctypes.c_size_t(1), one, None) == -1
    assert lib.zg_g1_compress(None, ctypes.c_size_t(1), one) == -1
    assert lib.zg_g1_decompress(ctx.h, one, ctypes.c_size_t(1 << 28), one, one) == -4  # ZG_ERR_UNSUPPORTED
    assert lib.zg_g1_decompress_dev(ctx.h, one, ctypes.c_size_t(1 << 28), one, one) == -4
    # a point off the curve gives bytes that do not decompress to it
    off = np.concatenate([zg.fq_from_int(1), zg.fq_from_int(3)])[None, :]
    points, valid = ctx.g1_decompress(zg.g1_compress(off))
    assert valid[0] == 1 and (zg.fq_to_int(points[0, 0:4]), zg.fq_to_int(points[0, 4:8])) == (1, Q - 2)


# ---------------------------------------------------------------------------------------------------- one real shape
def test_tiny_model_k14_image_to_proof(ctx, zg, orc):
    import witness_tape
    import wnn_circuit
    import wnn_model

    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    wnn, real = wnn_model.load_checked_in(name), wnn_model.load_test_image()
    s = Setup(orc, zg, ctx, [wnn_circuit.build(wnn, real, k)[:3]], GWC, seed=0x5EED, vk=0xC0FFEE)
    plan = zg.WitnessPlan(ctx, witness_tape.trace(wnn, k).arrays())
    proofs, outputs, sts = s.prover.prove_images(plan, real[None], [7])
    assert sts == [0]
    points, scalars = proof_ref.counts(s.cs, N=1, scheme=GWC)
    assert (points, scalars) == (30, 60) and len(proofs[0]) == 32 * (points + scalars) == proof_ref.proof_len(s.cs, N=1, transcript=BLAKE2B)
    assert [zg.fr_to_int(x) for x in outputs[0]] == wnn.predict(real)
    inst = outputs[0][None, :, :]
    assert s.verifier.verify([proofs[0]], [inst], 3) == [1]
    wrong = inst.copy()
    wrong[0, 7] = zg.fr_from_int(zg.fr_to_int(inst[0, 7]) + 1)
    assert s.verifier.verify([proofs[0]], [wrong], 3) == [0]
    plan.close()
    s.close()
