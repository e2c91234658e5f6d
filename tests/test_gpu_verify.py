"""Batched GWC verification on the device (csrc/verify.hip) and the verifying key's commitments
(zg_prover_vk_commitments): every verdict is checked against the oracle's pairing verifier, proof by proof, on accepted
proofs of every circuit shape the prover makes and on malformed or wrong ones."""
import numpy as np
import pytest

from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def cls(v):
    return 1 if v == 1 else 0 if v == 0 else -1


class Setup:
    def __init__(self, orc, zg, ctx, cs, asg, ilen, seed=0xABCDEF, vk=0x1234567, threads=16):
        self.cs, self.asg, self.ilen = cs, asg, ilen
        self.img = cs.to_c()
        self.params = orc.params_new(cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        fixed, sigma = asg.fixed_values(), asg.sigma_values()
        self.pk = orc.ProvingKey(self.img, fixed, sigma, self.params, self.vk_repr)
        self.prover = zg.Prover(ctx, self.img, fixed, sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr)
        fc, sc = self.prover.vk_commitments()
        self.verifier = zg.Verifier(ctx, self.img, fc, sc, self.params.g_np()[0], np.array(self.params.g2, np.uint64),
                                    np.array(self.params.s_g2, np.uint64), self.vk_repr)
        self.adv, self.inst = asg.advice_values(), asg.instance_values(ilen)

    def close(self):
        self.verifier.close()
        self.prover.close()

    def scalar_offset(self):
        c = self.img.c
        sets = (c.n_perm_columns + c.cs_degree - 3) // (c.cs_degree - 2) if c.n_perm_columns else 0
        return 64 * (c.n_advice + 3 * c.n_lookups + sets + 1 + c.cs_degree - 1)


def tiny(orc, zg, ctx):
    import wnn_circuit
    import wnn_model

    orc.load().orc_set_threads(16)
    kk, name = wnn_model.MNIST_TINY
    cs, asg, ilen, _ = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), kk)
    return Setup(orc, zg, ctx, cs, asg, ilen, seed=0x5EED, vk=0xC0FFEE)


def test_vk_commitments_match_commit_lagrange(ctx, zg, orc):
    for make in (lambda: Setup(orc, zg, ctx, *toy_circuit(5)), lambda: tiny(orc, zg, ctx)):
        s = make()
        fc, sc = s.prover.vk_commitments()
        gl = s.params.g_lagrange_np()
        for got, cols in ((fc, s.asg.fixed_values()), (sc, s.asg.sigma_values())):
            assert got.shape[0] == cols.shape[0]
            for c in range(cols.shape[0]):
                want = orc.normalise(orc.msm(cols[c], gl, threads=16))
                want = np.zeros(8, np.uint64) if not want[8:].any() else want[:8]
                assert np.array_equal(got[c], want), c
        s.close()


@pytest.mark.parametrize("k,force_degree", [(5, None), (5, 6), (6, 8), (8, 6), (10, None)])
def test_accepts_toy_proofs(ctx, zg, orc, k, force_degree):
    s = Setup(orc, zg, ctx, *toy_circuit(k, force_degree=force_degree))
    proofs = [s.prover.prove(s.adv, s.inst, seed) for seed in (1, 2, 3)]
    assert s.verifier.verify(proofs, [s.inst] * 3, 11) == [1, 1, 1]
    for p in proofs[:1]:
        assert orc.verify_proof_pairing(s.pk, s.inst, p) == 1
    s.close()


@pytest.mark.parametrize("kind", ["no_lookup", "gates_only", "wide_lookup", "advice_factor", "merged_selectors"])
def test_accepts_variant_proofs(ctx, zg, orc, kind):
    s = Setup(orc, zg, ctx, *variant_circuit(kind, k=6))
    proofs = [s.prover.prove(s.adv, s.inst, seed) for seed in (1, 2)]
    assert s.verifier.verify(proofs, [s.inst] * 2, 5) == [1, 1]
    assert orc.verify_proof_pairing(s.pk, s.inst, proofs[0]) == 1
    s.close()


def be(x: int) -> bytes:
    return x.to_bytes(32, "big")


def test_rejects_as_the_oracle_does(ctx, zg, orc):
    s = Setup(orc, zg, ctx, *toy_circuit(5))
    good = s.prover.prove(s.adv, s.inst, 1)
    s0 = s.scalar_offset()
    g0 = s.params.g_np()[0]
    g0b = be(orc.fq_to_int(g0[0:4])) + be(orc.fq_to_int(g0[4:8]))
    x0 = int.from_bytes(good[0:32], "big")
    sc0 = int.from_bytes(good[s0:s0 + 32], "big")
    bad_inst = s.inst.copy()
    bad_inst[0, 0] = orc.fr_from_int(orc.fr_to_int(bad_inst[0, 0]) + 1)
    unsat = s.adv.copy()
    unsat[2, 3] = orc.fr_from_int(99)
    cases = {
        "wrong instance": (good, bad_inst),
        "unsatisfied witness": (s.prover.prove(unsat, s.inst, 1), s.inst),
        "advice commitment x + 1": (be(x0 + 1) + good[32:], s.inst),
        "two commitments swapped": (good[64:128] + good[0:64] + good[128:], s.inst),
        "scalar + r": (good[:s0] + be(sc0 + R) + good[s0 + 32:], s.inst),
        "evaluation + 1": (good[:s0] + be((sc0 + 1) % R) + good[s0 + 32:], s.inst),
        "W replaced by g0": (good[:-64] + g0b, s.inst),
        "truncated by 32 bytes": (good[:-32], s.inst),
        "extended by 32 bytes": (good + bytes(32), s.inst),
    }
    other = Setup(orc, zg, ctx, *toy_circuit(5), seed=0x777)
    cases["made on another SRS"] = (other.prover.prove(s.adv, s.inst, 1), s.inst)
    names = list(cases)
    got = s.verifier.verify([cases[n][0] for n in names], [cases[n][1] for n in names], 3)
    for n, g in zip(names, got):
        want = orc.verify_proof_pairing(s.pk, cases[n][1], cases[n][0])
        assert cls(g) == cls(want), (n, g, want)
        assert g != 1, n
    # a proof checked against another circuit's verifier
    alt = Setup(orc, zg, ctx, *toy_circuit(5, force_degree=6))
    g = alt.verifier.verify([good], [s.inst], 3)[0]
    assert cls(g) == cls(orc.verify_proof_pairing(alt.pk, s.inst, good)) and g != 1
    # the good proof is still accepted beside all of them
    assert s.verifier.verify([good] + [cases[n][0] for n in names], [s.inst] + [cases[n][1] for n in names], 4)[0] == 1
    for x in (s, other, alt):
        x.close()


def test_tiny_model_batches(ctx, zg, orc):
    s = tiny(orc, zg, ctx)
    lone = s.prover.prove(s.adv, s.inst, 7)
    assert orc.verify_proof_pairing(s.pk, s.inst, lone) == 1
    assert s.verifier.verify([lone], [s.inst], 1) == [1]
    assert s.verifier.verify([], [], 1) == []
    s.prover.set_batch(64)
    s.prover.set_overlap(False)
    proofs, sts = s.prover.prove_batch([s.adv] * 64, [s.inst] * 64, list(range(100, 164)))
    assert all(x == 0 for x in sts)
    proofs = list(proofs)
    rng = np.random.default_rng(5)
    bad = sorted(int(i) for i in rng.choice(64, 3, replace=False))
    proofs[bad[0]] = proofs[bad[0]][:-32]
    s0 = s.scalar_offset()
    sc0 = int.from_bytes(proofs[bad[1]][s0:s0 + 32], "big")
    proofs[bad[1]] = proofs[bad[1]][:s0] + be((sc0 + 1) % R) + proofs[bad[1]][s0 + 32:]
    proofs[bad[2]] = proofs[bad[2]] + bytes(32)
    insts = [s.inst] * 64
    v1 = s.verifier.verify(proofs, insts, 21)
    v2 = s.verifier.verify(proofs, insts, 22)
    assert v1 == v2
    for b in range(64):
        if b in bad:
            assert cls(v1[b]) == cls(orc.verify_proof_pairing(s.pk, s.inst, proofs[b])), b
        else:
            assert v1[b] == 1, b
    assert [cls(v1[b]) for b in bad] == [-1, 0, 0]
    s.close()


def w0_offset(img):
    """Byte offset of W_0, the opening proof of the first point set (weight u^0 in L_b and R_b): after every scalar."""
    c = img.c
    sets = (c.n_perm_columns + c.cs_degree - 3) // (c.cs_degree - 2) if c.n_perm_columns else 0
    pts = c.n_advice + 3 * c.n_lookups + sets + 1 + c.cs_degree - 1
    scalars = c.n_advice_queries + c.n_fixed_queries + 1 + c.n_perm_columns + (3 * sets - 1 if sets else 0) + 5 * c.n_lookups
    return 64 * pts + 32 * scalars


def test_cancelling_errors_are_both_rejected(ctx, zg, orc):
    """Two copies of ONE proof whose W_0 is moved by +D and by -D.  W_0 has weight u^0 = 1 and both copies share x, so
    their errors e(+-D, [s - z_0]_2) cancel exactly in a batch whose weights are equal: only distinct r_b reject them."""
    s = Setup(orc, zg, ctx, *toy_circuit(5))
    p = s.prover.prove(s.adv, s.inst, 1)
    off = w0_offset(s.img)
    assert len(p) > off + 64
    d = s.params.g_np()[3]
    one = zg.fq_from_int(1)
    w = np.concatenate([zg.fq_from_int(int.from_bytes(p[off:off + 32], "big")),
                        zg.fq_from_int(int.from_bytes(p[off + 32:off + 64], "big")), one])

    def moved(sign):
        dd = np.concatenate([d, one])
        if sign < 0:
            dd[4:8] = zg.fq_from_int(Q - orc.fq_to_int(d[4:8]))
        aff = orc.normalise(orc.g1_add(w, dd))
        return p[:off] + be(orc.fq_to_int(aff[0:4])) + be(orc.fq_to_int(aff[4:8])) + p[off + 64:]

    plus, minus = moved(1), moved(-1)
    assert orc.verify_proof_pairing(s.pk, s.inst, plus) == 0 and orc.verify_proof_pairing(s.pk, s.inst, minus) == 0
    for key in (9, 10):
        assert s.verifier.verify([plus, p, minus, p], [s.inst] * 4, key) == [0, 1, 0, 1]
        assert s.verifier.verify([plus, minus], [s.inst] * 2, key) == [0, 0]
    s.close()


def test_all_zero_fixed_column(ctx, zg, orc):
    """A fixed column that is zero on every row commits to the identity (0, 0), and proofs that open it verify."""
    cs, asg, ilen = toy_circuit(5)
    z = cs.fixed_column()
    cs.create_gate([cs.fixed(z) * cs.advice(0)])  # opened at x like every other fixed query
    asg.fixed.append([0] * asg.n)
    s = Setup(orc, zg, ctx, cs, asg, ilen)
    fc, _ = s.prover.vk_commitments()
    assert fc.shape[0] == z + 1 and not fc[z].any()
    proofs = [s.prover.prove(s.adv, s.inst, seed) for seed in (1, 2)]
    assert orc.verify_proof_pairing(s.pk, s.inst, proofs[0]) == 1
    assert s.verifier.verify(proofs, [s.inst] * 2, 6) == [1, 1]
    bad = s.inst.copy()
    bad[0, 0] = orc.fr_from_int(orc.fr_to_int(bad[0, 0]) + 1)
    assert s.verifier.verify(proofs, [s.inst, bad], 6) == [1, 0]
    s.close()


def test_one_bad_proof_in_many(ctx, zg, orc):
    """The failure path: bad proofs at both ends and inside a batch are found; every other proof is accepted."""
    s = Setup(orc, zg, ctx, *toy_circuit(5))
    proofs = [s.prover.prove(s.adv, s.inst, seed) for seed in range(1, 41)]
    off = w0_offset(s.img)
    bad = {0, 17, 39}
    for b in bad:
        proofs[b] = proofs[b][:off] + proofs[(b + 1) % 40][off:off + 64] + proofs[b][off + 64:]
    got = s.verifier.verify(proofs, [s.inst] * 40, 12)
    assert got == [0 if b in bad else 1 for b in range(40)]
    assert orc.verify_proof_pairing(s.pk, s.inst, proofs[17]) == 0
    s.close()


@pytest.mark.parametrize("which", ["MNIST_SMALL", "MNIST_MEDIUM"])
def test_accepts_small_and_medium(ctx, zg, orc, which):
    import wnn_circuit
    import wnn_model

    kk, name = getattr(wnn_model, which)
    cs, asg, ilen, _ = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), kk)
    s = Setup(orc, zg, ctx, cs, asg, ilen, seed=0x5EED, vk=0xC0FFEE)
    p = s.prover.prove(s.adv, s.inst, 3)
    assert s.verifier.verify([p, p], [s.inst, s.inst], 2) == [1, 1]
    assert orc.verify_proof_pairing(s.pk, s.inst, p) == 1
    s.close()
