"""halo2's shuffle argument on the device: zg_prover_create_shuffles / zg_verifier_create_shuffles.
The oracle knows no shuffles, so the judge is tests/proof_ref.py, the Python-integer verify_proof (pinned to the oracle on
circuits without shuffles by tests/test_shuffle_host.py and to recorded proofs with shuffles by
tests/test_proof_golden_host.py), next to the library's own
batch verifier.  Circuits: tests/shuffle_circuits.py, k = 5 except where said.

Tolerances: none -- everything here is exact arithmetic mod r or bytes."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401 -- before the first HIP call of the process (tests/conftest.py)

import proof_ref
import shuffle_circuits
from circuit import R, omega_for
from circuits import toy_circuit
from shuffle_circuits import BAD

pytestmark = pytest.mark.gpu

GWC, SHPLONK, EVM, BLAKE2B = 0, 1, 0, 1
ZG_ERR_INVALID_ARG, ZG_ERR_UNSUPPORTED = -1, -4
FETCH_SHUFFLE_Z, FETCH_H, FETCH_H_PART1, FETCH_H_PART2 = 11, 0, 12, 13


class Setup:
    """prover + verifier with the circuit's shuffles + the reference's key"""

    def __init__(self, orc, zg, ctx, pc, seed=0xABCDEF, vk=0x1234567):
        self.pc, self.cs, self.zg, self.ctx, self.orc = pc, pc.cs, zg, ctx, orc
        self.img = pc.cs.to_c()
        self.params = orc.params_new(pc.cs.k, seed)
        self.vk_repr = orc.fr_from_int(vk)
        self.fixed, self.sigma = pc.fixed_values(), pc.sigma_values()
        self.prover = zg.Prover(ctx, self.img, self.fixed, self.sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr,
                                shuffles=self.img.shuffles)
        self.fc, self.sc = self.prover.vk_commitments()
        self.verifier = self.make_verifier(self.img.shuffles)
        self.phased = pc.n_phases > 1
        if self.phased:
            self.prover.set_phases(pc.advice_phase, pc.challenge_phase)
            self.verifier.set_phases(pc.advice_phase, pc.challenge_phase)
        self.vk = proof_ref.Vk(pc.cs, self.params, self.fixed, self.sigma, self.vk_repr)

    def make_verifier(self, shuffles):
        p = self.params
        return self.zg.Verifier(self.ctx, self.img, self.fc, self.sc, p.g_np()[0], np.array(p.g2, np.uint64), np.array(p.s_g2, np.uint64),
                                self.vk_repr, shuffles=shuffles)

    def advice(self, variant):
        return self.pc.full_advice([0] * len(self.pc.challenge_phase), variant)

    def prove(self, variants, seeds, prover=None):
        p = prover or self.prover
        insts = [self.pc.instance(v) for v in variants]
        if self.phased:
            proofs, st = p.prove_phased(self.pc.synthesize(variants), insts, seeds)
        elif len(variants) == 1:
            return [p.prove(self.advice(variants[0]), insts[0], seeds[0])]
        else:
            proofs, st = p.prove_batch([self.advice(v) for v in variants], insts, seeds)
        assert st == 0 or all(s == 0 for s in st)
        return proofs

    def ref(self, proof, variant=0, instance=None, scheme=GWC, transcript=EVM):
        inst = self.pc.instance(variant) if instance is None else instance
        return proof_ref.verify(self.vk, [inst], proof, advice_phase=self.pc.advice_phase, challenge_phase=self.pc.challenge_phase,
                                scheme=scheme, transcript=transcript)

    def dev(self, proofs, variants=None, verifier=None):
        insts = [self.pc.instance(v) for v in (variants or [0] * len(proofs))]
        return (verifier or self.verifier).verify(proofs, insts, 0xFEED)

    def close(self):
        self.verifier.close()
        self.prover.close()


def flip(proof, at):
    b = bytearray(proof)
    b[at] ^= 1
    return bytes(b)


def offsets(cs):
    """byte offsets (EVM transcript) of the first shuffle commitment and of the first shuffle evaluation"""
    S, NL, NS = proof_ref.n_sets(cs), len(cs.lookups), len(cs.shuffles)
    points, scalars = proof_ref.counts(cs, N=1, scheme=GWC)
    com = 64 * (cs.n_advice + 3 * NL + S)
    ev0 = 64 * (cs.n_advice + 3 * NL + S + NS + 1 + cs.degree() - 1)
    return com, ev0 + 32 * (scalars - 2 * NS)


def proof_size(cs, scheme=GWC, transcript=EVM):
    """what zg_prover_proof_size returns: SHPLONK's length is the proof's; GWC's bound counts one W per possible opening
    point (2 + every advice and fixed query) where the proof holds one per distinct point"""
    length = proof_ref.proof_len(cs, scheme=scheme, transcript=transcript)
    if scheme == SHPLONK:
        return length
    spare = 2 + len(cs.advice_queries) + len(cs.fixed_queries) - proof_ref.n_point_sets(cs)
    return length + (32 if transcript == BLAKE2B else 64) * spare


def read_slot(prover, slot=0):
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.zeros((prover.n_advice, prover.n, 4), np.uint64)
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(prover.advice_slot(slot)), ctypes.c_size_t(out.nbytes), 2) == 0
    return out


def ints(orc, arr):
    return [orc.fr_to_int(v) for v in arr]


# ---------------------------------------------------------------------------------------------- acceptance and rejection
@pytest.mark.parametrize("name", sorted(shuffle_circuits.SMALL))
def test_proofs_are_accepted_and_tampered_ones_rejected(ctx, zg, orc, name):
    pc = shuffle_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    assert s.prover.shuffles == len(pc.cs.shuffles) > 0
    (proof,) = s.prove([0], [7])
    assert len(proof) == proof_ref.proof_len(pc.cs) and s.prover.proof_cap == proof_size(pc.cs)
    assert s.ref(proof).verdict == 1
    assert s.dev([proof]) == [1]
    com, ev = offsets(pc.cs)
    for bad in (flip(proof, com + 40), flip(proof, ev + 31), flip(proof, ev + 32 + 31)):
        assert s.ref(bad).verdict <= 0 and s.dev([bad])[0] <= 0
    assert s.dev([proof, flip(proof, ev + 31), proof]) == [1, 0, 1]
    # ONE shuffled value changed: the call succeeds, the proof has full length, nobody accepts it
    (bad,) = s.prove([BAD], [7])
    assert len(bad) == len(proof)
    assert s.ref(bad, BAD).verdict == 0 and s.dev([bad], [BAD]) == [0]
    # a verifier that was not told the shuffles rejects the good proof
    plain = s.make_verifier(None)
    if s.phased:
        plain.set_phases(pc.advice_phase, pc.challenge_phase)
    assert s.dev([proof], verifier=plain)[0] <= 0
    plain.close()
    s.close()


def test_a_wrong_instance_is_rejected(ctx, zg, orc):
    """a circuit with an instance column beside its shuffle: toy's columns, advice 0 shuffled against itself"""
    cs, asg, ilen = toy_circuit(5)
    img0 = cs.to_c()
    # (the identity shuffle a against a needs no new witness: append its two monomials by hand)
    from circuit import ADVICE, MONT, _Monomial
    qi = cs.queries.index((ADVICE, 0, 0))
    nm = img0.c.n_monomials
    monos = (_Monomial * (nm + 1))()
    for i in range(nm):
        monos[i] = img0.monomials[i]
    for i in range(4):
        monos[nm].coeff[i] = (MONT >> (64 * i)) & 0xFFFFFFFFFFFFFFFF
    monos[nm].n_factors = 1
    monos[nm].factors[0] = qi
    img0.monomials = monos
    img0.c.monomials = ctypes.cast(monos, ctypes.POINTER(_Monomial))
    img0.c.n_monomials = nm + 1
    shuffles = [([(nm, 1)], [(nm, 1)])]
    cs.shuffles = [([cs.advice(0)], [cs.advice(0)])]
    params = orc.params_new(cs.k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x1234567)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    prover = zg.Prover(ctx, img0, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr, shuffles=shuffles)
    fc, sc = prover.vk_commitments()
    verifier = zg.Verifier(ctx, img0, fc, sc, params.g_np()[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr,
                           shuffles=shuffles)
    inst = asg.instance_values(ilen)
    proof = prover.prove(asg.advice_values(), inst, 9)
    vk = proof_ref.Vk(cs, params, fixed, sigma, vk_repr)
    assert len(proof) == proof_ref.proof_len(cs) == prover.proof_cap - 64 * (2 + len(cs.advice_queries) + len(cs.fixed_queries) - proof_ref.n_point_sets(cs))
    assert proof_ref.verify(vk, [inst], proof).verdict == 1 and verifier.verify([proof], [inst], 3) == [1]
    wrong = inst.copy()
    wrong[0, 0] = orc.fr_from_int(5)
    assert proof_ref.verify(vk, [wrong], proof).verdict == 0 and verifier.verify([proof], [wrong], 3) == [0]
    verifier.close()
    prover.close()


# ---------------------------------------------------------------------------------------------- the product and its commitment
@pytest.mark.parametrize("name,k", [("three", 5), ("rotated", 5), ("with_challenge", 5), ("plain", 11)])
def test_z_is_the_recurrence_and_its_commitment_the_msm(ctx, zg, orc, name, k):
    pc = shuffle_circuits.plain(k) if name == "plain" else shuffle_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    for overlap in (True, False):  # the grand product's block form (a lone proof) and its strip form
        s.prover.set_overlap(overlap)
        (proof,) = s.prove([1], [21])
        r = s.ref(proof, 1)
        assert r.verdict == 1 and s.dev([proof], [1]) == [1]
        cols = read_slot(s.prover)
        adv = [ints(orc, c) for c in cols]
        at = shuffle_circuits.cell_at(pc, adv, [r.challenges.get(j, 0) for j in range(len(pc.challenge_phase))])
        gl = s.params.g_lagrange_np()
        for j in range(len(pc.cs.shuffles)):
            zrow = s.prover.fetch(FETCH_SHUFFLE_Z, j, pc.n)
            z = ints(orc, zrow)
            want = proof_ref.shuffle_product(pc.cs, j, at, r.named["theta"], r.named["gamma"])
            assert z[0] == 1 and z[pc.usable] == 1
            assert z[:pc.usable + 1] == want, j
            assert len(set(z[pc.usable + 1:])) == pc.n - pc.usable - 1 and 0 not in z[pc.usable + 1:]  # (the blinding rows are drawn)
            com = orc.msm(np.ascontiguousarray(zrow), gl, threads=16)
            assert np.array_equal(proof_ref.affine(r.shuffle_z[0][j]), proof_ref.affine(com)), j
    s.close()


# ---------------------------------------------------------------------------------------------- the quotient
def lagrange_eval(values, p, n, w):
    """the polynomial with these n Lagrange values, at p (outside the domain)"""
    num = (pow(p, n, R) - 1) * pow(n, R - 2, R) % R
    acc, wi = 0, 1
    for v in values:
        if v:
            acc = (acc + v * wi % R * pow((p - wi) % R, R - 2, R)) % R
        wi = wi * w % R
    return acc * num % R


def quotient_at(orc, s, r, adv, zs, p, lk=()):
    """h(p) on Python integers for a circuit of gates, lookups and shuffles (no permutation): (sum of the terms folded by
    y) / (p^n - 1); lk: per lookup its product, a' and s' as read back"""
    pc, cs = s.pc, s.pc.cs
    n, w, bf = pc.n, omega_for(cs.k), cs.blinding_factors()
    theta, beta, gamma, y = r.named["theta"], r.named["beta"], r.named["gamma"], r.named["y"]
    w_inv = pow(w, R - 2, R)

    def cell(qi):
        kind, col, rot = cs.queries[qi]
        pt = p * pow(w, rot % n, R) % R
        return lagrange_eval(adv[col] if kind == 1 else pc.asg.col(kind)[col], pt, n, w)

    unit = lambda row: lagrange_eval([1 if i == row % n else 0 for i in range(n)], p, n, w)  # noqa: E731
    l0, llast = unit(0), unit(-(bf + 1))
    lactive = (1 - llast - sum(unit(-i) for i in range(1, bf + 1))) % R
    acc = 0
    for g in cs.gates:
        acc = (acc * y + g.eval(cell)) % R
    for (ins, tabs), (lz, pin, ptab) in zip(cs.lookups, lk):
        ai = ti = 0
        for e_in, e_tab in zip(ins, tabs):
            ai = (ai * theta + e_in.eval(cell)) % R
            ti = (ti * theta + e_tab.eval(cell)) % R
        z, zn = lagrange_eval(lz, p, n, w), lagrange_eval(lz, p * w % R, n, w)
        ap, apm, sp = lagrange_eval(pin, p, n, w), lagrange_eval(pin, p * w_inv % R, n, w), lagrange_eval(ptab, p, n, w)
        for term in ((1 - z) * l0, (z * z - z) * llast, ((ap + beta) * (sp + gamma) % R * zn - (ai + beta) * (ti + gamma) % R * z) * lactive,
                     (ap - sp) * l0, (ap - apm) * (ap - sp) % R * lactive):
            acc = (acc * y + term) % R
    for j, (ins, shs) in enumerate(cs.shuffles):
        ai = si = 0
        for e_in, e_sh in zip(ins, shs):
            ai = (ai * theta + e_in.eval(cell)) % R
            si = (si * theta + e_sh.eval(cell)) % R
        z, zn = lagrange_eval(zs[j], p, n, w), lagrange_eval(zs[j], p * w % R, n, w)
        for term in ((1 - z) * l0, (z * z - z) * llast, (zn * (si + gamma) - z * (ai + gamma)) % R * lactive):
            acc = (acc * y + term) % R
    return acc * pow((pow(p, n, R) - 1) % R, R - 2, R) % R


def test_h_is_the_quotient_on_every_part(ctx, zg, orc):
    """wide with its degree-6 gate at k = 5: the single coset in the latency form; the split 4n + n domain in the throughput
    form, with the terms by degree (the first part holds every term, the second the high ones: the gate of degree 6 and
    the shuffle's three, not the lookup's) and without (every term on both)"""
    pc = shuffle_circuits.wide(5, high_gate=True)
    s = Setup(orc, zg, ctx, pc)
    n, ek = pc.n, pc.cs.extended_k()
    zeta = orc.fr_to_int(s.prover.coset_generator())

    def inputs():
        (proof,) = s.prove([0], [33])
        r = s.ref(proof)
        assert r.verdict == 1 and s.dev([proof]) == [1]
        adv = [ints(orc, c) for c in read_slot(s.prover)]
        zs = [ints(orc, s.prover.fetch(FETCH_SHUFFLE_Z, j, n)) for j in range(len(pc.cs.shuffles))]
        lk = [tuple(ints(orc, s.prover.fetch(what, 0, n)) for what in (2, 3, 4))]  # lookup 0's product, a', s'
        return proof, r, adv, (zs, lk)

    def want(r, adv, zl, p):
        return quotient_at(orc, s, r, adv, zl[0], p, zl[1])

    proof, r, adv, zs = inputs()
    h = s.prover.fetch(FETCH_H, 0, 1 << ek)
    wx = omega_for(ek)
    for idx in (0, 1, n + 3, (1 << ek) - 1):
        assert orc.fr_to_int(h[idx]) == want(r, adv, zs, zeta * pow(wx, idx, R) % R), idx
    s.prover.set_overlap(False)
    assert s.prover.quotient_terms()["active"]
    for by_degree in (True, False):
        s.prover.set_quotient_terms(by_degree)
        proof2, r, adv, zs = inputs()
        assert proof2 == proof
        # the quotient the two parts were put together to, on the whole coset (from its coefficients)
        h = s.prover.fetch(FETCH_H, 0, 1 << ek)
        for idx in (0, 1, n + 3, (1 << ek) - 1):
            assert orc.fr_to_int(h[idx]) == want(r, adv, zs, zeta * pow(wx, idx, R) % R), (by_degree, idx)
        if by_degree:  # (the parts' buffers are reused: the first ends as coefficients of the high terms)
            with pytest.raises(zg.ZgError):
                s.prover.fetch(FETCH_H_PART1, 0, 4 * n)
            continue
        h1, h2 = s.prover.fetch(FETCH_H_PART1, 0, 4 * n), s.prover.fetch(FETCH_H_PART2, 0, n)
        w1, w2 = omega_for(pc.cs.k + 2), omega_for(pc.cs.k)
        for idx in (0, 5, 4 * n - 1):
            assert orc.fr_to_int(h1[idx]) == want(r, adv, zs, zeta * pow(w1, idx, R) % R), idx
        for idx in (0, 7, n - 1):
            assert orc.fr_to_int(h2[idx]) == want(r, adv, zs, zeta * zeta % R * pow(w2, idx, R) % R), idx
    s.close()


# ---------------------------------------------------------------------------------------------- forms, batches, forks
@pytest.mark.parametrize("name", ["three", "with_challenge_phased"])
def test_same_bytes_in_every_form(ctx, zg, orc, name):
    pc = shuffle_circuits.SMALL[name]()
    s = Setup(orc, zg, ctx, pc)
    s.prover.set_batch(3)
    variants, seeds = [0, 1, 2], [11, 12, 13]
    proofs = s.prove(variants, seeds)
    assert s.dev(proofs, variants) == [1, 1, 1] and all(s.ref(p, v).verdict == 1 for p, v in zip(proofs, variants))
    assert s.prove(variants, seeds) == proofs                                      # the same keys, the same bytes
    assert [s.prove([v], [sd])[0] for v, sd in zip(variants, seeds)] == proofs    # a batch is its single calls
    for overlap in (False, True):                                                  # both scheduling forms
        s.prover.set_overlap(overlap)
        assert s.prove(variants, seeds) == proofs
    child_ctx = zg.Ctx(0)
    child = s.prover.fork(child_ctx)
    assert child.shuffles == s.prover.shuffles
    assert s.prove(variants, seeds, prover=child) == proofs
    child.close()
    child_ctx.close()
    s.close()


@pytest.mark.parametrize("scheme,transcript", [(GWC, EVM), (SHPLONK, EVM), (GWC, BLAKE2B), (SHPLONK, BLAKE2B)])
def test_every_multiopen_and_transcript(ctx, zg, orc, scheme, transcript):
    pc = shuffle_circuits.three()
    s = Setup(orc, zg, ctx, pc)
    for obj in (s.prover, s.verifier):
        obj.set_multiopen(scheme)
        obj.set_transcript(transcript)
    (proof,) = s.prove([0], [5])
    assert len(proof) == proof_ref.proof_len(pc.cs, scheme=scheme, transcript=transcript)
    assert s.prover.proof_cap == proof_size(pc.cs, scheme, transcript) and (scheme == GWC or s.prover.proof_cap == len(proof))
    assert s.ref(proof, scheme=scheme, transcript=transcript).verdict == 1
    assert s.dev([proof]) == [1]
    bad = flip(proof, len(proof) - 40)
    assert s.ref(bad, scheme=scheme, transcript=transcript).verdict <= 0 and s.dev([bad])[0] <= 0
    (bad,) = s.prove([BAD], [5])
    assert s.ref(bad, BAD, scheme=scheme, transcript=transcript).verdict == 0 and s.dev([bad], [BAD]) == [0]
    s.close()


def test_split_domain_and_terms_by_degree_at_k14(ctx, zg, orc):
    """wide at k = 14 with a degree-6 gate: the split domain on and off and the terms by degree on and off give the bytes
    of the latency form"""
    pc = shuffle_circuits.wide(14, high_gate=True)
    s = Setup(orc, zg, ctx, pc)
    adv, inst = s.advice(0), pc.instance(0)
    proof = s.prover.prove(adv, inst, 3)
    assert len(proof) == proof_ref.proof_len(pc.cs) and s.dev([proof]) == [1] and s.ref(proof).verdict == 1
    s.prover.set_overlap(False)
    assert s.prover.quotient_terms()["active"]
    for by_degree in (True, False):
        s.prover.set_quotient_terms(by_degree)
        assert s.prover.prove(adv, inst, 3) == proof, by_degree
    s.close()
    zg.tuning_set("ZG_SPLIT_DOMAIN", 0)
    try:
        s2 = Setup(orc, zg, ctx, pc)
        s2.prover.set_overlap(False)
        assert not s2.prover.quotient_terms()["active"]
        assert s2.prover.prove(adv, inst, 3) == proof
        s2.close()
    finally:
        zg.tuning_set("ZG_SPLIT_DOMAIN", -1)


# ---------------------------------------------------------------------------------------------- no shuffles: nothing changes
def test_without_shuffles_the_new_entry_is_the_old_one(ctx, zg, orc):
    cs, asg, ilen = toy_circuit(5)
    img = cs.to_c()
    params = orc.params_new(cs.k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x1234567)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    st, want, _ = orc.create_proof(orc.ProvingKey(img, fixed, sigma, params, vk_repr), adv, inst, 7)
    assert st == 0
    counts = []
    for shuffles in (None, []):
        p = zg.Prover(ctx, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr, shuffles=(None, 0) if shuffles == [] else None)
        assert p.shuffles == 0
        assert p.prove(adv, inst, 7) == want
        ctx.profile(True)
        ctx.profile_collect()
        assert p.prove(adv, inst, 7) == want
        stats = ctx.profile_collect()
        ctx.profile(False)
        counts.append({name: v[0] for name, v in stats.items()})
        assert counts[-1] and not any(name.startswith("shuffle_") for name in counts[-1])
        p.close()
    assert counts[0] == counts[1]


# ---------------------------------------------------------------------------------------------- refusals and validation
def test_refusals_leave_the_prover_usable(ctx, zg, orc):
    pc = shuffle_circuits.plain()
    s = Setup(orc, zg, ctx, pc)
    s.prover.set_batch(2)
    adv, inst = s.advice(0), pc.instance(0)
    good = s.prover.prove(adv, inst, 4)

    def refused(call):
        with pytest.raises(zg.ZgError) as e:
            call()
        assert e.value.status == ZG_ERR_UNSUPPORTED and "shuffle" in str(e.value), str(e.value)
        assert s.prover.prove(adv, inst, 4) == good

    refused(lambda: s.prover.prove_multi([adv, adv], [inst, inst], [1, 2]))
    refused(lambda: s.verifier.verify_multi([good], [[inst, inst]], 1, 2))
    refused(lambda: s.prover.check(adv, inst))
    refused(lambda: s.prover.set_shard(0, 2, 0, lambda send, recv: None))
    zeros = np.zeros((1, pc.n, 4), np.uint64)
    one = orc.fr_from_int(1)
    refused(lambda: s.prover.evaluate_h(np.zeros((2, pc.n, 4), np.uint64), zeros[:0], zeros[:0], zeros[:0], zeros[:0], one, one, one, one,
                                        1 << pc.cs.extended_k()))
    # the image entries: no plan is at hand for this circuit and none is needed, the refusal comes before anything is asked
    # of the other arguments
    lib, h, one, none = ctx.lib, s.prover.h, ctypes.c_size_t(1), ctypes.c_size_t(0)
    refused(lambda: zg._check(lib.zg_prover_prove_images(h, None, None, one, None, None, none, None, None, None)))
    refused(lambda: zg._check(lib.zg_prover_prove_images_multi(h, None, None, one, None, None, none, None, None)))
    refused(lambda: zg._check(lib.zg_prover_check_images(h, None, None, one, None, None, none, None)))
    assert s.prover.prove_multi([adv], [inst], [4]) == good  # one circuit is the single proof
    s.close()


def test_create_validates_the_shuffles(ctx, zg, orc):
    pc = shuffle_circuits.plain()
    img = pc.cs.to_c()
    params = orc.params_new(pc.cs.k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x1234567)
    g, gl = params.g_np(), params.g_lagrange_np()
    fixed, sigma = pc.fixed_values(), pc.sigma_values()
    (ins, shs), nm = img.shuffles[0], img.c.n_monomials

    def create(shuffles, image=img):
        return zg.Prover(ctx, image, fixed, sigma, g, gl, vk_repr, shuffles=shuffles)

    def verifier(prover, shuffles):
        fc, sc = prover.vk_commitments()
        return zg.Verifier(ctx, img, fc, sc, g[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr, shuffles=shuffles)

    good = create(img.shuffles)
    adv, inst = pc.full_advice([], 0), pc.instance(0)
    proof = good.prove(adv, inst, 2)
    zero_width = zg.shuffle_array([(ins, shs)])
    zero_width[0][0].width = 0
    too_wide = zg.shuffle_array([(ins, shs)])
    too_wide[0][0].width = zg.MAX_LOOKUP_WIDTH + 1
    cases = [((None, 1), ZG_ERR_INVALID_ARG), (zero_width, ZG_ERR_INVALID_ARG), (too_wide, ZG_ERR_INVALID_ARG),
             ([(ins, [(nm, 1)])], ZG_ERR_INVALID_ARG), ([([(nm - 1, 2)], shs)], ZG_ERR_INVALID_ARG),
             ([(ins, shs)] * (zg.MAX_SHUFFLES + 1), ZG_ERR_UNSUPPORTED)]
    for shuffles, status in cases:
        with pytest.raises(zg.ZgError) as e:
            create(shuffles)
        assert e.value.status == status, (status, str(e.value))
        with pytest.raises(zg.ZgError) as e:
            verifier(good, shuffles)
        assert e.value.status == status, (status, str(e.value))
        assert good.prove(adv, inst, 2) == proof
    # a cs_degree smaller than the shuffles require: wide says 4, an image that says 3 is refused
    wide = shuffle_circuits.wide()
    wimg = wide.cs.to_c()
    wimg.c.cs_degree = 3
    with pytest.raises(zg.ZgError) as e:
        zg.Prover(ctx, wimg, wide.fixed_values(), wide.sigma_values(), g, gl, vk_repr, shuffles=wimg.shuffles)
    assert e.value.status == ZG_ERR_INVALID_ARG and "cs_degree" in str(e.value)
    with pytest.raises(zg.ZgError) as e:  # (the verifier asks the same, before it looks at the commitments)
        zg.Verifier(ctx, wimg, np.zeros((wimg.c.n_fixed, 8), np.uint64), np.zeros((0, 8), np.uint64), g[0], np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr,
                    shuffles=wimg.shuffles)
    assert e.value.status == ZG_ERR_INVALID_ARG and "cs_degree" in str(e.value)
    assert good.prove(adv, inst, 2) == proof
    top = create([(ins, shs)] * zg.MAX_SHUFFLES)  # the most there may be
    assert top.shuffles == zg.MAX_SHUFFLES
    top.close()
    good.close()
