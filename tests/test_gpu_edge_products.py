"""GPU parity for the field products taken off the edges of the hot kernels: the transform's constant factor (the ifft
divisor, the 2^5 of the `hat` form) riding on the inter-pass twiddle table, the pair start of the throughput MSM chains
(xyzz9_from_pair) and the theta-fold that starts from the first expression.  Every comparison is equality with the oracle."""
import numpy as np
import pytest
import torch

from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- transforms
@pytest.fixture(params=[1, 0], ids=["nine_limb", "eight_limb"])
def limb_form(request, zg):
    before = zg.tuning_get("ZG_NTT9")
    zg.tuning_set("ZG_NTT9", request.param)
    try:
        yield request.param
    finally:
        zg.tuning_set("ZG_NTT9", before)


_INVERSE_CASES = {}


def inverse_cases(zg, orc, log_n):
    """(name, input, oracle's lagrange_to_coeff) per input kind; computed once per size"""
    if log_n not in _INVERSE_CASES:
        n = 1 << log_n
        n2 = 1 << (log_n - log_n // 2)  # the inter-pass index is (j2, k1) with j = j1 * N2 + j2
        d = orc.domain(3, log_n)
        one = orc.fr_from_int(1)
        top = orc.fr_from_int(zg.FR_MODULUS - 1)

        def delta(at):
            e = np.zeros((n, 4), np.uint64)
            e[at] = one
            return e

        inputs = [("random", orc.fill_fr(4000 + log_n, n)), ("all r-1", np.tile(top, (n, 1))),
                  ("constant", np.tile(orc.fr_from_int(0xC0FFEE), (n, 1))), ("delta 0", delta(0)),
                  ("delta N2", delta(n2)), ("delta 1", delta(1))]
        _INVERSE_CASES[log_n] = d, [(name, a, orc.lagrange_to_coeff(d, a)) for name, a in inputs]
    return _INVERSE_CASES[log_n]


# 10: single pass (the divisor stays at the store); 11: smallest two-pass plan (5 + 6 stages); 14: the workload's n;
# 17: smallest plan on 2^11-element tiles
@pytest.mark.parametrize("log_n", [10, 11, 14, 17])
def test_inverse_transform_with_divisor(ctx, zg, orc, limb_form, log_n):
    d, cases = inverse_cases(zg, orc, log_n)
    omi, div = d.fe("omega_inv"), d.fe("ifft_divisor")
    for name, a, want in cases:
        got = ctx.ntt(a, omi, div)
        assert np.array_equal(got, want), name
        if name == "delta 0":  # every output is the divisor itself
            assert (got == div).all()
        if name == "constant":  # the only non-zero output is entry 0, whose inter-pass index is 0
            assert got[0].any() and not got[1:].any()
    # a second context of the same device shares the scaled tables
    c2 = zg.Ctx(0)
    try:
        for name, a, want in cases[:2]:
            assert np.array_equal(c2.ntt(a, omi, div), want), name
    finally:
        c2.close()


@pytest.mark.parametrize("log_n", [10, 11, 14])
def test_inverse_transform_batch_with_a_wide_stride(ctx, zg, orc, limb_form, log_n):
    d, cases = inverse_cases(zg, orc, log_n)
    n, stride, batch = 1 << log_n, (1 << log_n) + 24, 3
    pad = orc.fill_fr(99, stride - n)
    buf = np.zeros((batch, stride, 4), np.uint64)
    for b in range(batch):
        buf[b, :n] = cases[b][1]
        buf[b, n:] = pad
    t = torch.from_numpy(buf.view(np.int64)).cuda()
    ctx.ntt_batch_dev(t.data_ptr(), stride, batch, log_n, d.fe("omega_inv"), d.fe("ifft_divisor"))
    ctx.sync()
    got = t.cpu().numpy().view(np.uint64)
    for b in range(batch):
        assert np.array_equal(got[b, :n], cases[b][2]), cases[b][0]
        assert np.array_equal(got[b, n:], pad), "the gap between two arrays was written"


def test_more_divisors_than_a_size_keeps_tables_for(ctx, zg, orc, limb_form):
    """A size keeps a bounded number of scaled tables (csrc/ntt.hip MAX_SCALED_TABLES = 8); the divisors beyond them are
    applied at the store.  Both sides of that bound, and a second pass over the same divisors: d * NTT(a), entry by entry."""
    log_n, R = 19, zg.FR_MODULUS  # (a size no prover of the suite transforms at: its tables stay theirs)
    n = 1 << log_n
    a = orc.fill_fr(4300, n)
    _, omi = zg.domain_omega(log_n)
    plain = ctx.ntt(a, omi)
    at = [0, 1, 2, 63, 64, 65, n // 2, n - 1]
    base = [zg.fr_to_int(plain[i]) for i in at]
    for _ in range(2):
        for dv in range(3, 15):
            got = ctx.ntt(a, omi, orc.fr_from_int(dv))
            assert [zg.fr_to_int(got[i]) for i in at] == [v * dv % R for v in base], dv


# (8, 11): two-pass extended domain, single-pass n; (11, 14): two passes both ways.  out_len = 5 n: no power of two
@pytest.mark.parametrize("k", [8, 11])
def test_extended_domain_both_ways(ctx, zg, orc, limb_form, k):
    d = orc.domain(6, k)
    assert d.extended_k == k + 3 and d.quotient_poly_degree == 5
    n, out_len = 1 << k, 5 << k
    a = orc.fill_fr(4100 + k, n)
    h = orc.fill_fr(4200 + k, 1 << d.extended_k)
    want_ext, want_h = orc.coeff_to_extended(d, a), orc.extended_to_coeff(d, h)
    c2 = zg.Ctx(0)
    try:
        for c in (ctx, c2):
            ext = c.coeff_to_extended(a, k, d.extended_k)
            assert np.array_equal(ext, want_ext)
            assert np.array_equal(c.extended_to_coeff(h, k, d.extended_k, out_len), want_h)
            back = c.extended_to_coeff(ext, k, d.extended_k, out_len)
            assert np.array_equal(back[:n], a) and not back[n:].any()
    finally:
        c2.close()


# ---------------------------------------------------------------- the hat path (only reachable through a prover)
_PROOFS = {}


def circuit_and_proofs(orc, name):
    """circuit, key material and the oracle's proofs for seeds 21 and 22; computed once per circuit"""
    if name not in _PROOFS:
        if name == "wide_lookup":  # a width-2 lookup: the theta-fold from the second expression on
            k = 6
            cs, asg, ilen = variant_circuit(name, k=k)
        else:
            k = 11  # the smallest k whose n-point transforms take two passes
            cs, asg, ilen = toy_circuit(k, force_degree=6 if name == "toy degree 6" else None)
        img = cs.to_c()
        params = orc.params_new(k, 0xABCDEF)
        vk_repr = orc.fr_from_int(0x1234567)
        fixed, sigma = asg.fixed_values(), asg.sigma_values()
        pk = orc.ProvingKey(img, fixed, sigma, params, vk_repr)
        adv, inst = asg.advice_values(), asg.instance_values(ilen)
        want = []
        for seed in (21, 22):
            st, proof, _ = orc.create_proof(pk, adv, inst, seed)
            assert st == 0
            want.append(proof)
        _PROOFS[name] = (img, fixed, sigma, params, vk_repr, adv, inst, want, pk)
    return _PROOFS[name]


# "toy degree 6": (degree - 1) n = 4n + n, so the split extended domain really is two cosets, one of them n points
@pytest.mark.parametrize("name", ["toy", "toy degree 6", "wide_lookup"])
@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_two_proofs_in_both_forms(ctx, zg, orc, name, split):
    img, fixed, sigma, params, vk_repr, adv, inst, want, _pk = circuit_and_proofs(orc, name)
    before = zg.tuning_get("ZG_SPLIT_DOMAIN")
    zg.tuning_set("ZG_SPLIT_DOMAIN", split)  # (read when the prover is created)
    prover = None
    try:
        prover = zg.Prover(ctx, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr)
        prover.set_batch(2)
        for overlap in (False, True):
            prover.set_overlap(overlap)
            got, sts = prover.prove_batch([adv, adv], [inst, inst], [21, 22])
            assert sts == [0, 0]
            assert got[0] == want[0] and got[1] == want[1], (name, split, overlap)
    finally:
        zg.tuning_set("ZG_SPLIT_DOMAIN", before)
        if prover is not None:
            prover.close()


# ---------------------------------------------------------------- accumulation
@pytest.fixture(scope="module")
def pair_bases(zg, orc):
    """2^10 SRS points with, at neighbouring indices, the pairs a chain can start with"""
    gl = orc.params_new(12).g_lagrange_np()[: 1 << 10].copy()
    FQ = zg.FQ_MODULUS

    def neg(pt):
        out = pt.copy()
        out[4:] = zg.fq_from_int((FQ - zg.fq_to_int(pt[4:])) % FQ)
        return out

    b = gl.copy()
    b[1] = b[0]                                  # P, P
    b[3] = neg(b[2])                             # P, -P
    b[4] = 0                                     # identity, P
    b[7] = 0                                     # P, identity
    b[8:10] = 0                                  # identity, identity
    b[11], b[12] = b[10], neg(b[10])             # P, P, -P
    return b


@pytest.mark.parametrize("bit_table", [False, True], ids=["window_table", "bit_table"])
def test_throughput_chains_start_from_a_pair(zg, orc, pair_bases, bit_table):
    n, R = pair_bases.shape[0], zg.FR_MODULUS
    c2 = zg.Ctx(0)
    c2.set_msm_latency(False)
    try:
        bases = c2.register_bases(pair_bases)
        if bit_table:
            c2.enable_bit_table(bases, 9)
        same = np.tile(orc.fr_from_int(0x1234567), (n, 1))  # a bucket's first two entries are neighbouring bases
        pm = same.copy()
        pm[1::2] = orc.fr_from_int(R - 0x1234567)           # s, -s alternating
        vectors = [same, pm, np.tile(orc.fr_from_int(1), (n, 1)), np.tile(orc.fr_from_int(R - 1), (n, 1)),
                   orc.fill_fr(61, n), orc.fill_fr_sparse(62, n), np.zeros((n, 4), np.uint64)]
        got = c2.msm_batch(bases, np.stack(vectors))
        for v, sc in enumerate(vectors):
            assert np.array_equal(got[v], orc.msm(sc, pair_bases, threads=8)), (bit_table, v)
        for m in (1, 2, 3, 65):
            for sc in (orc.fill_fr(850 + m, m), np.tile(orc.fr_from_int(0x1234567), (m, 1))):
                assert np.array_equal(c2.msm(bases, sc), orc.msm(sc, pair_bases[:m], threads=4)), (bit_table, m)
        bases.free()
    finally:
        c2.close()
