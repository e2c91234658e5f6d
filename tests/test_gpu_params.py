"""An SRS without the toxic scalar: zg_params_lagrange (g_to_lagrange on the device, csrc/g1_fft.hip) against the oracle's
ParamsKZG::new and against a naive inverse DFT over G1, and zg_params_check (csrc/params.hip) on oracle SRSs and on files
broken in each way its `failed` bits name."""
import torch  # noqa: F401  (before anything loads the library: tests/conftest.py says why)

import ctypes

import numpy as np
import pytest

from circuits import toy_circuit

pytestmark = pytest.mark.gpu

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SEED = 0x5EED


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def affine(jac):
    """normalised Jacobian (orc.msm*, orc.normalise) -> affine, identity = (0, 0)"""
    return np.zeros(8, np.uint64) if not jac[8:].any() else jac[:8].copy()


def naive_lagrange(orc, g, k):
    """Row i of the inverse DFT: scalars omega^(-ij) 2^-k as Python integers, orc.msm_naive against g."""
    n = 1 << k
    omega_inv = pow(pow(pow(7, (R - 1) >> 28, R), 1 << (28 - k), R), -1, R)
    ninv = pow(n, -1, R)
    out = np.zeros((n, 8), np.uint64)
    for i in range(n):
        sc = np.stack([orc.fr_from_int(pow(omega_inv, i * j, R) * ninv % R) for j in range(n)])
        out[i] = affine(orc.msm_naive(sc, g[:n]))
    return out


def neg(orc, p):
    o = p.copy()
    y = np.ascontiguousarray(p[4:8])
    t = np.zeros(4, np.uint64)
    orc.load().orc_fq_neg(_p(t), _p(y))
    o[4:8] = t
    return o


def jac(orc, p):
    out = np.zeros(12, np.uint64)
    orc.load().orc_g1_from_affine(_p(out), _p(np.ascontiguousarray(p)))
    return out


def g1_add_affine(orc, p, q):
    return affine(orc.normalise(orc.g1_add(jac(orc, p), jac(orc, q))))


@pytest.fixture(scope="module")
def srs(orc):
    """oracle SRSs by k, made once and left alone: k -> (g, g_lagrange, g2, s_g2)"""
    cache = {}

    def get(k, seed=SEED):
        if (k, seed) not in cache:
            prm = orc.params_new(k, seed)
            cache[(k, seed)] = (prm.g_np(), prm.g_lagrange_np(), np.array(prm.g2, np.uint64), np.array(prm.s_g2, np.uint64))
        return cache[(k, seed)]

    return get


# ------------------------------------------------------------------ the transform
@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 6])
def test_lagrange_small_k_matches_oracle_and_naive(ctx, orc, srs, k):
    g, gl, _, _ = srs(k)
    got = ctx.params_lagrange(k, g)
    assert np.array_equal(got, gl)
    assert np.array_equal(got, naive_lagrange(orc, g, k))


def test_lagrange_arbitrary_points_against_naive(ctx, orc, srs):
    """equal points, identities and P / -P pairs in the input: additions that are doublings or cancellations"""
    k = 5
    g = srs(k)[0].copy()
    g[1] = g[0]
    g[7] = g[6]
    g[16] = g[0]
    g[2] = 0
    g[18] = 0
    g[10] = neg(orc, g[9])
    g[20] = neg(orc, g[4])
    assert np.array_equal(ctx.params_lagrange(k, g), naive_lagrange(orc, g, k))


def test_lagrange_constant_input(ctx, srs):
    """g = [P, P, ...] -> [P, inf, inf, ...]: every first-pass butterfly is a doubling (a = t) and a cancellation (a = -t)"""
    k = 7
    p = srs(k)[0][3]
    got = ctx.params_lagrange(k, np.tile(p, (1 << k, 1)))
    assert np.array_equal(got[0], p)
    assert not got[1:].any()


def test_lagrange_all_identities(ctx):
    k = 6
    assert not ctx.params_lagrange(k, np.zeros((1 << k, 8), np.uint64)).any()


@pytest.mark.parametrize("k", [10, 12])
def test_lagrange_larger_k_matches_oracle(ctx, srs, k):
    g, gl, _, _ = srs(k)
    assert np.array_equal(ctx.params_lagrange(k, g), gl)


@pytest.fixture(scope="module")
def downsized(ctx, orc, srs):
    """(g prefix of the k = 10 SRS, its own params_lagrange(8) output, the oracle's k = 8 parameters for the same scalar)"""
    g10 = srs(10)[0]
    small = orc.params_from_scalar(8, orc.fill_fr(SEED, 1)[0])
    return g10[:256].copy(), ctx.params_lagrange(8, g10), small


def test_downsize(srs, downsized):
    g8, gl8, small = downsized
    assert np.array_equal(g8, small.g_np())
    assert np.array_equal(gl8, small.g_lagrange_np())


def test_lagrange_device_path(ctx, orc, srs):
    k = 10
    n = 1 << k
    g, gl, _, _ = srs(k)
    d_g = torch.from_numpy(g.view(np.int64).reshape(-1).copy()).cuda()
    d_gl = torch.full((n * 8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.params_lagrange_dev(k, d_g.data_ptr(), d_gl.data_ptr())
    bases = ctx.register_bases_dev(d_gl.data_ptr(), n)  # (ordered behind the transform on the context stream)
    ev = orc.fill_fr(77, n)
    assert np.array_equal(ctx.msm(bases, ev), orc.msm(ev, gl, threads=8))  # commit_lagrange
    bases.free()
    ctx.sync()
    got = d_gl.cpu().numpy().view(np.uint64).reshape(n, 8)
    assert np.array_equal(got, ctx.params_lagrange(k, g))
    assert np.array_equal(got, gl)


def test_lagrange_errors(ctx, zg, srs):
    small = np.zeros((2, 8), np.uint64)
    st = ctx.lib.zg_params_lagrange(ctx.h, ctypes.c_uint32(25), _p(small), _p(small))  # (refused before anything is read)
    assert st == -4  # ZG_ERR_UNSUPPORTED
    d = torch.zeros(32 * 8, dtype=torch.int64, device="cuda")
    with pytest.raises(zg.ZgError) as e:
        ctx.params_lagrange_dev(5, d.data_ptr(), d.data_ptr())
    assert e.value.status == -1
    st = ctx.lib.zg_params_lagrange_dev(ctx.h, ctypes.c_uint32(25), ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(d.data_ptr() + 64))
    assert st == -4
    assert ctx.lib.zg_params_lagrange(ctx.h, ctypes.c_uint32(3), None, _p(small)) == -1
    g, gl, _, _ = srs(5)
    assert np.array_equal(ctx.params_lagrange(5, g), gl)  # the context still works


# ------------------------------------------------------------------ the check
K = 6


@pytest.mark.parametrize("k", [0, 1, 6, 10])
def test_check_accepts_oracle_srs(ctx, srs, k):
    g, gl, g2, s_g2 = srs(k)
    assert ctx.params_check(k, g, gl, g2, s_g2, 41) == (1, 0)
    assert ctx.params_check(k, g, None, g2, s_g2, 42) == (1, 0)


def test_check_accepts_downsized_pair(ctx, srs, downsized):
    g8, gl8, _ = downsized
    _, _, g2, s_g2 = srs(10)
    assert ctx.params_check(8, g8, gl8, g2, s_g2, 43) == (1, 0)


def fq2_neg_y(zg, pt):
    o = pt.copy()
    for c in (8, 12):
        o[c:c + 4] = zg.fq_from_int(Q - zg.fq_to_int(pt[c:c + 4]))
    return o


def test_check_powers_relation(ctx, zg, srs):
    g, gl, g2, s_g2 = srs(K)
    bad = g.copy()
    bad[5] = bad[6]
    assert ctx.params_check(K, bad, None, g2, s_g2, 1) == (0, zg.SRS_POWERS)
    other = srs(K, 0x777)[3]
    assert ctx.params_check(K, g, gl, g2, other, 2) == (0, zg.SRS_POWERS)
    assert ctx.params_check(K, g, gl, g2, fq2_neg_y(zg, s_g2), 3) == (0, zg.SRS_POWERS)
    assert "powers" in zg.load().zg_last_error().decode()


def test_check_powers_weights_are_random(ctx, zg, orc, srs):
    """g[3] += D and g[4] -= D cancel in sum g[i] and in sum g[i+1]: unit weights would accept them"""
    g, _, g2, s_g2 = srs(K)
    d = g[9]
    bad = g.copy()
    bad[3] = g1_add_affine(orc, g[3], d)
    bad[4] = g1_add_affine(orc, g[4], neg(orc, d))
    for key in (5, 6):
        assert ctx.params_check(K, bad, None, g2, s_g2, key) == (0, zg.SRS_POWERS)


def test_check_lagrange_relation(ctx, zg, srs):
    g, gl, g2, s_g2 = srs(K)
    bad = gl.copy()
    bad[[11, 40]] = bad[[40, 11]]
    assert ctx.params_check(K, g, bad, g2, s_g2, 7) == (0, zg.SRS_LAGRANGE)
    assert ctx.params_check(K, g, srs(7)[1][:64], g2, s_g2, 8) == (0, zg.SRS_LAGRANGE)


def test_check_malformed_g1(ctx, zg, srs):
    g, gl, g2, s_g2 = srs(K)
    bad = g.copy()
    bad[7, 4] += np.uint64(1)  # a y limb: off the curve
    assert ctx.params_check(K, bad, gl, g2, s_g2, 9) == (0, zg.SRS_G1_MALFORMED)
    assert "g[7]" in zg.load().zg_last_error().decode()
    bad = g.copy()
    bad[12, 0:4] = zg.int_to_limbs(Q)  # the limbs of q: not below q
    bad[30, 4:8] = zg.int_to_limbs(Q)
    assert ctx.params_check(K, bad, None, g2, s_g2, 10) == (0, zg.SRS_G1_MALFORMED)
    assert "g[12]" in zg.load().zg_last_error().decode()
    badl = gl.copy()
    badl[3, 0] += np.uint64(1)
    assert ctx.params_check(K, g, badl, g2, s_g2, 11) == (0, zg.SRS_G1_MALFORMED)
    assert "g_lagrange[3]" in zg.load().zg_last_error().decode()


def test_check_identity_in_g(ctx, zg, srs):
    g, gl, g2, s_g2 = srs(K)
    bad = g.copy()
    bad[0] = 0
    assert ctx.params_check(K, bad, gl, g2, s_g2, 12) == (0, zg.SRS_G1_IDENTITY)
    assert "g[0]" in zg.load().zg_last_error().decode()


# Fq2 = Fq[u]/(u^2 + 1) on Python integers, for a point of the twist outside the r-torsion
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * d % Q, -a[1] * d % Q)


def fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)  # q = 3 mod 4
    return r if r * r % Q == a % Q else None


def f2sqrt(a):
    if a[1] == 0:
        r = fq_sqrt(a[0])
        if r is not None:
            return (r, 0)
        return (0, fq_sqrt(-a[0] % Q))
    alpha = fq_sqrt((a[0] * a[0] + a[1] * a[1]) % Q)
    if alpha is None:
        return None
    for sign in (1, -1):
        delta = (a[0] + sign * alpha) * pow(2, -1, Q) % Q
        x0 = fq_sqrt(delta)
        if x0 is not None and x0 != 0:
            r = (x0, a[1] * pow(2 * x0, -1, Q) % Q)
            if f2mul(r, r) == (a[0] % Q, a[1] % Q):
                return r
    return None


def twist_point_outside_subgroup(zg, orc):
    b = f2mul((3, 0), f2inv((9, 1)))
    x0 = 1
    while True:
        x = (x0, 0)
        rhs = f2mul(f2mul(x, x), x)
        rhs = ((rhs[0] + b[0]) % Q, (rhs[1] + b[1]) % Q)
        y = f2sqrt(rhs)
        if y is not None:
            break
        x0 += 1
    pt = np.concatenate([zg.fq_from_int(c) for c in (x[0], x[1], y[0], y[1])]).astype(np.uint64)
    L = orc.load()
    assert L.orc_g2a_on_curve(_p(pt)) == 1
    # r * Q = (r - 1) * Q + Q is not the identity (the cofactor is ~2^254: a point found this way is outside the subgroup)
    t, s = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
    L.orc_g2a_mul(_p(t), _p(pt), _p(orc.fr_from_int(R - 1)))
    L.orc_g2a_add(_p(s), _p(t), _p(pt))
    assert L.orc_g2a_is_identity(_p(s)) == 0
    return pt


def test_check_bad_g2(ctx, zg, orc, srs):
    g, gl, g2, s_g2 = srs(K)
    off = s_g2.copy()
    off[8] += np.uint64(1)
    assert ctx.params_check(K, g, gl, g2, off, 13) == (0, zg.SRS_G2)
    assert "s_g2" in zg.load().zg_last_error().decode()
    assert ctx.params_check(K, g, gl, g2, np.zeros(16, np.uint64), 14) == (0, zg.SRS_G2)
    noncanonical = s_g2.copy()
    noncanonical[0:4] = zg.int_to_limbs(Q)
    assert ctx.params_check(K, g, gl, g2, noncanonical, 15) == (0, zg.SRS_G2)
    outside = twist_point_outside_subgroup(zg, orc)
    assert ctx.params_check(K, g, gl, g2, outside, 16) == (0, zg.SRS_G2)
    assert "subgroup" in zg.load().zg_last_error().decode()
    assert ctx.params_check(K, g, gl, outside, s_g2, 17) == (0, zg.SRS_G2)


def test_check_flags_are_independent(ctx, zg, srs):
    g, gl, g2, s_g2 = srs(K)
    other = srs(K, 0x777)[3]
    swapped = gl.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    assert ctx.params_check(K, g, swapped, g2, other, 18) == (0, zg.SRS_POWERS | zg.SRS_LAGRANGE)
    # a malformed point and a bad G2 point are both named; the relations are then not evaluated
    bad = g.copy()
    bad[7, 4] += np.uint64(1)
    bad[9] = 0
    assert ctx.params_check(K, bad, swapped, g2, np.zeros(16, np.uint64), 19) == (0, zg.SRS_G1_MALFORMED | zg.SRS_G1_IDENTITY | zg.SRS_G2)
    assert ctx.params_check(K, g, gl, g2, s_g2, 20) == (1, 0)


# ------------------------------------------------------------------ end to end
def test_srs_file_to_verified_proof(ctx, zg, orc, srs, tmp_path):
    """A k = 8 SRS file serves a k = 6 circuit: checked, downsized on the device, proved against and verified."""
    import formats

    g8, gl8, g2_8, s_g2_8 = srs(8)
    path = str(tmp_path / "srs.bin")
    formats.write_srs(path, 8, g8, gl8, g2_8, s_g2_8)
    k, g, gl, g2, s_g2 = formats.read_srs(path)
    assert k == 8
    assert ctx.params_check(k, g, gl, g2, s_g2, 99) == (1, 0)
    kc = 6
    gl6 = ctx.params_lagrange(kc, g)
    bases_g = ctx.register_bases(np.asarray(g[:1 << kc]))
    bases_gl = ctx.register_bases(gl6)
    cs, asg, ilen = toy_circuit(kc)
    img = cs.to_c()
    vk_repr = orc.fr_from_int(0x1234567)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    prover = zg.Prover(ctx, img, fixed, sigma, bases_g, bases_gl, vk_repr)
    proof = prover.prove(adv, inst, 5)
    pk = orc.ProvingKey(img, fixed, sigma, orc.params_from_scalar(kc, orc.fill_fr(SEED, 1)[0]), vk_repr)
    st, want, _ = orc.create_proof(pk, adv, inst, 5)
    assert st == 0 and proof == want
    fc, sc = prover.vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sc, np.asarray(g[0]), g2, s_g2, vk_repr)
    assert verifier.verify([proof], [inst], 6) == [1]
    verifier.close()
    prover.close()
    bases_g.free()
    bases_gl.free()
