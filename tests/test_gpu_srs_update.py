"""One contribution to an updatable SRS (csrc/srs_update.hip): zg_params_update / _dev against the oracle's
ParamsKZG::new of the product scalar, zg_params_check_update on honest steps and on steps broken in each way its bits
name, and a two-contribution SRS, made and checked by the library alone, that a proof is made and verified under.
Every comparison is equality of bytes."""
import torch  # noqa: F401  (before anything loads the library: tests/conftest.py says why)

import ctypes
import random

import numpy as np
import pytest

import srs_cases as sc
from circuits import toy_circuit

pytestmark = pytest.mark.gpu

R = sc.R
S = 0x1D0C5EED0123456789ABCDEF02468ACE13579BDF0FEDCBA9876543210F00DFACE % R  # the scalar of the string a step starts from
OMEGA4 = pow(7, (R - 1) // 4, R)  # a primitive 4th root of unity: its powers cycle through 1, w, -1, -w
T_RANDOM = random.Random(31).randrange(1, R)
TS = {"1": 1, "2": 2, "r-1": R - 1, "omega4": OMEGA4, "random": T_RANDOM}


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def srs(orc):
    """oracle parameters by (k, scalar), made once and left alone: -> (g, g_lagrange, g2, s_g2)"""
    cache = {}

    def get(k, s):
        s %= R
        if (k, s) not in cache:
            prm = orc.params_from_scalar(k, orc.fr_from_int(s))
            cache[(k, s)] = (prm.g_np(), prm.g_lagrange_np(), np.array(prm.g2, np.uint64), np.array(prm.s_g2, np.uint64))
        return cache[(k, s)]

    return get


def test_constants():
    assert pow(OMEGA4, 4, R) == 1 and pow(OMEGA4, 2, R) == R - 1


# ------------------------------------------------------------------ the update
@pytest.mark.parametrize("tname", list(TS))
@pytest.mark.parametrize("k", [0, 1, 5, 6, 7, 10])
def test_update_equals_the_oracle_of_the_product_scalar(ctx, zg, srs, k, tname):
    t = TS[tname]
    g, gl, g2, s_g2 = srs(k, S)
    want_g, want_gl, want_g2, want_s_g2 = srs(k, S * t)
    g_out, gl_out, s_g2_out, record = ctx.params_update(k, sc.fr_mont(t), g, g2, s_g2)
    assert np.array_equal(g_out, want_g)
    assert np.array_equal(gl_out, want_gl)
    assert np.array_equal(s_g2_out, want_s_g2) and np.array_equal(g2, want_g2)
    # the record: t * g[0] and t * g2, which are g[1] and s_g2 of the string of t itself
    assert np.array_equal(record[:8], srs(1, t)[0][1])
    assert np.array_equal(record[8:], srs(1, t)[3])
    if t == 1:
        assert np.array_equal(g_out, g) and np.array_equal(gl_out, gl) and np.array_equal(s_g2_out, s_g2)
    # without the Lagrange leg: the same g
    g_only, none, _, _ = ctx.params_update(k, sc.fr_mont(t), g, g2, s_g2, lagrange=False)
    assert none is None and np.array_equal(g_only, want_g)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def from_dev(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 8)


def test_device_form_in_place_equals_the_host_form(ctx, srs):
    k, t = 7, T_RANDOM
    n = 1 << k
    g, _, g2, s_g2 = srs(k, S)
    g_host, gl_host, _, _ = ctx.params_update(k, sc.fr_mont(t), g, g2, s_g2)
    d_g = to_dev(g)
    d_gl = torch.full((n * 8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.params_update_dev(k, sc.fr_mont(t), d_g.data_ptr(), d_g.data_ptr(), d_gl.data_ptr())
    ctx.sync()
    assert np.array_equal(from_dev(d_g), g_host) and np.array_equal(from_dev(d_gl), gl_host)
    # out of place, no Lagrange leg: the input stays
    d_in, d_out = to_dev(g), torch.full((n * 8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.params_update_dev(k, sc.fr_mont(t), d_in.data_ptr(), d_out.data_ptr())
    ctx.sync()
    assert np.array_equal(from_dev(d_in), g) and np.array_equal(from_dev(d_out), g_host)


def test_two_steps_equal_one_step_of_the_product(ctx, srs):
    k, t1, t2 = 6, T_RANDOM, OMEGA4 + 12345
    g, _, g2, s_g2 = srs(k, S)
    g1, _, s1, _ = ctx.params_update(k, sc.fr_mont(t1), g, g2, s_g2)
    g12, gl12, s12, _ = ctx.params_update(k, sc.fr_mont(t2), g1, g2, s1)
    one = ctx.params_update(k, sc.fr_mont(t1 * t2 % R), g, g2, s_g2)
    assert np.array_equal(g12, one[0]) and np.array_equal(gl12, one[1]) and np.array_equal(s12, one[2])


def test_refused_scalars_leave_the_outputs_alone(ctx, zg, srs):
    k = 5
    n = 1 << k
    g, _, g2, s_g2 = srs(k, S)
    mark = np.uint64(0x5A5A5A5A5A5A5A5A)
    for bad in (np.zeros(4, np.uint64), sc.fr_raw_limbs(R), sc.fr_raw_limbs((1 << 256) - 1)):
        g_out, gl_out = np.full((n, 8), mark), np.full((n, 8), mark)
        s_out, rec = np.full(16, mark), np.full(24, mark)
        st = ctx.lib.zg_params_update(ctx.h, ctypes.c_uint32(k), _p(bad), _p(g), _p(g2), _p(s_g2), _p(g_out), _p(gl_out), _p(s_out), _p(rec))
        assert st == -1
        assert (g_out == mark).all() and (gl_out == mark).all() and (s_out == mark).all() and (rec == mark).all()
        d_g = to_dev(g)
        torch.cuda.synchronize()
        with pytest.raises(zg.ZgError) as e:
            ctx.params_update_dev(k, bad, d_g.data_ptr(), d_g.data_ptr())
        assert e.value.status == -1
        ctx.sync()
        assert np.array_equal(from_dev(d_g), g)
    st = ctx.lib.zg_params_update(ctx.h, ctypes.c_uint32(25), _p(sc.fr_mont(2)), _p(g), _p(g2), _p(s_g2), _p(g_out), None, _p(s_out), _p(rec))
    assert st == -4 and (g_out == mark).all()


# ------------------------------------------------------------------ the check
@pytest.fixture(scope="module")
def step(ctx, srs):
    """honest steps by k: (prev g, g_next, g_lagrange_next, g2, s_g2_next, record); made once, left alone"""
    cache = {}

    def get(k, t=T_RANDOM):
        if (k, t) not in cache:
            g, _, g2, s_g2 = srs(k, S)
            g_out, gl_out, s_g2_out, record = ctx.params_update(k, sc.fr_mont(t), g, g2, s_g2)
            cache[(k, t)] = (g, g_out, gl_out, g2, s_g2_out, record)
        return cache[(k, t)]

    return get


@pytest.mark.parametrize("k", [1, 6, 10])
def test_check_accepts_the_honest_step(ctx, step, k):
    g, g_next, gl_next, g2, s_g2_next, record = step(k)
    assert ctx.params_check_update(k, g[:2], g_next, gl_next, g2, s_g2_next, record, 51) == (1, 0)
    assert ctx.params_check_update(k, g[:2], g_next, None, g2, s_g2_next, record, 52) == (1, 0)


K = 6


def test_check_rejects_a_record_of_another_scalar(ctx, zg, step):
    g, g_next, gl_next, g2, s_g2_next, _ = step(K)
    other = step(K, 2)[5]  # a consistent record, of t = 2
    assert ctx.params_check_update(K, g[:2], g_next, gl_next, g2, s_g2_next, other, 53) == (0, zg.SRS_UPDATE_LINK)
    assert "previous g[1]" in zg.load().zg_last_error().decode()


def test_check_rejects_bad_record_points(ctx, zg, orc, step):
    from test_gpu_params import twist_point_outside_subgroup

    g, g_next, gl_next, g2, s_g2_next, record = step(K)

    def verdict(rec, key):
        return ctx.params_check_update(K, g[:2], g_next, gl_next, g2, s_g2_next, rec, key)

    ident = record.copy()
    ident[8:] = 0
    assert verdict(ident, 54) == (0, zg.SRS_UPDATE_LINK)
    off = record.copy()
    off[8 + 8] ^= np.uint64(1)  # y.c0 of t_g2
    assert verdict(off, 55) == (0, zg.SRS_UPDATE_LINK)
    outside = record.copy()
    outside[8:] = twist_point_outside_subgroup(zg, orc)
    assert verdict(outside, 56) == (0, zg.SRS_UPDATE_LINK)
    assert "subgroup" in zg.load().zg_last_error().decode()
    # t_g1 of another scalar than t_g2's; not a point; the identity
    mixed = record.copy()
    mixed[:8] = step(K, 2)[5][:8]
    assert verdict(mixed, 57) == (0, zg.SRS_UPDATE_LINK)
    assert "same multiple" in zg.load().zg_last_error().decode()
    offcurve = record.copy()
    offcurve[4] ^= np.uint64(1)
    assert verdict(offcurve, 58) == (0, zg.SRS_UPDATE_LINK)
    noident = record.copy()
    noident[:8] = 0
    assert verdict(noident, 59) == (0, zg.SRS_UPDATE_LINK)
    assert verdict(record, 60) == (1, 0)


def test_check_rejects_a_changed_string(ctx, zg, step, srs):
    g, g_next, gl_next, g2, s_g2_next, record = step(K)
    # g_next[0] is no longer the previous g[0]: the base bit (and g_next is no sequence of powers any more)
    moved = g_next.copy()
    moved[0] = g_next[3]
    assert ctx.params_check_update(K, g[:2], moved, None, g2, s_g2_next, record, 61) == (0, zg.SRS_POWERS | zg.SRS_UPDATE_BASE)
    # ... or the caller names another previous string
    other_prev = srs(K, S + 1)[0][:2].copy()
    other_prev[0] = g[5]
    v, failed = ctx.params_check_update(K, other_prev, g_next, gl_next, g2, s_g2_next, record, 62)
    assert v == 0 and failed & zg.SRS_UPDATE_BASE
    # one tampered point further up: the powers relation of zg_params_check
    tampered = g_next.copy()
    tampered[5] = tampered[6]
    assert ctx.params_check_update(K, g[:2], tampered, None, g2, s_g2_next, record, 63) == (0, zg.SRS_POWERS)
    # s_g2_next of another scalar
    assert ctx.params_check_update(K, g[:2], g_next, gl_next, g2, srs(K, S + 1)[3], record, 64) == (0, zg.SRS_POWERS)
    # g_next[1] moved alone: powers AND link
    second = g_next.copy()
    second[1] = g_next[2]
    assert ctx.params_check_update(K, g[:2], second, None, g2, s_g2_next, record, 65) == (0, zg.SRS_POWERS | zg.SRS_UPDATE_LINK)
    # the step not applied at all (next = prev) under the record of a real step
    assert ctx.params_check_update(K, g[:2], g, None, g2, srs(K, S)[3], record, 66) == (0, zg.SRS_UPDATE_LINK)


def test_check_of_k0_is_an_argument_error(ctx, step, srs):
    g, _, g2, s_g2 = srs(0, S)
    record = step(1)[5]
    two = np.concatenate([g, g])
    verdict, failed = ctypes.c_int(-7), ctypes.c_uint32(77)
    st = ctx.lib.zg_params_check_update(ctx.h, ctypes.c_uint32(0), _p(two), _p(g), None, _p(g2), _p(s_g2), _p(record),
                                        (5).to_bytes(32, "little"), ctypes.byref(verdict), ctypes.byref(failed))
    assert st == -1 and verdict.value == -7 and failed.value == 77


# ------------------------------------------------------------------ end to end
def test_two_contributions_make_an_srs_a_proof_verifies_under(ctx, zg, orc, srs, tmp_path):
    """zg_params_new(s = 1) -> two contributions, each checked -> an SRS file written from the library's own g2 / s_g2 ->
    a k = 6 proof from that file, accepted by the library's verifier and by the oracle's pairing verifier."""
    import formats

    k = 6
    t1, t2 = random.Random(61).randrange(1, R), random.Random(62).randrange(1, R)
    g, _ = ctx.params_new(k, sc.fr_mont(1))  # (g_lagrange of s = 1 is not used: every update makes its own)
    g2, s_g2 = zg.params_g2(sc.fr_mont(1))
    assert np.array_equal(g2, s_g2) and (g == g[0]).all()
    gl = None
    for step_no, t in enumerate((t1, t2)):
        g_next, gl, s_g2_next, record = ctx.params_update(k, sc.fr_mont(t), g, g2, s_g2)
        assert ctx.params_check_update(k, g[:2], g_next, gl, g2, s_g2_next, record, 70 + step_no) == (1, 0)
        g, s_g2 = g_next, s_g2_next
    want = srs(k, t1 * t2)
    assert all(np.array_equal(a, b) for a, b in zip((g, gl, g2, s_g2), want))
    path = str(tmp_path / "srs.bin")
    formats.write_srs(path, k, g, gl, g2, s_g2)
    k_f, g_f, gl_f, g2_f, s_g2_f = formats.read_srs(path)
    assert k_f == k
    cs, asg, ilen = toy_circuit(k)
    img = cs.to_c()
    vk_repr = orc.fr_from_int(0x7654321)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    prover = zg.Prover(ctx, img, fixed, sigma, np.array(g_f), np.array(gl_f), vk_repr)
    proof = prover.prove(adv, inst, 9)
    fc, sgc = prover.vk_commitments()
    verifier = zg.Verifier(ctx, img, fc, sgc, np.asarray(g_f[0]), g2_f, s_g2_f, vk_repr)
    pk = orc.ProvingKey(img, fixed, sigma, orc.params_from_scalar(k, orc.fr_from_int(t1 * t2 % R)), vk_repr)
    wrong = inst.copy()
    wrong[0, 0] = orc.fr_from_int(orc.fr_to_int(wrong[0, 0]) + 1)
    assert verifier.verify([proof, proof], [inst, wrong], 10) == [1, 0]
    assert orc.verify_proof_pairing(pk, inst, proof) == 1
    assert orc.verify_proof_pairing(pk, wrong, proof) != 1
    verifier.close()
    prover.close()
