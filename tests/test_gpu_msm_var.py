"""GPU parity of zg_msm_var* -- multiexp over points that are NOT registered -- with the oracle's restatement of halo2's
best_multiexp (orc.msm) and with the naive sum (orc.msm_naive).  Every comparison is equality of normalised points: the
arithmetic is exact.  Points come from orc.params_new(12), re-arranged in numpy."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before anything loads the library: tests/conftest.py says why)

pytestmark = pytest.mark.gpu

N = 4096


@pytest.fixture(scope="module")
def g(orc):
    a = orc.params_new(12).g_np()
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def uniform(orc):
    a = orc.fill_fr(2101, N)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def want_uniform(orc, g, uniform):
    """orc.msm of the first n uniform scalars, computed once per size"""
    memo = {}

    def at(n):
        if n not in memo:
            memo[n] = orc.msm(uniform[:n], g[:n], threads=8)
        return memo[n]

    return at


def is_identity(zg, r):
    return not r[:4].any() and not r[8:].any() and zg.fq_to_int(r[4:8]) == 1


def neg(zg, pt):
    """(x, q - y) on the Montgomery limbs of y: the Montgomery form is linear"""
    out = pt.copy()
    out[4:] = zg.int_to_limbs(zg.FQ_MODULUS - zg.limbs_to_int(pt[4:]))
    return out


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096])
def test_sizes_match_the_oracle(ctx, g, uniform, want_uniform, n):
    assert np.array_equal(ctx.msm_var(g[:n], uniform[:n]), want_uniform(n))


def test_no_points_give_the_identity(ctx, zg, g):
    assert is_identity(zg, ctx.msm_var(g[:0], np.zeros((0, 4), np.uint64)))
    out = ctx.msm_var_batch(g[:0], np.zeros((3, 0, 4), np.uint64))
    assert out.shape == (3, 12) and all(is_identity(zg, r) for r in out)
    # batch = 0: ZG_OK, nothing written
    assert ctx.lib.zg_msm_var_batch(ctx.h, None, None, 0, 5, 0, None) == 0


# ---- 2. widths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 3, 7, 8, 13, 16])
def test_every_width_gives_the_same_bytes(ctx, g, uniform, want_uniform, c):
    assert np.array_equal(ctx.msm_var(g[:1000], uniform[:1000], c), want_uniform(1000))


@pytest.mark.parametrize("c", [9, 10, 11, 12])
def test_widths_at_which_the_reduction_changes_its_strips(ctx, g, uniform, want_uniform, c):
    """msm_var_strip walks 1, 2, 4 and 8 buckets per lane at these widths (256 lanes of msm_var_strip_sum per bucket set)"""
    assert np.array_equal(ctx.msm_var(g[:1000], uniform[:1000], c), want_uniform(1000))


@pytest.mark.parametrize("c", [2, 16])
def test_widths_when_every_window_carries(ctx, zg, orc, g, c):
    mx = np.tile(orc.fr_from_int(zg.FR_MODULUS - 1), (65, 1))
    assert np.array_equal(ctx.msm_var(g[:65], mx, c), orc.msm(mx, g[:65], threads=4))


# ---- 3. edge scalars at n = 4096 -----------------------------------------------------------------------------------------
def test_edge_scalars(ctx, zg, orc, g):
    assert is_identity(zg, ctx.msm_var(g, np.zeros((N, 4), np.uint64)))
    ones = np.tile(orc.fr_from_int(1), (N, 1))  # every point in ONE bucket of window 0
    assert np.array_equal(ctx.msm_var(g, ones), orc.msm(ones, g, threads=8))
    mx = np.tile(orc.fr_from_int(zg.FR_MODULUS - 1), (N, 1))
    assert np.array_equal(ctx.msm_var(g, mx), orc.msm(mx, g, threads=8))
    for idx in (0, 1, N - 1):
        e = np.zeros((N, 4), np.uint64)
        e[idx] = orc.fr_from_int(1)
        r = ctx.msm_var(g, e)
        assert np.array_equal(r[:8], g[idx]) and zg.fq_to_int(r[8:]) == 1, idx
    sp = orc.fill_fr_sparse(2105, N)
    assert np.array_equal(ctx.msm_var(g, sp), orc.msm(sp, g, threads=8))


def test_a_bucket_beyond_the_task_cap(ctx, orc, g):
    """more than 16 * 1024 points in ONE bucket (scalar 1 everywhere): the bucket's tasks grow past 16 points instead of
    multiplying; the points are the 4096 five times over, so every point also occurs five times"""
    pts = np.tile(g, (5, 1))
    ones = np.tile(orc.fr_from_int(1), (pts.shape[0], 1))
    want = orc.msm(ones, pts, threads=8)
    assert np.array_equal(want, orc.msm(np.tile(orc.fr_from_int(5), (N, 1)), g, threads=8))
    assert np.array_equal(ctx.msm_var(pts, ones), want)


# ---- 4. edge bases at n = 1024 -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_bases(zg, g):
    """an identity, 64 and 56 copies of one point, a P / -P pair, among distinct points (the set the judge was checked on)"""
    n = 1024
    b = g[:n].copy()
    b[5] = 0
    b[100:164] = g[100]
    b[300:412:2] = g[100]
    assert (b == g[100]).all(axis=1).sum() == 64 + 56
    b[10] = g[11]
    b[11] = neg(zg, g[11])
    b.setflags(write=False)
    return b


def test_edge_bases(ctx, zg, orc, g, uniform, edge_bases):
    n = edge_bases.shape[0]
    ones = np.tile(orc.fr_from_int(1), (n, 1))
    for s in (uniform[:n], ones):
        want = orc.msm(s, edge_bases, threads=8)
        assert np.array_equal(want, orc.msm_naive(s, edge_bases))  # (the judge agrees with itself on this set)
        assert np.array_equal(ctx.msm_var(edge_bases, s), want)
    # every point the same, every scalar 77: 77 n times that point
    same = np.tile(g[7], (n, 1))
    s77 = np.tile(orc.fr_from_int(77), (n, 1))
    want = orc.msm(orc.fr_from_int(77 * n).reshape(1, 4), g[7:8])
    assert np.array_equal(orc.msm(s77, same, threads=8), want)
    assert np.array_equal(ctx.msm_var(same, s77), want)
    # P, -P alone with equal scalars
    pair = np.stack([g[9], neg(zg, g[9])])
    for s in (np.tile(uniform[3], (2, 1)), np.tile(orc.fr_from_int(1), (2, 1))):
        assert is_identity(zg, orc.msm(s, pair))
        assert is_identity(zg, ctx.msm_var(pair, s))
    # nothing but identities
    assert is_identity(zg, ctx.msm_var(np.zeros((n, 8), np.uint64), uniform[:n]))


# ---- 5. batch ------------------------------------------------------------------------------------------------------------
def test_batch_matches_single_calls_and_the_oracle(ctx, orc, g, uniform, want_uniform):
    vectors = np.stack([uniform, orc.fill_fr_sparse(2111, N), np.zeros((N, 4), np.uint64), np.tile(orc.fr_from_int(1), (N, 1)),
                        orc.fill_fr(2112, N)])
    got = ctx.msm_var_batch(g, vectors)
    for b in range(vectors.shape[0]):
        assert np.array_equal(got[b], ctx.msm_var(g, vectors[b])), b
        assert np.array_equal(got[b], want_uniform(N) if b == 0 else orc.msm(vectors[b], g, threads=8)), b


# ---- 6. device form ------------------------------------------------------------------------------------------------------
def test_device_form_gives_the_host_form_bytes(ctx, orc, g, uniform):
    n, batch = 1000, 3
    stride = n + 7
    buf = np.full((batch, stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)  # (the seven words between the vectors are not scalars)
    vectors = [uniform[:n], orc.fill_fr_sparse(2121, n), orc.fill_fr(2122, n)]
    for b, s in enumerate(vectors):
        buf[b, :n] = s
    d_s = torch.from_numpy(buf.view(np.int64).reshape(-1).copy()).cuda()
    d_b = torch.from_numpy(g[:n].view(np.int64).reshape(-1).copy()).cuda()
    d_out = torch.full((batch * 16,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.msm_var_dev(d_b.data_ptr(), d_s.data_ptr(), stride, batch, n, d_out.data_ptr())
    got = ctx.msm_finish(d_out.data_ptr(), batch)
    want = ctx.msm_var_batch(g[:n], np.stack(vectors))
    assert np.array_equal(got, want)
    for b, s in enumerate(vectors):
        assert np.array_equal(got[b], orc.msm(s, g[:n], threads=8)), b
    # n = 0 through the device form: identities, copied without a launch
    ctx.msm_var_dev(0, 0, 0, batch, 0, d_out.data_ptr())
    ident = ctx.msm_finish(d_out.data_ptr(), batch)
    assert not ident[:, :4].any() and not ident[:, 8:].any()


# ---- 7. agreement with the fixed-base path; the workspace pool comes back intact ----------------------------------------
def test_agrees_with_registered_bases_and_returns_the_pool(ctx, orc, g, uniform, want_uniform):
    bases = ctx.register_bases(g)
    try:
        before = ctx.msm(bases, uniform)
        assert np.array_equal(before, ctx.msm_var(g, uniform))
        for n in (33, 4096, 1000):
            assert np.array_equal(ctx.msm_var(g[:n], uniform[:n]), want_uniform(n))
        assert np.array_equal(ctx.msm(bases, uniform), before)
        assert np.array_equal(before, want_uniform(N))
    finally:
        bases.free()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx, zg, g, uniform):
    for c in (1, 17):
        with pytest.raises(zg.ZgError) as e:
            ctx.msm_var(g[:8], uniform[:8], c)
        assert e.value.status == -1
    out = np.zeros(12, np.uint64)
    s = np.ascontiguousarray(uniform[:8])
    p = np.ascontiguousarray(g[:8])
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert ctx.lib.zg_msm_var(ctx.h, None, ptr(s), 8, 0, ptr(out)) == -1
    assert ctx.lib.zg_msm_var(ctx.h, ptr(p), None, 8, 0, ptr(out)) == -1
    assert ctx.lib.zg_msm_var(ctx.h, ptr(p), ptr(s), 8, 0, None) == -1
    # n = 2^23 through the HOST entry, with small real buffers: the sizes are checked before anything is read or allocated
    assert ctx.lib.zg_msm_var(ctx.h, ptr(p), ptr(s), 1 << 23, 0, ptr(out)) == -4
    ptrs = (ctypes.c_void_p * 1)(s.ctypes.data)
    assert ctx.lib.zg_msm_var_batch(ctx.h, ptr(p), ptrs, 257, 8, 0, ptr(out)) == -4  # ZG_MSM_VAR_MAX_BATCH = 256
    assert ctx.lib.zg_msm_var_dev(ctx.h, None, None, 8, 1, 1 << 23, 0, None) == -4
    assert ctx.lib.zg_msm_var_dev(ctx.h, None, None, 8, 1, 8, 0, None) == -1
    # the context still works
    assert np.array_equal(ctx.msm_var(p, s), ctx.msm_var(p, s, 5))


# ---- 9. profile ----------------------------------------------------------------------------------------------------------
def test_profile_names_and_unit_bytes(ctx, g, uniform, want_uniform):
    ctx.profile(True)
    try:
        ctx.profile_collect()
        got = ctx.msm_var(g, uniform)
        stats = ctx.profile_collect()
    finally:
        ctx.profile(False)
    assert np.array_equal(got, want_uniform(N))
    names = [k for k in stats if k.startswith("msm_var_")]
    print({k: stats[k] for k in names})
    assert len(names) >= 5 and "msm_var_accumulate" in names and "msm_var_horner" in names
    assert not [k for k in stats if k.startswith("msm_") and not k.startswith("msm_var_")]  # no launch of the table path
    assert sum(stats[k][3] for k in names) == N * 96 + 96
    assert all(stats[k][0] == 1 and stats[k][1] > 0.0 for k in names)
