"""zg_g1_mul_each / zg_g1_mul_each_dev (csrc/g1_mul.hip): n independent multiplications out[i] = scalars[i] * points[i]
against BN254 arithmetic on Python integers (tests/srs_cases.py; test_srs_update_host.py holds that reference against
the oracle).  Sizes on both sides of a wave, a workgroup and a two-workgroup grid; scalars at the edges of the signed
recoding (small values, r - j, the all-maximum and all-minimum digit patterns); identities, repeated and opposite
points.  Every comparison is equality of bytes."""
import torch  # noqa: F401  (before anything loads the library: tests/conftest.py says why)

import ctypes
import os
import re

import numpy as np
import pytest

import srs_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "0g-halo2_amd", "csrc")
W = int(re.search(r"G1_MUL_W = (\d+);", open(os.path.join(CSRC, "g1_mul_digits.h")).read()).group(1))
WG = int(re.search(r"G1MUL_WG = (\d+);", open(os.path.join(CSRC, "g1_mul.hip")).read()).group(1))
N_MAX = 2 * WG + 1
SIZES = sorted({0, 1, 63, 64, 65, WG - 1, WG, WG + 1, 2 * WG - 1, 2 * WG, N_MAX})
R = sc.R


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def master():
    """N_MAX distinct points (none the generator) with the edge scalars spread over the lanes, and their products: made
    once, never modified (the tests below copy)"""
    edge = sc.edge_scalars(W)
    first_rminus = (1 << W) + 2  # the index of r - 1 in the list: lane 0 gets it (n = 1 then multiplies by r - 1)
    assert edge[first_rminus] == R - 1 and len(edge) <= WG
    scalars = [edge[(i + first_rminus) % len(edge)] for i in range(N_MAX)]
    points = []
    p, step = sc.mul(sc.G, 5), sc.mul(sc.G, 0xDEADBEEF)
    for _ in range(N_MAX):
        points.append(p)
        p = sc.add(p, step)
    return points, scalars, sc.points_np(points), sc.scalars_np(scalars), sc.mul_each_ref(points, scalars)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def from_dev(t, width):
    return t.cpu().numpy().view(np.uint64).reshape(-1, width)


def test_cases_cover_the_recoding_edges(master):
    _, scalars, _, _, want = master
    half = 1 << (W - 1)
    ds = [sc.digits(s, W) for s in scalars[:WG]]
    assert any(all(d == half - 1 for d in dd[3:]) for _, _, dd in ds)   # every digit but the top few at its maximum
    assert any(all(d == -half for d in dd[3:]) and any(d == -half for d in dd) for _, _, dd in ds)
    assert all(top == 0 for _, top, _ in ds)  # (the bit above the windows is set only from 0.85 2^254 on: never below r)
    assert {0, 1, 2, R - 1, R - 2, 1 << 253, (R - 1) // 2, (R + 1) // 2} <= set(scalars[:WG])
    assert not want[scalars.index(0)].any() and np.array_equal(want[scalars.index(1)], master[2][scalars.index(1)])


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, master, n):
    _, _, pts, scs, want = master
    got = ctx.g1_mul_each(pts[:n], scs[:n])
    assert got.shape == (n, 8)
    assert np.array_equal(got, want[:n])


def test_same_point_in_every_lane(ctx, master):
    points, scalars, _, _, _ = master
    n = WG + 1
    p = points[7]
    want = sc.mul_each_ref([p] * n, scalars[:n])
    assert np.array_equal(ctx.g1_mul_each(sc.points_np([p] * n), sc.scalars_np(scalars[:n])), want)


def test_opposite_points_in_neighbouring_lanes(ctx, master):
    points, scalars, _, _, want = master
    n = WG
    pts = [points[i - (i & 1)] if not i & 1 else sc.neg(points[i - 1]) for i in range(n)]
    ks = [scalars[i - (i & 1)] for i in range(n)]
    got = ctx.g1_mul_each(sc.points_np(pts), sc.scalars_np(ks))
    for i in range(0, n, 2):
        assert np.array_equal(got[i], want[i]), i
        assert np.array_equal(got[i + 1], sc.affine_to_np(sc.neg(sc.np_to_affine(want[i])))), i


@pytest.mark.parametrize("where", ["lane0", "lane1", "last", "workgroup", "side_by_side"])
def test_identities_disturb_no_neighbour(ctx, master, where):
    _, _, pts, scs, want = master
    n = N_MAX
    pts, scs, want = pts.copy(), scs.copy(), want.copy()
    if where == "side_by_side":  # (0,0) with a non-zero scalar beside a point with scalar 0, twice
        for i in (20, WG + 2):
            assert scs[i].any() and scs[i + 1].any()
            pts[i] = 0
            scs[i + 1] = 0
            want[i] = 0
            want[i + 1] = 0
    else:
        rows = {"lane0": [0], "lane1": [1], "last": [n - 1], "workgroup": list(range(WG, 2 * WG))}[where]
        pts[rows] = 0
        want[rows] = 0
    assert np.array_equal(ctx.g1_mul_each(pts, scs), want)


def test_all_identities_and_all_zero_scalars(ctx, master):
    _, _, pts, scs, _ = master
    n = WG + 1
    assert not ctx.g1_mul_each(np.zeros((n, 8), np.uint64), scs[:n]).any()
    assert not ctx.g1_mul_each(pts[:n], np.zeros((n, 4), np.uint64)).any()


def test_host_and_device_forms_give_the_same_bytes(ctx, master):
    _, _, pts, scs, want = master
    n = N_MAX
    host = ctx.g1_mul_each(pts, scs)
    d_p, d_s = to_dev(pts), to_dev(scs)
    d_o = torch.full((n * 8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.g1_mul_each_dev(d_p.data_ptr(), d_s.data_ptr(), n, d_o.data_ptr())
    ctx.sync()
    assert np.array_equal(from_dev(d_p, 8), pts) and np.array_equal(from_dev(d_s, 4), scs)  # inputs left alone
    out_of_place = from_dev(d_o, 8)
    ctx.g1_mul_each_dev(d_p.data_ptr(), d_s.data_ptr(), n, d_p.data_ptr())
    ctx.sync()
    in_place = from_dev(d_p, 8)
    assert np.array_equal(host, want) and np.array_equal(out_of_place, want) and np.array_equal(in_place, want)


def test_limits_touch_no_output(ctx, master):
    _, _, pts, scs, want = master
    lib = ctx.lib
    sentinel = np.full((4, 8), 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = sentinel.copy()
    n4, big = ctypes.c_size_t(4), ctypes.c_size_t(1 << 28)
    assert lib.zg_g1_mul_each(ctx.h, None, _p(scs), n4, _p(out)) == -1
    assert lib.zg_g1_mul_each(ctx.h, _p(pts), None, n4, _p(out)) == -1
    assert lib.zg_g1_mul_each(ctx.h, _p(pts), _p(scs), n4, None) == -1
    assert lib.zg_g1_mul_each(ctx.h, _p(pts), _p(scs), big, _p(out)) == -4  # refused before anything is read
    assert lib.zg_g1_mul_each(ctx.h, None, None, ctypes.c_size_t(0), None) == 0  # n = 0: nothing to do
    assert np.array_equal(out, sentinel)
    d_p, d_s, d_o = to_dev(pts[:4]), to_dev(scs[:4]), to_dev(sentinel)
    torch.cuda.synchronize()
    vp = ctypes.c_void_p
    assert lib.zg_g1_mul_each_dev(ctx.h, None, vp(d_s.data_ptr()), n4, vp(d_o.data_ptr())) == -1
    assert lib.zg_g1_mul_each_dev(ctx.h, vp(d_p.data_ptr()), None, n4, vp(d_o.data_ptr())) == -1
    assert lib.zg_g1_mul_each_dev(ctx.h, vp(d_p.data_ptr()), vp(d_s.data_ptr()), n4, None) == -1
    assert lib.zg_g1_mul_each_dev(ctx.h, vp(d_p.data_ptr()), vp(d_s.data_ptr()), big, vp(d_o.data_ptr())) == -4
    assert lib.zg_g1_mul_each_dev(ctx.h, None, None, ctypes.c_size_t(0), None) == 0
    ctx.sync()
    assert np.array_equal(from_dev(d_o, 8), sentinel)
    assert np.array_equal(ctx.g1_mul_each(pts[:4], scs[:4]), want[:4])  # the context still works
