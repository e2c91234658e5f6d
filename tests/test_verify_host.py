"""The product's host pairing (zg_pairing_check, csrc/pairing.hip) against the oracle's (orc_pairing_check): the same
verdict on products of pairings that are and are not 1.  No device needed."""
import ctypes

import numpy as np
import pytest

from test_oracle_pairing import R, g1_mul, g2_mul


def orc_check(orc, ps, qs):
    ps = np.ascontiguousarray(np.array(ps, dtype=np.uint64).reshape(-1, 8))
    qs = np.ascontiguousarray(np.array(qs, dtype=np.uint64).reshape(-1, 16))
    return int(orc.load().orc_pairing_check(ctypes.c_void_p(ps.ctypes.data), ctypes.c_void_p(qs.ctypes.data),
                                            ctypes.c_size_t(ps.shape[0])))


def both(zg, orc, ps, qs):
    got = zg.pairing_check(np.array(ps, dtype=np.uint64).reshape(-1, 8), np.array(qs, dtype=np.uint64).reshape(-1, 16))
    want = orc_check(orc, ps, qs)
    assert got == want
    return got


@pytest.mark.parametrize("a,b", [(1, 1), (5, 7), (R - 2, 3), (123456789, 987654321)])
def test_bilinear_product_is_one(zg, orc, a, b):
    # e(aP, bQ) e(-abP, Q) = 1
    assert both(zg, orc, [g1_mul(orc, a), g1_mul(orc, (R - a * b) % R)], [g2_mul(orc, b), g2_mul(orc, 1)]) == 1


@pytest.mark.parametrize("a,b", [(5, 7), (R - 2, 3)])
def test_one_scalar_off_by_one(zg, orc, a, b):
    assert both(zg, orc, [g1_mul(orc, a + 1), g1_mul(orc, (R - a * b) % R)], [g2_mul(orc, b), g2_mul(orc, 1)]) == 0
    assert both(zg, orc, [g1_mul(orc, a), g1_mul(orc, (R - a * b) % R)], [g2_mul(orc, b + 1), g2_mul(orc, 1)]) == 0


def test_identity_inputs(zg, orc):
    z1, z2 = np.zeros(8, np.uint64), np.zeros(16, np.uint64)
    assert both(zg, orc, [z1], [g2_mul(orc, 3)]) == 1
    assert both(zg, orc, [g1_mul(orc, 3)], [z2]) == 1
    assert both(zg, orc, [z1, g1_mul(orc, 2)], [z2, g2_mul(orc, 2)]) == 0
    assert both(zg, orc, [g1_mul(orc, 2), g1_mul(orc, R - 2), z1], [g2_mul(orc, 9), g2_mul(orc, 9), z2]) == 1


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_products_of_n(zg, orc, n):
    # n pairs whose exponents sum to 0 (mod r) are 1; the same with the last exponent + 1 is not
    if n == 0:
        assert zg.pairing_check(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64)) == 1
        return
    rng = np.random.default_rng(n)
    ks = [int(rng.integers(1, 1 << 62)) for _ in range(n)]
    ms = [int(rng.integers(1, 1 << 62)) for _ in range(n)]
    tot = sum(k * m for k, m in zip(ks[:-1], ms[:-1])) % R
    last = (R - tot) * pow(ms[-1], -1, R) % R  # k_last * m_last = -tot
    ps = [g1_mul(orc, k) for k in ks[:-1]] + [g1_mul(orc, last)]
    qs = [g2_mul(orc, m) for m in ms]
    assert both(zg, orc, ps, qs) == 1  # (n = 1: the exponent is 0, the identity)
    ps[-1] = g1_mul(orc, last + 1)
    assert both(zg, orc, ps, qs) == 0


def test_srs_points(zg, orc):
    # e([s]_1, [1]_2) = e([1]_1, [s]_2) with the parameters' own points; e(g, s_g2) alone is not 1
    prm = orc.params_new(5)
    g = prm.g_np()
    g2 = np.array(prm.g2, dtype=np.uint64)
    sg2 = np.array(prm.s_g2, dtype=np.uint64)
    neg_g0 = g[0].copy()
    y = orc.fq_to_int(g[0][4:8])
    Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
    neg_g0[4:8] = zg.fq_from_int(Q - y)
    assert both(zg, orc, [g[1], neg_g0], [g2, sg2]) == 1
    assert both(zg, orc, [g[2], neg_g0], [g2, sg2]) == 0
    assert both(zg, orc, [g[0]], [sg2]) == 0
