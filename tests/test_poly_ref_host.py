"""The oracle's grand product, evaluation and division by X - z pinned to tests/poly_ref.py (Python integers) on every value
family of tests/test_gpu_poly_scans.py, the zero rules included; no GPU.  That file lets the oracle judge the HIP kernels at
the sizes where Python integers are too slow: this file is why it may."""
import numpy as np
import pytest

import poly_ref as pr

SIZES = [1, 2, 3, 257, 1025]


def test_converters(orc, zg):
    vals = [0, 1, 2, pr.R - 1, pr.R - 2, 1 << 253, 0x1234567 << 128] + pr.to_ints(orc.fill_fr(5, 8))
    arr = pr.from_ints(vals)
    assert arr.dtype == np.uint64 and arr.shape == (len(vals), 4)
    for v, row in zip(vals, arr):
        assert np.array_equal(row, orc.fr_from_int(v)) and np.array_equal(row, zg.fr_from_int(v))
        assert zg.fr_to_int(row) == orc.fr_to_int(row) == v
    assert pr.to_ints(arr) == vals and pr.to_int(arr[3]) == pr.R - 1
    top = pr.stored([pr.R - 1, 5])
    assert zg.limbs_to_int(top[0]) == pr.R - 1 and zg.limbs_to_int(top[1]) == 5
    assert pr.to_int(top[0]) == (pr.R - 1) * pow(1 << 256, -1, pr.R) % pr.R == orc.fr_to_int(top[0])
    with pytest.raises(AssertionError):
        pr.stored([pr.R])


def gp_matches(orc, name, num, den, z0):
    want = pr.grand_product(pr.to_ints(num), pr.to_ints(den), pr.to_int(z0))
    assert np.array_equal(orc.grand_product(num, den, z0), pr.from_ints(want)), name
    return want


@pytest.mark.parametrize("n", SIZES)
def test_grand_product(orc, n):
    for name, (num, den, z0) in pr.gp_zero_free(orc.fill_fr, n, True).items():
        assert all(gp_matches(orc, name, num, den, z0)), name  # no zero row
    for name, (num, den, z0, live) in pr.gp_degenerate(orc.fill_fr, n).items():
        z = gp_matches(orc, name, num, den, z0)
        assert all(z[:live]) and not any(z[live:]), name


@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("which", ["denominator", "numerator"])
def test_grand_product_with_one_zero(orc, n, which):
    num, den, z0 = pr.gp_zero_free(orc.fill_fr, n, False)["random"]
    free = gp_matches(orc, "zero-free", num, den, z0)
    places = pr.zero_places(n) if n > 1024 else [0, 1, 255, n - 2, n - 1]
    for t in places:
        m, d = num.copy(), den.copy()
        (d if which == "denominator" else m)[t] = 0
        z = gp_matches(orc, t, m, d, z0)
        assert z[:t + 1] == free[:t + 1] and all(z[:t + 1]) and not any(z[t + 1:]), t
    assert z == free  # t = n - 1: the last numerator and denominator enter no row


@pytest.mark.parametrize("n", SIZES)
def test_eval_poly_and_kate_division(orc, zg, n):
    omega = zg.domain_omega(n.bit_length() - 1)[0] if n > 1 and n & (n - 1) == 0 else None
    pts = pr.points(orc.fill_fr, n, omega)
    for pname, a in pr.polynomials(orc.fill_fr, n).items():
        ai = pr.to_ints(a)
        for xname, x in pts.items():
            xi = pr.to_int(x)
            assert np.array_equal(orc.eval_poly(a, x), pr.from_int(pr.eval_poly(ai, xi))), (pname, xname)
            q = pr.kate_division(ai, xi)
            assert np.array_equal(orc.kate_division(a, x), pr.from_ints(q)), (pname, xname)
            # a(X) = q(X) (X - z) + a(z), coefficient by coefficient
            rem = pr.eval_poly(ai, xi)
            for i in range(n):
                assert ai[i] == ((q[i - 1] if i else 0) - xi * q[i] + (rem if i == 0 else 0)) % pr.R, (pname, xname, i)
