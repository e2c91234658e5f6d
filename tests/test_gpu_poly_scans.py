"""The three scans of csrc/poly.hip at their edges, through the context-level entries: zg_grand_product_dev (and the
host-pointer zg_grand_product), zg_eval_polys_dev and zg_kate_division_dev.

Every case runs in both forms -- latency (256-row blocks and a 1024-lane totals / heads kernel, n <= 2^18) and throughput
(1024 lanes with a strip of ceil(n / 1024) rows each) -- and is compared for EQUALITY of field elements with
tests/poly_ref.py (Python integers) up to n = 2^14 and with the oracle above that; tests/test_poly_ref_host.py holds the
oracle against poly_ref on the same value families.  The sizes bracket the blocks (256), the lanes (1024), the strips, the
form bound 2^18 and the lazy dot product's bound 2^20; the values are chosen so that a wrong factor SHOWS: a grand-product
case asserts, before the device is asked, that its expected rows are non-zero wherever a product is compared."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import poly_ref as pr

pytestmark = pytest.mark.gpu

PY_MAX = 1 << 14  # poly_ref judges up to here, the oracle above
FORMS = [True, False]  # set_msm_latency: latency form, throughput form


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@contextmanager
def form(ctx, latency: bool):
    ctx.set_msm_latency(latency)
    try:
        yield
    finally:
        ctx.set_msm_latency(True)


@contextmanager
def lazy_dot(zg, value: int):
    zg.tuning_set("ZG_LAZY_DOT", value)
    try:
        yield
    finally:
        zg.tuning_set("ZG_LAZY_DOT", -1)


def launched(ctx, call) -> set:
    """the launch labels of one call"""
    ctx.profile(True)
    try:
        ctx.profile_collect()
        call()
        return set(ctx.profile_collect())
    finally:
        ctx.profile(False)


def nonzero(z: np.ndarray) -> np.ndarray:
    return z.reshape(-1, 4).any(axis=1)


# ------------------------------------------------------------------ grand product
def gp_want(orc, num, den, z0) -> np.ndarray:
    if num.shape[0] <= PY_MAX:
        return pr.from_ints(pr.grand_product(pr.to_ints(num), pr.to_ints(den), pr.to_int(z0)))
    return orc.grand_product(num, den, z0)


def gp_both_forms(ctx, num, den, z0, want, name, host_entry=False):
    n = num.shape[0]
    dn, dd = dev(num), dev(den)
    for latency in FORMS:
        dz = torch.full_like(dn, -1)
        with form(ctx, latency):
            ctx.grand_product_dev(dn.data_ptr(), dd.data_ptr(), z0, n, dz.data_ptr())
            assert np.array_equal(host(dz), want), (name, n, latency)
            if host_entry:
                assert np.array_equal(ctx.grand_product(num, den, z0), want), (name, n, latency, "host pointers")


GP_SIZES = [1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 3073, 1 << 14, (1 << 16) + 255,
            (1 << 18) - 1, 1 << 18, (1 << 18) + 1]
GP_ALL_FAMILIES = (513, 2049, 1 << 14)  # stored r - 1 everywhere and z0 = 1 go with these
GP_HOST_ENTRY = (1, 257, 1025, 2049, 1 << 14)
GP_ZERO_SIZES = [1025, 2049, 1 << 14]


@pytest.mark.parametrize("n", GP_SIZES)
def test_grand_product_without_zeros(ctx, orc, n):
    """Every row is a product that a wrong lane constant, D' suffix, 1/T, block total or strip edge changes: the expected
    output has no zero row (asserted first)."""
    for name, (num, den, z0) in pr.gp_zero_free(orc.fill_fr, n, n in GP_ALL_FAMILIES).items():
        want = gp_want(orc, num, den, z0)
        assert nonzero(want).all(), (name, "a zero row in a zero-free case")
        gp_both_forms(ctx, num, den, z0, want, name, host_entry=n in GP_HOST_ENTRY)


@pytest.mark.parametrize("n", GP_ZERO_SIZES)
@pytest.mark.parametrize("which", ["denominator", "numerator"])
def test_grand_product_with_one_zero(ctx, orc, n, which):
    """One zero at row t (rows 0, 1, 255, 256, the first and last row of a strip, n - 2, n - 1): rows <= t are the zero-free
    product, rows > t are 0; t = n - 1 changes nothing, the kernels fold den[n-1] into T and D' and no row depends on it."""
    num, den, z0 = pr.gp_zero_free(orc.fill_fr, n, False)["random"]
    free = gp_want(orc, num, den, z0)
    assert nonzero(free).all()
    for t in pr.zero_places(n):
        m, d = num.copy(), den.copy()
        (d if which == "denominator" else m)[t] = 0
        want = gp_want(orc, m, d, z0)
        assert np.array_equal(want[:t + 1], free[:t + 1]) and not nonzero(want[t + 1:]).any(), t
        if t == n - 1:
            assert nonzero(want).all()
        gp_both_forms(ctx, m, d, z0, want, (which, t), host_entry=t == 256 and n == 1025)


@pytest.mark.parametrize("n", [3, 257] + GP_ZERO_SIZES)
def test_grand_product_degenerate(ctx, orc, n):
    """Two zeros in one block or strip (denominators, and a numerator with a denominator in either order), every
    denominator zero, z0 = 0."""
    for name, (num, den, z0, live) in pr.gp_degenerate(orc.fill_fr, n).items():
        want = gp_want(orc, num, den, z0)
        assert nonzero(want[:live]).all() and not nonzero(want[live:]).any(), name
        gp_both_forms(ctx, num, den, z0, want, name)


# ------------------------------------------------------------------ the launch sequences either side of 2^18
@pytest.mark.parametrize("n", [1 << 18, (1 << 18) + 1])
@pytest.mark.parametrize("latency", FORMS)
def test_launch_sequences(ctx, orc, n, latency):
    """The latency form's block kernels run up to n = 2^18 (1024 block totals: a full totals / heads workgroup); above it,
    and in the throughput form at any size, the strip kernels do."""
    blocks = latency and n <= 1 << 18
    d = dev(orc.fill_fr(1, 2 * n))
    out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    z = orc.fill_fr(3, 1)[0]
    with form(ctx, latency):
        gp = launched(ctx, lambda: ctx.grand_product_dev(d.data_ptr(), d.data_ptr() + 32 * n, z, n, out.data_ptr()))
        kd = launched(ctx, lambda: ctx.kate_division_dev(d.data_ptr(), n, z, out.data_ptr()))
    assert ("grand_product_local" in gp, "grand_product_totals" in gp, "grand_product_scan" in gp) == (blocks, blocks, not blocks), gp
    assert ("kate_local" in kd, "kate_heads" in kd, "kate_apply" in kd, "kate_division" in kd) == (blocks, blocks, blocks, not blocks), kd


# ------------------------------------------------------------------ evaluation
def omega_of(zg, n):
    return zg.domain_omega(n.bit_length() - 1)[0] if n > 1 and n & (n - 1) == 0 else None


def eval_want(orc, a, ai, x) -> np.ndarray:
    if a.shape[0] <= PY_MAX:
        return pr.from_int(pr.eval_poly(ai, pr.to_int(x)))
    return orc.eval_poly(a, x)


EVAL_KERNELS = [(1, True), (1, False), (0, True), (0, False)]  # (ZG_LAZY_DOT, latency form)
EVAL_SIZES = [1, 2, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 3071, 3072, 3073, 4095, 4096, 4097, 1 << 14]


def eval_all_kernels(ctx, zg, d, n, idx, pts, want, combos=EVAL_KERNELS):
    for lazy, latency in combos:
        with lazy_dot(zg, lazy), form(ctx, latency):
            got = ctx.eval_polys_dev(d.data_ptr(), n, n, idx, pts)
        bad = [j for j in range(len(idx)) if not np.array_equal(got[j], want[j])]
        assert not bad, (n, "ZG_LAZY_DOT", lazy, "latency", latency, "pairs", bad)


@pytest.mark.parametrize("n", EVAL_SIZES)
def test_eval_polys(ctx, zg, orc, n):
    """Every polynomial family at every point (0, 1, r - 1, stored r - 1, 2, omega where n = 2^k, random): one call of a few
    dozen pairs, served 16 at a time.  The three kernels share the label eval_dot; they are selected by
      ZG_LAZY_DOT = 1, latency form     dot9_kernel<1024> (n <= 2^20), powers_kernel<4>
      ZG_LAZY_DOT = 1, throughput form  dot9_kernel<256>  (n <= 2^20), powers_kernel<16>
      ZG_LAZY_DOT = 0, either form      dot_kernel (eight limbs, 1024 lanes), powers_kernel<4> / <16>
    The sizes bracket one and three terms per lane of both workgroup sizes (the three-term loop and its tail) and a
    powers_kernel strip of 4 and 16 at 256 lanes.  A lone 1 at coefficient n - 1 gives x^(n-1): the top of the power table."""
    polys = pr.polynomials(orc.fill_fr, n)
    pts = pr.points(orc.fill_fr, n, omega_of(zg, n))
    stack = np.stack(list(polys.values()))
    ints = [pr.to_ints(a) if n <= PY_MAX else None for a in stack]
    idx, xs, want = [], [], []
    for p in range(stack.shape[0]):
        for x in pts.values():
            idx.append(p)
            xs.append(x)
            want.append(eval_want(orc, stack[p], ints[p], x))
    top = list(polys).index("a lone 1 at coefficient n - 1") * len(pts) + list(pts).index("random")
    assert pr.to_int(want[top]) == pow(pr.to_int(pts["random"]), n - 1, pr.R)
    eval_all_kernels(ctx, zg, dev(stack), n, idx, np.stack(xs), want)


@pytest.mark.parametrize("count", [1, 16, 17, 33])
def test_eval_polys_pair_counts(ctx, zg, orc, count):
    """The entry serves the pairs 16 at a time: a lone pair, one whole chunk, a chunk and one, two chunks and one -- with
    repeated polynomial indices and repeated points."""
    n = 769
    stack = np.stack([orc.fill_fr(20 + i, n) for i in range(3)])
    ints = [pr.to_ints(a) for a in stack]
    five = orc.fill_fr(98, 5)
    idx = [(7 * j + j // 5) % 3 for j in range(count)]
    xs = np.stack([five[(3 * j) % 5] for j in range(count)])
    want = [eval_want(orc, stack[p], ints[p], x) for p, x in zip(idx, xs)]
    eval_all_kernels(ctx, zg, dev(stack), n, idx, xs, want)


@pytest.mark.parametrize("latency", FORMS)
def test_eval_polys_at_the_lazy_bound(ctx, zg, orc, latency):
    """ZG_LAZY_DOT = 1 either side of n <= 2^20: at 2^20 the nine-limb kernel (a 256-lane workgroup sums 4096 terms per
    lane, stored r - 1 everywhere being the largest it can meet), at 2^20 + 1 the eight-limb kernel behind the rule."""
    try:
        for n in (1 << 20, (1 << 20) + 1):
            stack = np.stack([orc.fill_fr(30, n), np.tile(pr.stored([pr.R - 1]), (n, 1))])
            stack[0, n - 1] = pr.from_int(1)
            xs = np.stack([orc.fill_fr(97, 1)[0], pr.stored([pr.R - 1])[0], pr.from_int(pr.R - 1)])
            idx = [0, 1, 1]
            want = [orc.eval_poly(stack[p], x) for p, x in zip(idx, xs)]
            eval_all_kernels(ctx, zg, dev(stack), n, idx, xs, want, combos=[(1, latency)])
    finally:
        ctx.drop_workspace()  # the entry reserves 16 power tables of n elements


# ------------------------------------------------------------------ Kate division
KATE_SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 1 << 14, (1 << 18) - 1, 1 << 18, (1 << 18) + 1]
KATE_IDENTITY = (257, 1025, 2049)  # a(X) = q(X) (X - z) + a(z) in Python integers, a(z) from eval_polys_dev


def kate_divisors(orc):
    return {"0": pr.from_int(0), "1": pr.from_int(1), "r - 1": pr.from_int(pr.R - 1), "random": orc.fill_fr(96, 1)[0]}


def kate_both_forms(ctx, orc, n, latency_forms=FORMS):
    polys = pr.polynomials(orc.fill_fr, n)
    zs = kate_divisors(orc)
    for pname, a in polys.items():
        ai = pr.to_ints(a) if n <= PY_MAX else None
        da = dev(a)
        for zname, z in zs.items():
            zi = pr.to_int(z)
            want = pr.from_ints(pr.kate_division(ai, zi)) if ai is not None else orc.kate_division(a, z)
            if pname == "a lone 1 at coefficient n - 1" and n >= 2 and zname == "random":  # q_i = z^(n-2-i)
                assert pr.to_int(want[0]) == pow(zi, n - 2, pr.R) and nonzero(want[:n - 1]).all()
            for latency in latency_forms:
                dq = torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
                with form(ctx, latency):
                    ctx.kate_division_dev(da.data_ptr(), n, z, dq.data_ptr())
                    got = host(dq)
                    assert np.array_equal(got, want), (n, pname, zname, latency)
                    if n in KATE_IDENTITY:
                        rem = pr.to_int(ctx.eval_polys_dev(da.data_ptr(), n, n, [0], z[None, :])[0])
                        q = pr.to_ints(got)
                        for i in range(n):
                            assert ai[i] == ((q[i - 1] if i else 0) - zi * q[i] + (rem if i == 0 else 0)) % pr.R, (pname, zname, i)


@pytest.mark.parametrize("n", [n for n in KATE_SIZES if n <= PY_MAX])
def test_kate_division(ctx, orc, n):
    """Every polynomial family by every divisor (z = 0, 1, r - 1, random).  A lone 1 at coefficient n - 1 gives
    q_i = z^(n-2-i): every weight of every scan step shows.  The upper half zero (and only a constant term) makes the carries
    into the lower blocks zero: kd_apply_kernel skips its product there."""
    kate_both_forms(ctx, orc, n)


@pytest.mark.parametrize("latency", FORMS)
@pytest.mark.parametrize("n", [n for n in KATE_SIZES if n > PY_MAX])
def test_kate_division_at_the_form_bound(ctx, orc, n, latency):
    """2^18 gives 1024 block heads, a full heads workgroup; 2^18 + 1 goes to the strip kernel in either form."""
    kate_both_forms(ctx, orc, n, [latency])


# ------------------------------------------------------------------ arguments
def test_arguments(ctx, zg, orc):
    a = orc.fill_fr(1, 8)
    d = dev(a)
    out = torch.full((8, 4), -1, dtype=torch.int64, device="cuda")
    z = orc.fill_fr(3, 1)[0]
    ctx.grand_product_dev(d.data_ptr(), d.data_ptr(), z, 0, out.data_ptr())  # n = 0: success, nothing written
    ctx.sync()
    assert (out.cpu() == -1).all()
    for call, status in [(lambda: ctx.grand_product(a[:0], a[:0], z), -4),  # ZG_ERR_UNSUPPORTED
                         (lambda: ctx.kate_division_dev(d.data_ptr(), 0, z, out.data_ptr()), -1),  # ZG_ERR_INVALID_ARG
                         (lambda: ctx.eval_polys_dev(d.data_ptr(), 8, 4, [0], z[None, :]), -4)]:
        with pytest.raises(zg.ZgError) as e:
            call()
        assert e.value.status == status
    assert (out.cpu() == -1).all()
