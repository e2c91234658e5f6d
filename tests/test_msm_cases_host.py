"""CPU: tests/msm_cases.py is what it claims -- the recoding sums back, every family has the histogram it states, the
oracle's best_multiexp and the one-scalar-multiplication judge agree on every family, and the GPU file's comparison
rejects a wrong point."""
import numpy as np
import pytest

import msm_cases as mc
from field9_ref import R

SEED = 0x5EED
K_SRS = 8  # n = 256


@pytest.fixture(scope="module")
def srs(orc):
    prm = orc.params_new(K_SRS, SEED)
    toxic = orc.fr_to_int(orc.fill_fr(SEED, 1)[0])
    return toxic, {"g": prm.g_np(), "g_lagrange": prm.g_lagrange_np()}


def _families(n):
    """name -> scalar vectors (Python integers) of n points"""
    out = {}
    c = mc.default_window_bits(n)
    for K in (4, 16, 48):
        out[f"task_edges-{K}"] = [mc.from_histogram(n, c, mc.task_edges(K))]
    out["hot_threshold-16-16"] = [mc.from_histogram(n, c, mc.hot_threshold(16, 16, 5 * n))]
    out["hot_threshold-48-4"] = [mc.from_histogram(n, c, mc.hot_threshold(48, 4, 4 * n))]
    out["span_edges-4"] = [mc.from_histogram(n, c, mc.span_edges(4))]
    out["many_hot-257"] = [mc.from_histogram(n, 11, mc.many_hot(257, 5))]
    out["lone_buckets"] = [mc.from_histogram(n, cc, mc.lone_buckets(cc), window=w) for cc, w in ((4, 0), (11, 1), (16, 3))]
    for cc in (2, 7, 11, 16):
        vals = mc.carry_digits(cc)
        out[f"carry_digits-{cc}"] = [(vals[i:i + n] + [0] * n)[:n] for i in range(0, len(vals), n)]
    return out


@pytest.mark.parametrize("c", range(2, 17))
def test_window_digits_sum_back(c):
    W, nb = mc.windows_of(c), 1 << (c - 1)
    vals = mc.carry_digits(c)
    assert len(vals) > (4 if c > 2 else 3) * (W - 2)  # (c = 2: nb + 1 = 2^c - 1)
    for v in vals:
        d = mc.window_digits_ref(v, c)
        assert len(d) == W and all(-nb < x <= nb for x in d)
        assert sum(x << (c * w) for w, x in enumerate(d)) == v
    # the carry's two sides
    assert mc.window_digits_ref(nb, c)[:2] == [nb, 0]
    assert mc.window_digits_ref(nb + 1, c)[:2] == [-(nb - 1), 1]
    assert mc.window_digits_ref((1 << c) - 1, c)[:2] == [-1, 1]
    assert mc.window_digits_ref(R - 1, c)[-1] > 0


def test_histogram_counts_every_window():
    c = 5
    s = [3 | (3 << 5) | (16 << 10), 17, 0, 31 << 20]  # 17 -> -15, carry 1; 31 -> -1, carry 1
    assert mc.histogram(s, c) == {3: 2, 16: 1, 15: 1, 1: 3}
    with pytest.raises(AssertionError):
        mc.histogram([1 << (c * (mc.windows_of(c) - 1) - 1)], c)  # a large scalar


@pytest.mark.parametrize("n", [256, 300, 4096])
def test_families_have_their_histograms(n):
    c = mc.default_window_bits(n)
    stride = mc._stride(n)
    assert np.gcd(stride, n) == 1 and 1 < stride < n - 1
    for K in (4, 16, 32, 48, 120):
        h = mc.task_edges(K)
        assert sorted(h.values()) == sorted([1, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 3 * K + 1])
        v = mc.from_histogram(n, c, h)
        assert len(v) == n and mc.histogram(v, c) == h
        v1 = mc.from_histogram(n, c, h, window=2)
        assert mc.histogram(v1, c) == h and v1 != v
    for K, thr in ((16, 16), (48, 4), (16, 1), (48, 1), (16, 64), (48, 64)):
        need = 4 * thr * K + K + 2
        entries = n * ((need + n - 1) // n)
        if (entries + n - 1) // n > mc.windows_of(c) - 1:
            continue
        h = mc.hot_threshold(K, thr, entries)
        assert sum(h.values()) == entries and mc.histogram(mc.from_histogram(n, c, h), c) == h
        assert [mc.is_hot(h[k], K, thr) for k in (1, 2, 3, 4)] == [False, False, True, True]
    h = mc.span_edges(4)
    assert sum(h.values()) == 2819 and all(mc.is_hot(v, 4, 1) for v in h.values())
    assert mc.histogram(mc.from_histogram(n, c, h), c) == h
    for count in (255, 256, 257, 513):
        h = mc.many_hot(count, 5)
        assert len(h) == count and set(h.values()) == {5} and mc.is_hot(5, 4, 1) and not mc.is_hot(4, 4, 1)
        assert mc.histogram(mc.from_histogram(n, 11, h), 11) == h
    for cc in range(2, 17):
        h = mc.lone_buckets(cc)
        nb = 1 << (cc - 1)
        assert set(h) == {k for k in mc.LONE + (nb - 1, nb) if 1 <= k <= nb} and set(h.values()) == {1}
        assert mc.histogram(mc.from_histogram(n, cc, h), cc) == h


def test_entries_of_a_bucket_do_not_sit_together():
    n, c = 4096, 11
    v = mc.from_histogram(n, c, {7: 100})
    idx = [i for i, s in enumerate(v) if s]
    assert len(idx) == 100 and all(b - a > 1 for a, b in zip(idx, idx[1:]))


@pytest.mark.parametrize("kind", ["g", "g_lagrange"])
def test_oracle_msm_equals_one_scalar_multiplication(orc, srs, kind):
    toxic, bases = srs
    n = 1 << K_SRS
    fams = _families(n)
    fams["uniform"] = [mc.fr_ints(orc.fill_fr(77, n)), mc.fr_ints(orc.fill_fr(78, 100))]
    fams["zero"] = [[0] * n]
    for name, vectors in fams.items():
        for i, v in enumerate(vectors):
            want = orc.msm(mc.fr_array(v), bases[kind][:len(v)])
            why = mc.check_point(want, want, mc.horner_point(v, toxic, kind, K_SRS))
            assert why is None, (name, i, why)
    assert mc.horner_point([0] * n, toxic, kind, K_SRS) is None


def test_fr_array_is_the_oracles_form(orc):
    vals = [0, 1, 2, R - 1, (R - 1) // 2, 1 << 253]
    a = mc.fr_array(vals)
    assert mc.fr_ints(a) == vals
    for v, row in zip(vals, a):
        assert np.array_equal(row, orc.fr_from_int(v))


def test_a_wrong_point_is_rejected(orc, srs):
    toxic, bases = srs
    n = 1 << K_SRS
    v = mc.from_histogram(n, 7, mc.task_edges(16))
    want = orc.msm(mc.fr_array(v), bases["g"])
    aff = mc.horner_point(v, toxic, "g")
    assert mc.check_point(want, want, aff) is None and mc.check_point(want, want) is None
    for limb in range(12):
        bad = want.copy()
        bad[limb] ^= np.uint64(1)
        assert "oracle" in mc.check_point(bad, want, aff), limb
    # the oracle and the library agreeing on a wrong point: the second judge says so
    v2 = list(v)
    v2[v2.index(0)] = 1
    other = orc.msm(mc.fr_array(v2), bases["g"])
    assert "expected" in mc.check_point(other, other, aff)
    ident = orc.msm(mc.fr_array([0] * n), bases["g"])
    assert mc.check_point(ident, ident, None) is None and mc.check_point(want, want, None) is not None


def test_a_wrong_batch_is_rejected(orc, srs):
    toxic, bases = srs
    n = 1 << K_SRS
    vectors = [mc.from_histogram(n, 7, mc.task_edges(4, first=1 + b), window=b % 3) for b in range(10)] + [[0] * n]
    want = [orc.msm(mc.fr_array(v), bases["g"]) for v in vectors]
    logs = [mc.horner_scalar(v, toxic, "g") for v in vectors]
    assert mc.check_batch(np.stack(want), want, logs) is None
    bad = np.stack(want)
    bad[4, 5] ^= np.uint64(1 << 17)
    assert mc.check_batch(bad, want, logs).startswith("vector 4 of 11 differs from the oracle")
    # the library and the oracle agreeing on two wrong vectors whose plain sum is right: the weights tell
    swapped = [want[1], want[0]] + want[2:]
    assert "is not" in mc.check_batch(np.stack(swapped), swapped, logs)
