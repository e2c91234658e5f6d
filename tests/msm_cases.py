"""Scalar vectors that dictate the bucket histogram of the registered-base MSM (csrc/msm.hip), and a second judge.

The lever: every window of a vector shares ONE bucket set (the table holds 2^(c w) P_i for every window w), and a scalar
k 2^(c w) with 1 <= k <= nb = 2^(c-1) leaves exactly one entry, in bucket k.  So a test can write down the histogram it
wants -- bucket -> population -- and `from_histogram` returns a vector that has it, entry for entry.  What the launch
sequence does after the digits (tasks, hot buckets, the reduction's blocks and strips) depends on that histogram and on
nothing else, so each threshold of `msm_plan` / `msm_scan_kernel` can be given a population on either side of it.

Everything here is Python integers (CPU only, nothing from the library):

  window_digits_ref(s, c)            signed c-bit digits of s, lowest window first (no t*r shift: that is the kernel's choice)
  histogram(scalars, c)              bucket -> entries of a vector of "small" scalars
  from_histogram(n, c, counts, ...)  a vector with exactly that histogram
  task_edges / hot_threshold / span_edges / many_hot / lone_buckets   histograms, each asserting which side it is on
  carry_digits(c) / special(w)       adversarial VALUES for the digit kernels
  horner_point(scalars, toxic, kind) the MSM over an SRS as ONE scalar multiplication: no buckets, no windows
  check_point(got, want, affine)     the comparison of the GPU file: None, or why the point is wrong
  check_batch(...)                   the same for a large batch: the oracle per vector, ONE scalar multiplication for all
"""
from math import gcd

import numpy as np

from field9_ref import G, Q, R, ec_add, ec_mul

MONT = 1 << 256
# halo2curves bn256::Fr::ROOT_OF_UNITY (order 2^28), canonical
ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C
ROOT_ORDER_LOG = 28
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- conversions
def fr_array(ints):
    """Python integers in [0, r) -> uint64[n, 4] Montgomery limbs (the library's scalar form)"""
    out = np.zeros((len(ints), 4), np.uint64)
    for i, v in enumerate(ints):
        if v:
            assert 0 < v < R
            m = v * MONT % R
            out[i] = [(m >> (64 * j)) & M64 for j in range(4)]
    return out


def fr_ints(a):
    """uint64[n, 4] Montgomery limbs -> canonical Python integers"""
    inv = pow(MONT, -1, R)
    return [(int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192) * inv % R for x in np.asarray(a).reshape(-1, 4)]


def _fq_int(limbs):
    return (int(limbs[0]) | int(limbs[1]) << 64 | int(limbs[2]) << 128 | int(limbs[3]) << 192) * pow(MONT, -1, Q) % Q


def affine_of_result(p):
    """uint64[12] normalised Jacobian (x, y, 1) or (0, 1, 0) -> affine integers, None for the identity"""
    p = np.asarray(p).reshape(12)
    x, y, z = _fq_int(p[0:4]), _fq_int(p[4:8]), _fq_int(p[8:12])
    if z == 0:
        assert x == 0 and y == 1, "an identity that is not (0, 1, 0)"
        return None
    assert z == 1, "the point is not normalised"
    return (x, y)


def check_point(got, want, affine=False):
    """The GPU file's comparison.  got, want: uint64[12] normalised points (the library's and the oracle's); they must be
    the same bytes.  affine: the second judge's point ((x, y) integers or None for the identity) when there is one; False
    when the bases are not an SRS.  Returns None, or one line saying which judge disagrees."""
    got = np.asarray(got, dtype=np.uint64).reshape(12)
    want = np.asarray(want, dtype=np.uint64).reshape(12)
    if not np.array_equal(got, want):
        return "differs from the oracle's best_multiexp: limbs %s" % np.flatnonzero(got != want).tolist()
    if affine is not False:
        a = affine_of_result(got)
        if a != affine:
            return "equals the oracle but not (sum c_i w_i) G: %r, expected %r" % (a, affine)
    return None


# ---------------------------------------------------------------- the recoding
def windows_of(c):
    return (255 + c - 1) // c


def window_digits_ref(s, c):
    """The signed digits d_w of s, sum_w d_w 2^(c w) = s, |d_w| <= nb = 2^(c-1): a raw digit above nb is taken as
    digit - 2^c and carries one into the next window (msm_digits_kernel's `carry = d > nb`).  W = ceil(255 / c) digits;
    s < r < 2^254 <= 2^(c W - 1) leaves no carry out of the top window."""
    assert 2 <= c <= 16 and 0 <= s < R
    W, nb, mask = windows_of(c), 1 << (c - 1), (1 << c) - 1
    out, carry = [], 0
    rest = s
    while rest or carry:  # (the windows above the last bit and the last carry hold zeros)
        d = (rest & mask) + carry
        rest >>= c
        carry = 1 if d > nb else 0
        out.append(d - (1 << c) if carry else d)
    assert len(out) <= W, "a carry out of the top window"
    return out + [0] * (W - len(out))


def is_large(s, c):
    """msm_digits_kernel's `large`: any bit at or above c (W - 1) - 1.  Only such scalars may be shifted by t r."""
    return (s >> (c * (windows_of(c) - 1) - 1)) != 0


def histogram(scalars, c):
    """bucket -> number of entries of the vector, all windows together (the vector's one bucket set)"""
    h = {}
    for s in scalars:
        if s == 0:
            continue
        assert not is_large(s, c), "a large scalar: the device may recode s + t r instead"
        for d in window_digits_ref(s, c):
            if d:
                h[abs(d)] = h.get(abs(d), 0) + 1
    return h


def _stride(n):
    """an odd stride near n / phi that is coprime to n: consecutive entries land far apart"""
    s = max(1, int(n * 0.6180339887)) | 1
    while gcd(s, n) != 1:
        s += 2
    return s


def from_histogram(n, c, counts, window=0):
    """n scalars (Python integers) whose histogram is exactly `counts` (bucket -> population), zeros elsewhere.  Entry j
    of the histogram (buckets in ascending order, a bucket's entries one after the other) goes to point (j * stride) % n
    with stride coprime to n, so the entries of one bucket never sit contiguously; the first n entries take window
    `window`, the next n the window above, and so on -- a histogram of more than n entries (hot buckets at K = 48, n = 300)
    spends several windows of the same points."""
    W, nb = windows_of(c), 1 << (c - 1)
    total = sum(counts.values())
    assert all(1 <= k <= nb and v >= 0 for k, v in counts.items()), "bucket outside 1 .. nb"
    layers = (total + n - 1) // n
    assert window + layers <= W - 1, "the top window is not free for a chosen bucket"
    stride = _stride(n)
    out = [0] * n
    j = 0
    for k in sorted(counts):
        for _ in range(counts[k]):
            w = window + j // n
            out[(j * stride) % n] += k << (c * w)
            j += 1
    want = {k: v for k, v in counts.items() if v}
    assert histogram(out, c) == want, "the vector does not have the histogram asked for"
    return out


# ---------------------------------------------------------------- what msm_plan / msm_scan_kernel make of a population
def default_window_bits(n):
    """default_window_bits (csrc/msm.hip) without the tuning override"""
    lg = n.bit_length() - 1
    c = lg - 2 if lg >= 14 else lg - 1
    return min(16, max(4, c))


def default_k(latency, n):
    """msm_plan: `p.K = ...` -- 16 / 32 / 48 by n in the latency form, 48 in the throughput form"""
    if not latency:
        return 48
    return 48 if n >= 1 << 17 else 32 if n >= 1 << 16 else 16


def default_heavy(latency):
    """msm_plan: `p.heavy_thr = ...` -- MSM_HEAVY = 16, MSM_HEAVY_THROUGHPUT = 4"""
    return 16 if latency else 4


def tasks(v, K):
    """msm_scan_kernel: `nt = (v + MSM_K - 1) / MSM_K`"""
    return (v + K - 1) // K


def task_lengths(v, K):
    """msm_accumulate_kernel: `share = total / nt, extra = total % nt` -- the task lengths of a bucket of v entries"""
    nt = tasks(v, K)
    return [v // nt + (1 if j < v % nt else 0) for j in range(nt)]


def is_hot(v, K, thr):
    """msm_scan_kernel: `if (nt > heavy_thr)`"""
    return tasks(v, K) > thr


def heavy_span(partials):
    """msm_heavy_kernel: `span = 32; while (span < t1 - t0 && span < 256) span <<= 1`"""
    span = 32
    while span < partials and span < 256:
        span <<= 1
    return span


# ---------------------------------------------------------------- histogram families
def task_edges(K, first=1):
    """Buckets first .. first + 7 holding 1, K-1, K, K+1, 2K-1, 2K, 2K+1, 3K+1 entries: either side of
    msm_scan_kernel's `nt = (v + MSM_K - 1) / MSM_K` at one, two and three tasks, and task lengths `v / nt` with and
    without the `extra` of msm_accumulate_kernel's `share = total / nt, extra = total % nt`."""
    pops = [1, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 3 * K + 1]
    assert [tasks(v, K) for v in pops] == [1, 1, 1, 2, 2, 2, 3, 4]
    for v in pops:
        ls = task_lengths(v, K)
        assert sum(ls) == v and max(ls) - min(ls) <= 1 and max(ls) <= K
    assert task_lengths(2 * K, K) == [K, K] and task_lengths(2 * K - 1, K) == [K, K - 1]  # extra = 0, extra = 1
    return {first + i: v for i, v in enumerate(pops)}


def hot_threshold(K, thr, entries):
    """Buckets 1 .. 4 holding thr K - 1, thr K, thr K + 1 and (thr + 1) K + 1 entries, bucket 5 the rest of `entries`:
    either side of msm_scan_kernel's `if (nt > heavy_thr)` -- thr tasks stay with the reduction's own lane, thr + 1 go to
    msm_heavy / msm_heavy_groups.  (`entries` is n while the four fit one window of n points, a multiple of n beyond.)"""
    pops = [thr * K - 1, thr * K, thr * K + 1, (thr + 1) * K + 1]
    assert [is_hot(v, K, thr) for v in pops] == [False, False, True, True]
    assert [tasks(v, K) for v in pops] == [thr, thr, thr + 1, thr + 2]
    rest = entries - sum(pops)
    assert rest > 0, "no room for the rest bucket"
    h = {i + 1: v for i, v in enumerate(pops)}
    h[5] = rest
    return h


def span_edges(K):
    """Hot buckets with 32, 33, 64, 65, 256 and 257 task partials (K p entries for p = 32, 64, 256, and one more entry for
    p + 1): msm_heavy_kernel's `while (span < t1 - t0 && span < 256) span <<= 1` at the ends of 32 / 64 / 128 / 256, and
    past 256 where a lane takes two partials.  Meant for K = 4, HEAVY = 1: 2819 entries, one window of n = 4096."""
    h, k = {}, 3
    for p in (32, 64, 256):
        h[k], h[k + 1] = K * p, K * p + 1
        k += 5
    parts = [tasks(v, K) for _, v in sorted(h.items())]
    assert parts == [32, 33, 64, 65, 256, 257]
    assert [heavy_span(p) for p in parts] == [32, 64, 64, 128, 256, 256]
    return h


def many_hot(count, each, first=1):
    """`count` buckets of `each` entries (first .. first + count - 1).  With `each` past the hot threshold: either side of
    msm_heavy_kernel's flat grid of MSM_HEAVY_WGS = 256 workgroups (`for (h = first; h < nh; h += gridDim.x)`) and of one
    round of msm_heavy_groups_kernel (`stride = gridDim.x * NG` = 4096 groups)."""
    return {first + i: each for i in range(count)}


LONE = (1, 2, 8, 9, 63, 64, 65, 128, 129, 255, 256, 257, 1024, 1025, 2048, 2049)


def lone_buckets(c):
    """One entry each in the buckets either side of a reduction block (64 / 128 / 256 buckets: msm_bucket_scan_kernel's
    `k = blk * RB + j + 1`), of a strip (8: msm_strip_kernel's `k = j * S + s + 1`) and of a summing lane's strips
    (msm_strip_sum_kernel's `jj = l * per + t`), and in nb - 1 and nb.  The sum is sum_k k P_k: every bucket's weight is
    on show."""
    nb = 1 << (c - 1)
    ks = sorted({k for k in LONE + (nb - 1, nb) if 1 <= k <= nb})
    assert nb in ks
    return {k: 1 for k in ks}


# ---------------------------------------------------------------- adversarial values
def special(w):
    """The adversarial scalars of test_free_position_digits_on_adversarial_scalars (w: the digit width): runs of ones,
    alternating bits, single bits and the extreme values across every 32-bit limb boundary."""
    sp = [0, 1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 253), (1 << 253) - 1, (1 << 253) + 1]
    sp += [1 << e for e in (28, 29, 30, 31, 32, 33, 47, 48, 63, 64, 65, 95, 96, 127, 128, 191, 192, 224, 250, 252)]
    sp += [(1 << e) - 1 for e in (15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 200, 253)]
    sp += [int("aa" * 31, 16), int("55" * 31, 16), int("ff" * 31, 16) % R, int("0f" * 31, 16), int("f0" * 31, 16) % R]
    sp += [((1 << w) - 1) << s for s in (0, 1, 17, 31, 32, 33, 48, 64 - w, 64, 200)]
    sp += [(((1 << (w - 1)) + 1) << s) % R for s in (0, 15, 31, 32, 63, 64, 100, 230)]
    return [v % R for v in sp]


def carry_digits(c):
    """Values for msm_digits_kernel's `carry = d > nb ? 1u : 0u` and its top-window test (`large`, the t r shift of
    msm_plan's `tbits`): nb (the largest digit that does NOT carry), nb + 1 (the smallest that does), 2^c - 1 and 2^c at
    every window position; nb + 1 in every window (a carry through all of them); r - 1, r - 2, (r +- 1) / 2; special(c).
    Only values below r are kept, which none of the four is in the top window: there the scalar's own largest digit,
    the one below it and 1 stand in."""
    W, nb = windows_of(c), 1 << (c - 1)
    heads = sorted({nb, nb + 1, (1 << c) - 1, 1 << c})
    vals = []
    for w in range(W):
        for k in heads:
            v = k << (c * w)
            if v < R:
                vals.append(v)
            else:
                assert w >= W - 2, "only the top of the scalar can pass r"
    # (nb 2^(c (W - 1)) = 2^(c W - 1) >= 2^254 > r: none of the four fits the top window; a scalar's own top digit is
    #  at most (r - 1) >> c (W - 1), so that one, the one below and 1 stand there instead -- where the window holds a bit
    #  of r at all: at c = 2 it starts at bit 254 and only a carry or the t r shift reaches it)
    assert all(v >> (c * (W - 1)) in (0, 1) for v in vals)  # (2^c in window W - 2 is the top window's 1)
    top = (R - 1) >> (c * (W - 1))
    assert (top > 0) == (c * (W - 1) <= 253) and top < nb
    vals += [k << (c * (W - 1)) for k in sorted({1, top - 1, top}) if 1 <= k <= top]
    for k in (nb, nb + 1):  # either side of the carry, at every window below the top
        for w in range(W - 1):
            if k << (c * w) >= R:
                continue
            d = window_digits_ref(k << (c * w), c)
            assert d[w] == (nb if k == nb else -(nb - 1)) and d[w + 1] == (0 if k == nb else 1)
    # a carry through every window: nb + 1 in each of the m lowest windows, m as large as a scalar below r allows (W - 1,
    # or W - 2 where c (W - 1) = 254), so that the last carry arrives alone in window m ...
    m = W - 1
    while sum((nb + 1) << (c * w) for w in range(m)) >= R:
        m -= 1
    assert m >= W - 2
    chain = sum((nb + 1) << (c * w) for w in range(m))
    cd = window_digits_ref(chain, c)
    # (every window below m carries: its digit is nb + 2 - 2^c, negative, or zero at c = 2)
    assert cd[0] == -(nb - 1) and all(d == nb + 2 - (1 << c) for d in cd[1:m]) and cd[m] == 1 and not any(cd[m + 1:])
    vals.append(chain)
    full = chain + ((nb + 1) << (c * m))  # ... and one window further where that is still a scalar
    if full < R:
        vals.append(full)
    vals += [R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
    vals += special(c)
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    assert all(0 <= v < R for v in out)
    for v in out:
        assert sum(d << (c * w) for w, d in enumerate(window_digits_ref(v, c))) == v
    return out


# ---------------------------------------------------------------- the second judge
def horner_scalar(scalars, toxic, kind, k=None):
    """The discrete logarithm of sum_i c_i B_i for the first len(scalars) points of the SRS of toxic scalar `toxic`:
    kind "g": B_i = toxic^i G, so it is sum_i c_i toxic^i mod r; kind "g_lagrange": B_i = L_i(toxic) G over the 2^k-th
    roots of unity, L_i(x) = omega^i (x^n - 1) / (n (x - omega^i))."""
    acc = 0
    if kind == "g":
        p = 1
        for c_i in scalars:
            if c_i:
                acc += c_i * p
            p = p * toxic % R
    else:
        assert kind == "g_lagrange" and k is not None and len(scalars) <= 1 << k
        n = 1 << k
        omega = pow(ROOT_OF_UNITY, 1 << (ROOT_ORDER_LOG - k), R)
        assert pow(omega, n, R) == 1 and (k == 0 or pow(omega, n // 2, R) == R - 1)
        lead = (pow(toxic, n, R) - 1) * pow(n, -1, R) % R
        wi = 1
        for c_i in scalars:
            if c_i:
                acc += c_i * (wi * lead % R * pow((toxic - wi) % R, -1, R) % R)
            wi = wi * omega % R
    return acc % R


def horner_point(scalars, toxic, kind, k=None):
    """sum_i c_i B_i for the first len(scalars) points of the SRS of toxic scalar `toxic`, as ONE scalar multiplication
    (field9_ref.ec_mul, the affine chord-tangent law): affine integers, None for the identity."""
    return ec_mul(horner_scalar(scalars, toxic, kind, k), G)


def check_batch(got, want, scalars_of):
    """A whole batch: every got[b] must be want[b], byte for byte, and sum_b (b + 1) got[b] must be the ONE scalar
    multiplication (sum_b (b + 1) a_b) G with a_b = horner_scalar of vector b (the weights keep two wrong vectors from
    cancelling).  scalars_of: the a_b.  None, or one line."""
    for b in range(len(want)):
        why = check_point(got[b], want[b])
        if why:
            return "vector %d of %d %s" % (b, len(want), why)
    acc, total = None, 0
    for b, a in enumerate(scalars_of):
        acc = ec_add(acc, ec_mul(b + 1, affine_of_result(got[b])))
        total += (b + 1) * a
    if acc != ec_mul(total % R, G):
        return "every vector equals the oracle, but sum_b (b + 1) P_b is not (sum_b (b + 1) a_b) G"
    return None
