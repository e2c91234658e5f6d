"""The registered-base MSM (csrc/msm.hip) at its task, hot-bucket and reduction edges, in both forms.

tests/msm_cases.py dictates the bucket histogram of a vector (a scalar k 2^(c w) leaves one entry, in bucket k), so every
threshold of msm_plan / msm_scan_kernel and every grid, span and block boundary of the kernels behind them gets a
population on either side.  Every result must be the oracle's best_multiexp, byte for byte, and -- the bases being the
first n points of an SRS -- the one scalar multiplication (sum_i c_i w_i) G of msm_cases.horner_point, which shares no
bucket, window or table with either."""
import contextlib

import numpy as np
import pytest

import msm_cases as mc

pytestmark = pytest.mark.gpu

SEED = 0x5EED
K_SRS = 12
FORMS = ["latency", "throughput"]


class World:
    """One SRS (k = 12, both base kinds), a context per form, and the base sets registered so far."""

    def __init__(self, zg, orc):
        self.zg, self.orc = zg, orc
        prm = orc.params_new(K_SRS, SEED)
        self.toxic_fr = orc.fill_fr(SEED, 1)[0]
        self.toxic = orc.fr_to_int(self.toxic_fr)
        self.points = {"g": prm.g_np(), "g_lagrange": prm.g_lagrange_np()}
        self.k = {"g": K_SRS, "g_lagrange": K_SRS}
        self.ctx = {"latency": zg.Ctx(0), "throughput": zg.Ctx(0)}
        self.ctx["throughput"].set_msm_latency(False)
        self.bases = {}

    def registered(self, form, kind, n, c=0):
        key = (form, kind, n, c)
        if key not in self.bases:
            b = self.ctx[form].register_bases(self.points[kind][:n], c)
            assert b.window_bits == (c or mc.default_window_bits(n))
            self.bases[key] = b
        return self.bases[key]

    def close(self):
        for b in self.bases.values():
            b.free()
        for c in self.ctx.values():
            c.close()

    def check(self, form, kind, n_bases, c, vectors, tag=""):
        """vectors: lists of Python integers, all of one length <= n_bases; ONE batched launch sequence, every vector
        against its own oracle point and its own scalar multiplication"""
        bases = self.registered(form, kind, n_bases, c)
        arr = np.stack([mc.fr_array(v) for v in vectors])
        got = self.ctx[form].msm_batch(bases, arr)
        pts = self.points[kind]
        where = f"{tag} {form} {kind} n={len(vectors[0])} c={c}"
        # (the oracle's thread pool costs more than it saves on a vector of a few hundred entries)
        want = [self.orc.msm(arr[b], pts[:len(v)], threads=1 if 4 * sum(1 for s in v if s) < len(v) else 8)
                for b, v in enumerate(vectors)]
        if len(vectors) > 8:  # one scalar multiplication for the whole batch (msm_cases.check_batch)
            why = mc.check_batch(got, want, [mc.horner_scalar(v, self.toxic, kind, self.k[kind]) for v in vectors])
            assert why is None, f"{where}: {why}"
            return
        for b, v in enumerate(vectors):
            why = mc.check_point(got[b], want[b], mc.horner_point(v, self.toxic, kind, self.k[kind]))
            assert why is None, f"{where} vector {b} of {len(vectors)}: {why}"


@pytest.fixture(scope="module")
def world(zg, orc):
    w = World(zg, orc)
    yield w
    w.close()


@contextlib.contextmanager
def knobs(zg, **kw):
    """tuning knobs for the duration of a case; None leaves a knob alone"""
    before = {name: zg.tuning_get(name) for name, v in kw.items() if v is not None}
    try:
        for name in before:
            zg.tuning_set(name, kw[name])
        yield
    finally:
        for name, v in before.items():
            zg.tuning_set(name, v)


def k_knob(form):
    return "ZG_MSM_K_LAT" if form == "latency" else "ZG_MSM_K"


def uniform(orc, seed, n):
    return mc.fr_ints(orc.fill_fr(seed, n))


# ---------------------------------------------------------------- tasks
@pytest.mark.parametrize("K", [None, 4, 120])
@pytest.mark.parametrize("form", FORMS)
def test_task_edges(world, zg, form, K):
    """1, K-1, K, K+1, 2K-1, 2K, 2K+1, 3K+1 entries per bucket at the form's own K and at the knob's two ends (at 120 the
    length classes of msm_scan_kernel reach bin 120 of 128); in the lowest buckets and in the highest, window 0 and 3"""
    n = 1 << 12
    c = mc.default_window_bits(n)
    nb = 1 << (c - 1)
    k_eff = K or mc.default_k(form == "latency", n)
    with knobs(zg, **{k_knob(form): K}):
        for kind in ("g", "g_lagrange"):
            vectors = [mc.from_histogram(n, c, mc.task_edges(k_eff)),
                       mc.from_histogram(n, c, mc.task_edges(k_eff, first=nb - 7), window=3)]
            world.check(form, kind, n, 0, vectors, f"task_edges({k_eff})")


@pytest.fixture(scope="module")
def big(world):
    """2^17 points s^i G from zg_params_new (the oracle's own setup of that size takes minutes), registered once on the
    latency-form context; horner_point judges them as it judges the oracle's"""
    g, _ = world.ctx["latency"].params_new(17, world.toxic_fr)
    world.points["big"] = g
    bases = world.ctx["latency"].register_bases(g)
    assert bases.window_bits == 15
    yield g, bases
    bases.free()


@pytest.mark.parametrize("n, K, pair", [((1 << 16) - 1, 16, True), (1 << 16, 32, False), (1 << 17, 48, False)])
def test_task_edges_where_the_latency_form_changes_its_task_size(world, big, n, K, pair):
    """msm_plan: `k_lat_default = n >= 2^17 ? 48 : n >= 2^16 ? 32 : 16` and `pair_tasks = msm_pair && N < 2^16` -- n scalars
    against the same 2^17 registered points, the populations K-1 .. 3K+1 of that n's K"""
    g, bases = big
    assert mc.default_k(True, n) == K and (n < 1 << 16) == pair
    c = 15
    v = mc.from_histogram(n, c, mc.task_edges(K, first=(1 << (c - 1)) - 7))
    arr = mc.fr_array(v)
    got = world.ctx["latency"].msm(bases, arr)
    want = world.orc.msm(arr, g[:n], threads=8)
    why = mc.check_point(got, want, mc.horner_point(v, world.toxic, "g"))
    assert why is None, why


# ---------------------------------------------------------------- hot buckets
@pytest.mark.parametrize("heavy", [None, 1, 64])
@pytest.mark.parametrize("form", FORMS)
def test_hot_threshold(world, zg, form, heavy):
    """thr K - 1 and thr K entries stay with the reduction's lane, thr K + 1 and (thr + 1) K + 1 go to msm_heavy /
    msm_heavy_groups; the rest of the entries in a fifth bucket.  (K, thr) = (16, 16) and (48, 4), thr = 1 and 64."""
    n = 1 << 12
    c = mc.default_window_bits(n)
    latency = form == "latency"
    K, thr = mc.default_k(latency, n), heavy or mc.default_heavy(latency)
    need = 4 * thr * K + K + 2
    h = mc.hot_threshold(K, thr, n * ((need + n - 1) // n))
    with knobs(zg, ZG_MSM_HEAVY=heavy):
        world.check(form, "g", n, 0, [mc.from_histogram(n, c, h)], f"hot_threshold({K}, {thr})")
        world.check(form, "g_lagrange", n, 0, [mc.from_histogram(n, c, h, window=1)], f"hot_threshold({K}, {thr})")


@pytest.mark.parametrize("form", FORMS)
def test_hot_spans(world, zg, form):
    """hot buckets of 32, 33, 64, 65, 256 and 257 task partials: msm_heavy_kernel's tree over 32 / 64 / 128 / 256 slots,
    and msm_heavy_groups_kernel's sixteen lanes taking 2 .. 17 partials each"""
    n = 1 << 12
    c = mc.default_window_bits(n)
    with knobs(zg, **{k_knob(form): 4, "ZG_MSM_HEAVY": 1}):
        world.check(form, "g", n, 0, [mc.from_histogram(n, c, mc.span_edges(4))], "span_edges")


@pytest.mark.parametrize("count", [255, 256, 257])
@pytest.mark.parametrize("form", FORMS)
def test_hot_counts_of_one_vector(world, zg, form, count):
    """255 / 256 / 257 hot buckets in ONE vector: msm_heavy_kernel's flat grid of 256 workgroups comes round again"""
    n, c = 1 << 12, 11
    with knobs(zg, **{k_knob(form): 4, "ZG_MSM_HEAVY": 1}):
        world.check(form, "g", n, c, [mc.from_histogram(n, c, mc.many_hot(count, 5, first=3))], f"many_hot({count})")


def test_hot_counts_past_one_round_of_groups(world, zg):
    """9 vectors of 513 hot buckets: 4617 (vector, bucket) pairs, more than the 4096 groups of one round of
    msm_heavy_groups_kernel; vectors differ in where their buckets start and in the window"""
    n, c = 1 << 12, 11
    vectors = [mc.from_histogram(n, c, mc.many_hot(513, 5, first=1 + 50 * b), window=b % 4) for b in range(9)]
    with knobs(zg, ZG_MSM_K=4, ZG_MSM_HEAVY=1):
        world.check("throughput", "g", n, c, vectors, "many_hot(513) x 9")


@pytest.mark.parametrize("B", [6, 70])
@pytest.mark.parametrize("form", FORMS)
def test_hot_and_cold_vectors_interleave(world, form, B):
    """none, many, none, one, many, none, ...: the flat (vector, hot bucket) index of msm_heavy_kernel (`item`) and
    msm_heavy_groups_kernel (`first_of`) across vectors that bring 0, 20 and 1 pairs, at the forms' own K and threshold.
    At B = 70 the launch holds 23 * 20 + 12 = 472 pairs: the flat grid wraps inside a vector that is not the first."""
    n = 1 << 12
    c = mc.default_window_bits(n)
    latency = form == "latency"
    K, thr = mc.default_k(latency, n), mc.default_heavy(latency)
    hot = thr * K + 1
    assert mc.is_hot(hot, K, thr) and not any(mc.is_hot(v, K, thr) for v in mc.task_edges(K).values())
    vectors = []
    for b in range(B):
        kind = ("none", "many", "none", "one", "many", "none")[b % 6]
        first = 1 + 7 * (b // 6)
        if kind == "none":
            h = mc.task_edges(K, first=first)
        elif kind == "one":
            h = {first + 2: hot}
        else:
            h = mc.many_hot(20, hot, first=first)
        vectors.append(mc.from_histogram(n, c, h, window=b % 3))
    assert sum(20 if b % 6 in (1, 4) else 1 if b % 6 == 3 else 0 for b in range(B)) == (41 if B == 6 else 472)
    world.check(form, "g", n, 0, vectors, "interleave")


# ---------------------------------------------------------------- batch sizes
@pytest.mark.parametrize("B", [1, 7, 8, 9, 63, 64, 65])
def test_batch_sizes_around_the_scatter_grid(world, B):
    """msm_launch_sort: `by_xcd = B >= 64` (the flat grid laid out XCD by XCD, groups of eight vectors, the last one
    partial at 65), at n = 300: two scatter chunks of 256, the second partial.  Uniform, task-edge and zero vectors mixed,
    each against its own point."""
    n = 300
    c = mc.default_window_bits(n)
    assert c == 7
    vectors = []
    for b in range(B):
        kind = (b + B) % 3
        if kind == 0:
            vectors.append(uniform(world.orc, 1000 + b, n))
        elif kind == 1:
            vectors.append(mc.from_histogram(n, c, mc.task_edges(48, first=1 + b % 50), window=b % 5))
        else:
            vectors.append([0] * n)
    world.check("throughput", "g", n, 0, vectors, f"B={B}")


# ---------------------------------------------------------------- the reduction's geometry
def _geometry_vectors(orc, n, c, B):
    """launches of B vectors: B = 1 -> the lone buckets alone, then uniform mass alone; else one launch that mixes them"""
    lone = mc.lone_buckets(c)
    if B == 1:
        return [[mc.from_histogram(n, c, lone)], [uniform(orc, 40 + c, n)]]
    half = uniform(orc, 80 + c, n // 2) + [0] * (n - n // 2)
    return [[mc.from_histogram(n, c, lone), uniform(orc, 40 + c, n), mc.from_histogram(n, c, lone, window=1), [0] * n,
             uniform(orc, 60 + c, n), mc.from_histogram(n, c, lone, window=2), half][:B]]


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("c", [7, 8, 11, 13, 14, 16])
def test_latency_reduction_blocks(world, c, B):
    """msm_plan's `quad_fits` / `want` / `p.rb`: 64-bucket blocks with four lanes while nblk64 * B <= CUs (c = 13: B = 1
    yes, B = 7 no), 128 with two beyond, 256 at c = 16; one entry each side of every block edge, and uniform mass"""
    n = 1 << 10
    for vectors in _geometry_vectors(world.orc, n, c, B):
        world.check("latency", "g", n, c, vectors, f"blocks B={B}")


@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("rb", [64, 128, 256])
def test_latency_reduction_instances(world, zg, rb, lanes):
    """the five (L, RB) instances of msm_bucket_scan / msm_bucket_sum at c = 11 (16, 8 and 4 blocks)"""
    n, c = 1 << 10, 11
    with knobs(zg, ZG_MSM_RB=rb, ZG_MSM_LANES=lanes):
        for vectors in _geometry_vectors(world.orc, n, c, 1) + _geometry_vectors(world.orc, n, c, 3):
            world.check("latency", "g", n, c, vectors, f"RB={rb} L={lanes}")


@pytest.mark.parametrize("c, strip", [(4, None), (11, None), (13, None), (16, None), (13, 2), (13, 16)])
def test_throughput_strips(world, zg, c, strip):
    """msm_plan: `nstrips = nb / strip`, `strip_per` doubling while strip_per * 256 < nstrips -- 1, 128, 512 and 4096
    strips of eight (strip_per 1, 1, 2, 16), 2048 of two and 256 of sixteen at c = 13"""
    n = 1 << 10
    nstrips = ((1 << (c - 1)) + (strip or 8) - 1) // (strip or 8)
    assert (c, strip, nstrips) in ((4, None, 1), (11, None, 128), (13, None, 512), (16, None, 4096), (13, 2, 2048), (13, 16, 256))
    with knobs(zg, ZG_MSM_STRIP=strip):
        for vectors in _geometry_vectors(world.orc, n, c, 1) + _geometry_vectors(world.orc, n, c, 3):
            world.check("throughput", "g", n, c, vectors, f"strip={strip}")


# ---------------------------------------------------------------- digits of the window form
@pytest.mark.parametrize("c", range(2, 17))
@pytest.mark.parametrize("form", FORMS)
def test_window_digits_on_adversarial_scalars(world, form, c):
    """msm_digits_kernel at every window size, those with c W = 255 among them (c = 3, 5, 15: msm_plan's `spare` is 0 and
    `tbits` off): the carry's two sides at every window position, a carry through every window, the scalars around r and
    r / 2 -- alone, scattered in uniform mass -- and r - 1 everywhere"""
    assert ((c * mc.windows_of(c) - 255) == 0) == (c in (3, 5, 15))
    n = 1 << 9
    vals = mc.carry_digits(c)
    rng = np.random.default_rng(c)
    vectors = []
    for i in range(0, len(vals), n):
        chunk = vals[i:i + n]
        vectors.append(chunk + [0] * (n - len(chunk)))
        mass = uniform(world.orc, 300 + 20 * c + i // n, n)
        for p, v in zip(rng.permutation(n)[:len(chunk)], chunk):
            mass[p] = v
        vectors.append(mass)
    vectors.append([mc.R - 1] * n)
    world.check(form, "g_lagrange", n, c, vectors, "carry_digits")
