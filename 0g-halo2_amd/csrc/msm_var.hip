// Pippenger multi-scalar multiplication over CALLER-SUPPLIED points on BN254 G1 for gfx950 -- halo2_proofs::arithmetic::
// best_multiexp(coeffs, bases) with the bases as an argument (halo2_proofs v2023_04_20 src/arithmetic.rs), for points that
// are used once: nothing is built ahead of time and nothing stays resident.
//
// msm.hip multiplies against registered base sets: every point gets ceil(255/c) window-shifted affine copies (254
// dependent doublings and as many conversions to affine PER POINT) so that all windows share one bucket set and the
// window combine disappears.  Here that table does not exist.  With W = ceil(255/c) windows an MSM of `batch` vectors over
// n points is batch x W "virtual vectors": vector (b, w) holds window w's signed digit of every scalar of b against the
// UNSHIFTED point i, has a bucket set of its own, and is the one-bucket-set problem of msm.hip; the windows meet in a
// doubling ladder of 254 dependent doublings per vector -- the serial chain the tables exist to avoid, paid once per
// vector instead of once per point, and by all vectors of a batch side by side.
//
//   msm_var_points      the n points once into the x * 2^261 form of field9.h (the identity stays (0, 0))
//   msm_var_digits      scalars -> canonical integers -> signed c-bit digits (msm_var_digits.h), dig[b][w][i]
//   msm_var_sort        one workgroup per (b, w): bucket histogram in LDS, scan, entries into bucket order; task offsets
//   msm_var_accumulate  one lane per task (at most K points of one bucket; a crowded bucket is cut into tasks): mixed
//                       additions in XYZZ on nine 29-bit limbs
//   msm_var_merge       a bucket's task sums, sixteen per lane: what a crowded bucket leaves the reduction is short again
//   msm_var_strip       sum_k k B_k, stage 1: a lane walks a strip of buckets from the top (run += B_k, loc += run)
//   msm_var_strip_sum   ... stage 2, one workgroup per (b, w): S_w = sum loc + strip * sum_j j U_j
//   msm_var_horner      one lane per vector: acc <- 2^c acc + S_w from w = W - 1 down to 0
// No kernel waits for another workgroup or for the host; every loop is bounded by a launch argument or by counts the
// sort derived from n.  The additions of field9.h settle equal-x operands (P + P, P + (-P)), which a caller's points can
// make routine here: repeated points, a point and its negative, identities are all accepted.
#include "msm.h"
#include "field9.h"
#include "msm_var_digits.h"

namespace zg {

namespace {

constexpr uint32_t VAR_K = 16;            // points per accumulate task
constexpr uint32_t VAR_MAX_SPLIT = 1024;  // tasks per bucket at most (a bucket of more than 16 384 points gets longer tasks)
constexpr uint32_t VAR_K2 = 16;           // task sums per merge task (msm_var_merge)
constexpr uint32_t VAR_STRIP = 8;         // buckets per lane of msm_var_strip at most (powers of two)
constexpr uint32_t VAR_SUM_LANES = 256;   // workgroup of msm_var_strip_sum
constexpr size_t VAR_MAX_BATCH = 256;     // include/zg_halo2.h: ZG_MSM_VAR_MAX_BATCH

__device__ __forceinline__ Fe var_ld_fe(const Fe* p) {
    Fe r;
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}
__device__ __forceinline__ void var_st_fe(Fe* p, const Fe& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// tasks of a bucket with v entries: ceil(v / K), at most VAR_MAX_SPLIT (a bucket that holds more gets longer tasks)
__device__ __forceinline__ uint32_t var_tasks(uint32_t v, uint32_t K) {
    const uint32_t nt = (v + K - 1) / K;
    return nt > VAR_MAX_SPLIT ? VAR_MAX_SPLIT : nt;
}
// merge tasks of a bucket with nt task sums: ceil(nt / K2), what msm_var_strip is left to add up in sequence
__device__ __forceinline__ uint32_t var_tasks2(uint32_t nt) { return (nt + VAR_K2 - 1) / VAR_K2; }

// lane t's bucket: the k with off[k] <= t < off[k + 1] (off[0] = 0, off non-decreasing, off[nb + 1] > t)
__device__ __forceinline__ uint32_t var_bucket_of(const uint32_t* __restrict__ off, uint32_t nb, uint32_t t) {
    uint32_t lo = 0, hi = nb + 1;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the j-th of `parts` even shares of [first, first + total): lengths differ by one at most
__device__ __forceinline__ void var_share(uint32_t first, uint32_t total, uint32_t parts, uint32_t j, uint32_t& start, uint32_t& len) {
    const uint32_t share = total / parts, extra = total % parts;
    start = first + j * share + (j < extra ? j : extra);
    len = share + (j < extra ? 1u : 0u);
}

}  // namespace

// pts[i] = bases[i] with both coordinates times 2^5: the library's x * 2^256 form -> the x * 2^261 form (packed,
// canonical) the accumulation unpacks into nine limbs, as row 0 of msm_table_kernel; (0, 0) stays (0, 0).
__global__ __launch_bounds__(256) void msm_var_points_kernel(const Affine* __restrict__ bases, Affine* __restrict__ pts, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fe c261 = Fq9Params::c261_fe();
    var_st_fe(&pts[i].x, Fq::mul(var_ld_fe(&bases[i].x), c261));
    var_st_fe(&pts[i].y, Fq::mul(var_ld_fe(&bases[i].y), c261));
}

// dig[(b W + w) n + i] = window w's signed digit of scalar i of vector b (bucket | sign << 31, 0 = none)
__global__ __launch_bounds__(256) void msm_var_digits_kernel(const Fe* __restrict__ scalars, size_t stride, uint32_t n, uint32_t c,
                                                             uint32_t windows, uint32_t* __restrict__ dig) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    const Fe s = Fr::to_raw(var_ld_fe(scalars + (size_t)b * stride + i));  // below r < 2^254
    msm_var_recode(s.l, c, windows, dig + (size_t)b * windows * n + i, n);
}

// One 1024-lane workgroup per virtual vector v = b W + w.  cnt[k] (LDS) counts the entries of bucket k = 1 .. 2^(c-1);
// a strip scan over the lanes turns the counts into entry offsets boff[v][k] (bucket k's entries are
// sorted[v][boff[k] .. boff[k+1]); boff[nb+1] = the vector's entries) and the task counts into task offsets toff[v][k]
// (toff[nb+1] = the vector's tasks) and those of the merge tasks, toff2; then every entry takes the next free slot of its bucket (an LDS atomic on the
// bucket's cursor: the order inside a bucket is whatever the lanes make it, the bucket's SUM does not depend on it).
// No global atomics.  Scalars that all hold the same digit serialise on one LDS word: right, not fast.
__global__ __launch_bounds__(1024) void msm_var_sort_kernel(const uint32_t* __restrict__ dig, uint32_t n, uint32_t c, uint32_t K,
                                                            uint32_t* __restrict__ boff, uint32_t* __restrict__ toff,
                                                            uint32_t* __restrict__ toff2, uint32_t* __restrict__ sorted) {
    extern __shared__ uint32_t cnt[];  // [nb + 2]
    __shared__ uint32_t se[1024], st[1024], s2[1024];
    const uint32_t nb = 1u << (c - 1), v = blockIdx.x, tid = threadIdx.x;
    const uint32_t* db = dig + (size_t)v * n;
    for (uint32_t k = tid; k < nb + 2; k += 1024) cnt[k] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 1024) {
        const uint32_t k = db[i] & 0x7fffffffu;  // <= nb by the recoding; the guard keeps a violated contract inside LDS
        if (k != 0 && k <= nb) atomicAdd(&cnt[k], 1u);
    }
    __syncthreads();
    const uint32_t per = (nb + 2 + 1023) / 1024;
    uint32_t lo = tid * per, hi = lo + per;
    if (lo > nb + 2) lo = nb + 2;
    if (hi > nb + 2) hi = nb + 2;
    uint32_t es = 0, ts = 0, t2s = 0;
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t nt = var_tasks(cnt[k], K);
        es += cnt[k];
        ts += nt;
        t2s += var_tasks2(nt);
    }
    se[tid] = es;
    st[tid] = ts;
    s2[tid] = t2s;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        uint32_t ve = 0, vt = 0, v2 = 0;
        if (tid >= o) {
            ve = se[tid - o];
            vt = st[tid - o];
            v2 = s2[tid - o];
        }
        __syncthreads();
        se[tid] += ve;
        st[tid] += vt;
        s2[tid] += v2;
        __syncthreads();
    }
    uint32_t eb = se[tid] - es, tb = st[tid] - ts, t2b = s2[tid] - t2s;
    uint32_t* bo = boff + (size_t)v * (nb + 2);
    uint32_t* to = toff + (size_t)v * (nb + 2);
    uint32_t* to2 = toff2 + (size_t)v * (nb + 2);
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t cv = cnt[k], nt = var_tasks(cv, K);
        bo[k] = eb;
        to[k] = tb;
        to2[k] = t2b;
        cnt[k] = eb;  // the bucket's cursor
        eb += cv;
        tb += nt;
        t2b += var_tasks2(nt);
    }
    __syncthreads();
    uint32_t* so = sorted + (size_t)v * n;
    for (uint32_t i = tid; i < n; i += 1024) {
        const uint32_t d = db[i], k = d & 0x7fffffffu;
        if (k != 0 && k <= nb) {
            const uint32_t pos = atomicAdd(&cnt[k], 1u);  // < boff[k+1] <= n
            so[pos] = i | (d & 0x80000000u);              // point (23 bits) | sign
        }
    }
}

// One lane per task.  Lane t of vector v finds its bucket k by bisection over the task offsets (toff[k] <= t < toff[k+1]);
// the bucket's nt tasks share its entries evenly (lengths differ by one at most).  The first point of a task is kept
// affine, the second joins it through xyzz9_from_pair (6 products), the rest are mixed additions (10 products); a pair
// that cancels leaves the sum empty.  Partial sums leave in task order, which is bucket order.
__global__ __launch_bounds__(256) void msm_var_accumulate_kernel(const Affine* __restrict__ pts, uint32_t c,
                                                                 const uint32_t* __restrict__ boff, const uint32_t* __restrict__ toff,
                                                                 const uint32_t* __restrict__ sorted, uint32_t n, uint32_t max_tasks,
                                                                 XYZZ9* __restrict__ partial) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, v = blockIdx.y;
    const uint32_t nb = 1u << (c - 1);
    const uint32_t* to = toff + (size_t)v * (nb + 2);
    const uint32_t* bo = boff + (size_t)v * (nb + 2);
    if (t >= to[nb + 1] || t >= max_tasks) return;  // (tasks <= max_tasks by construction; the second test keeps the store inside)
    const uint32_t k = var_bucket_of(to, nb, t);
    uint32_t start, len;
    var_share(bo[k], bo[k + 1] - bo[k], to[k + 1] - to[k], t - to[k], start, len);
    const uint32_t* so = sorted + (size_t)v * n + start;
    XYZZ9 acc;
    bool inf = true, aff = false;
    for (uint32_t e = 0; e < len; e++) {
        const uint32_t ent = so[e];
        const Affine* src = pts + (ent & 0x7fffffu);
        const F9 qx = f9_unpack(var_ld_fe(&src->x));
        F9 qy = f9_unpack(var_ld_fe(&src->y));
        if (f9_limbs_zero(qx) && f9_limbs_zero(qy)) continue;  // the identity among the caller's points
        if (ent >> 31) qy = f9_neg(qy);
        if (inf) {
            acc.x = qx;
            acc.y = f9_norm(qy);  // (a negated y arrives with negative limbs)
            inf = false;
            aff = true;
        } else if (aff) {
            aff = false;
            xyzz9_from_pair(acc.x, acc.y, qx, qy, acc, inf);
        } else {
            xyzz9_madd(acc, inf, qx, qy);
        }
    }
    if (aff) acc.zz = acc.zzz = Fq9Params::one();
    st_xyzz9(partial + (size_t)v * max_tasks + t, inf ? xyzz9_identity() : acc);
}

// One lane per merge task: the nt task sums of a bucket are shared evenly among its ceil(nt / 16) merge tasks, each a chain
// of full additions.  A bucket of a few points has one task and one merge task (a copy); a CROWDED bucket -- and every
// vector has some: the top window of scalars below r < 2^254 holds only the few bits above c (W - 1), so its n entries meet
// in a handful of buckets, and so do repeated or tiny scalars in window 0 -- leaves msm_var_strip's lane a sixteenth of its
// task sums to add up in sequence (1 300 entries: 82 task sums, 6 merge sums).
__global__ __launch_bounds__(256) void msm_var_merge_kernel(const XYZZ9* __restrict__ partial, const uint32_t* __restrict__ toff,
                                                            const uint32_t* __restrict__ toff2, uint32_t c, uint32_t max_tasks,
                                                            uint32_t max_tasks2, XYZZ9* __restrict__ partial2) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, v = blockIdx.y;
    const uint32_t nb = 1u << (c - 1);
    const uint32_t* to = toff + (size_t)v * (nb + 2);
    const uint32_t* to2 = toff2 + (size_t)v * (nb + 2);
    if (t >= to2[nb + 1] || t >= max_tasks2) return;
    const uint32_t k = var_bucket_of(to2, nb, t);
    uint32_t start, len;
    var_share(to[k], to[k + 1] - to[k], to2[k + 1] - to2[k], t - to2[k], start, len);
    const XYZZ9* pp = partial + (size_t)v * max_tasks;
    XYZZ9 acc = xyzz9_identity();
    for (uint32_t e = 0; e < len && start + e < max_tasks; e++) acc = xyzz9_add(acc, ld_xyzz9(pp + start + e));
    st_xyzz9(partial2 + (size_t)v * max_tasks2 + t, acc);
}

// sum_k k B_k over the buckets k = 1 .. nb of one virtual vector, stage 1 (the scheme of msm_strip_kernel): lane j walks
// the buckets [j S + 1, (j + 1) S] from the top, B = the bucket's merge sums added up; run += B; loc += run leaves
// run = U_j (the strip's sum) and loc = sum_s (s + 1) B_(j S + s + 1), so that sum_k k B_k = sum_j loc_j + S sum_j j U_j.
// (partial / toff / max_tasks: the merge sums, their offsets and their array's length per vector)
__global__ __launch_bounds__(64) void msm_var_strip_kernel(const XYZZ9* __restrict__ partial, const uint32_t* __restrict__ toff,
                                                           uint32_t max_tasks, uint32_t c, uint32_t nstrips, uint32_t S,
                                                           XYZZ9* __restrict__ strip_u, XYZZ9* __restrict__ strip_loc) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, v = blockIdx.y;
    if (j >= nstrips) return;
    const uint32_t nb = 1u << (c - 1);
    const uint32_t* to = toff + (size_t)v * (nb + 2);
    const XYZZ9* pp = partial + (size_t)v * max_tasks;
    XYZZ9 run = xyzz9_identity(), loc = xyzz9_identity();
    for (uint32_t s = S; s-- > 0;) {
        const uint32_t k = j * S + s + 1;
        if (k <= nb) {
            uint32_t t0 = to[k], t1 = to[k + 1];
            if (t1 > max_tasks) t1 = max_tasks;  // (never: the launch sizes the array for every merge task)
            for (uint32_t t = t0; t < t1; t++) run = xyzz9_add(run, ld_xyzz9(pp + t));
        }
        loc = xyzz9_add(loc, run);
    }
    st_xyzz9(strip_u + (size_t)v * nstrips + j, run);
    st_xyzz9(strip_loc + (size_t)v * nstrips + j, loc);
}

// Stage 2 (the scheme of msm_strip_sum_kernel), one workgroup per virtual vector: lane l folds `per` consecutive strips
// (C_l = their sum, w_l = sum_t t U_(l per + t), a_l = the sum of their loc), a suffix scan over the lanes gives
// sfx_l = sum_{l' >= l} C_l' (so sum_{l >= 1} sfx_l = sum_l l C_l), and
//     Y_l = S (per sfx_l + w_l) + a_l,   sum_l Y_l = sum_k k B_k
// with the powers of two S and per applied by doublings, per lane, before ONE tree.  The sum stays in the nine-limb form
// for the ladder.
__global__ __launch_bounds__(VAR_SUM_LANES) void msm_var_strip_sum_kernel(const XYZZ9* __restrict__ strip_u,
                                                                         const XYZZ9* __restrict__ strip_loc, uint32_t nstrips,
                                                                         uint32_t per, uint32_t S, XYZZ9* __restrict__ wsum) {
    __shared__ XYZZ9 sh[VAR_SUM_LANES];
    const uint32_t l = threadIdx.x, v = blockIdx.x;
    const XYZZ9* U = strip_u + (size_t)v * nstrips;
    const XYZZ9* L = strip_loc + (size_t)v * nstrips;
    XYZZ9 C = xyzz9_identity(), w = xyzz9_identity(), a = xyzz9_identity();
    for (uint32_t t = per; t-- > 0;) {
        const uint32_t jj = l * per + t;
        if (jj >= nstrips) continue;
        w = xyzz9_add(w, C);
        C = xyzz9_add(C, ld_xyzz9(U + jj));
        a = xyzz9_add(a, ld_xyzz9(L + jj));
    }
    sh[l] = C;
    __syncthreads();
    for (uint32_t o = 1; o < VAR_SUM_LANES; o <<= 1) {
        XYZZ9 x = xyzz9_identity();
        const bool has = l + o < VAR_SUM_LANES;
        if (has) x = sh[l + o];
        __syncthreads();
        if (has) sh[l] = xyzz9_add(sh[l], x);
        __syncthreads();
    }
    XYZZ9 X = l >= 1 ? sh[l] : xyzz9_identity();
    __syncthreads();
    for (uint32_t d = per; d > 1; d >>= 1) X = xyzz9_dbl(X);  // per * sfx_l
    X = xyzz9_add(X, w);
    for (uint32_t d = S; d > 1; d >>= 1) X = xyzz9_dbl(X);    // S * (...)
    sh[l] = xyzz9_add(X, a);
    __syncthreads();
    for (uint32_t o = VAR_SUM_LANES / 2; o > 0; o >>= 1) {
        if (l < o) sh[l] = xyzz9_add(sh[l], sh[l + o]);
        __syncthreads();
    }
    if (l == 0) st_xyzz9(wsum + v, sh[0]);
}

// One lane per vector: sum_w 2^(c w) S_w by Horner's rule, c doublings and one addition per window, (W - 1) c <= 254
// dependent doublings in all -- the chain a table of shifted points removes.  The vectors of a batch sit side by side in
// the lanes.  The result leaves in the library's packed XYZZ form, as msm_dev leaves it.
__global__ __launch_bounds__(64) void msm_var_horner_kernel(const XYZZ9* __restrict__ wsum, uint32_t windows, uint32_t c, uint32_t B,
                                                            XYZZ* __restrict__ out) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const XYZZ9* sw = wsum + (size_t)b * windows;
    XYZZ9 acc = ld_xyzz9(sw + windows - 1);
    for (uint32_t w = windows - 1; w-- > 0;) {
        for (uint32_t d = 0; d < c; d++) acc = xyzz9_dbl(acc);
        acc = xyzz9_add(acc, ld_xyzz9(sw + w));
    }
    const XYZZ r = xyzz9_to_xyzz(acc, false);
    var_st_fe(&out[b].x, r.x);
    var_st_fe(&out[b].y, r.y);
    var_st_fe(&out[b].zz, r.zz);
    var_st_fe(&out[b].zzz, r.zzz);
}

// The launch sequence.  d_out[b] (XYZZ, device memory) = sum_i scalars_b[i] * bases[i]; asynchronous on the context stream.
// Every buffer is a block of the context's workspace pool and goes back to it when the call returns (the stream orders
// the next user behind these kernels).
static int msm_var_launch(zg_ctx* ctx, const Affine* d_bases, const Fe* d_scalars, size_t stride, size_t batch, size_t n,
                          uint32_t c, XYZZ* d_out) {
    const uint32_t B = (uint32_t)batch, N = (uint32_t)n, W = msm_var_windows(c), nb = 1u << (c - 1);
    const uint32_t V = B * W;  // <= 256 * 128: inside a grid's second dimension
    const uint32_t K = VAR_K;
    // tasks of a virtual vector: sum_k ceil(cnt_k / K) <= n / K + (non-empty buckets) <= n / K + min(n, nb)
    const uint32_t max_tasks = N / K + (N < nb ? N : nb) + 1;
    // ... and its merge tasks: sum_k ceil(nt_k / K2) <= tasks / K2 + (non-empty buckets)
    const uint32_t max_tasks2 = max_tasks / VAR_K2 + (N < nb ? N : nb) + 1;
    // buckets per lane of msm_var_strip: as few as keep the strips of a vector within ONE pass of msm_var_strip_sum's 256 lanes
    // (per = 1; both stages are chains of dependent additions, 2 S + merges here and 3 per + ~20 there), at most VAR_STRIP
    uint32_t S = 1;
    while (S < VAR_STRIP && S * VAR_SUM_LANES < nb) S <<= 1;
    const uint32_t nstrips = (nb + S - 1) / S;
    uint32_t per = 1;
    while (per * VAR_SUM_LANES < nstrips) per <<= 1;
    WsScope ws(ctx);
    Affine* pts = ws.get<Affine>(n);
    uint32_t* dig = ws.get<uint32_t>((size_t)V * n);
    uint32_t* sorted = ws.get<uint32_t>((size_t)V * n);
    uint32_t* boff = ws.get<uint32_t>((size_t)V * (nb + 2));
    uint32_t* toff = ws.get<uint32_t>((size_t)V * (nb + 2));
    uint32_t* toff2 = ws.get<uint32_t>((size_t)V * (nb + 2));
    XYZZ9* partial = ws.get<XYZZ9>((size_t)V * max_tasks);
    XYZZ9* partial2 = ws.get<XYZZ9>((size_t)V * max_tasks2);
    XYZZ9* strip_u = ws.get<XYZZ9>((size_t)V * nstrips);
    XYZZ9* strip_loc = ws.get<XYZZ9>((size_t)V * nstrips);
    XYZZ9* wsum = ws.get<XYZZ9>(V);
    if (ws.failed) return ZG_ERR_OOM;
    const size_t sort_lds = (size_t)(nb + 2) * 4;
    if (sort_lds + 3 * 1024 * 4 > 64 * 1024) {  // dynamic LDS above 64 KB is an opt-in per function AND per device
        DeviceState& ds = device_state(ctx->device);
        std::lock_guard<std::mutex> lock(ds.mu);
        if (!ds.msm_var_attrs) {
            ZG_HIP(hipFuncSetAttribute((const void*)msm_var_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
            ds.msm_var_attrs = true;
        }
    }
    const double ent = (double)V * (double)N;
    const double msm_bytes = (double)B * ((double)N * 96.0 + 96.0);  // the unit: one MSM, charged once
    ZG_LAUNCH(ctx, "msm_var_points", (double)N * 128.0, msm_var_points_kernel, dim3((N + 255) / 256), dim3(256), 0, d_bases, pts, N);
    ZG_LAUNCH(ctx, "msm_var_digits", (double)B * N * 32.0 + ent * 4.0, msm_var_digits_kernel, dim3((N + 255) / 256, B), dim3(256), 0,
              d_scalars, stride, N, c, W, dig);
    ZG_LAUNCH(ctx, "msm_var_sort", ent * 8.0 + (double)V * (nb + 2.0) * 12.0, msm_var_sort_kernel, dim3(V), dim3(1024), sort_lds, dig, N,
              c, K, boff, toff, toff2, sorted);
    ZG_LAUNCH_U(ctx, "msm_var_accumulate", msm_bytes, msm_bytes, msm_var_accumulate_kernel, dim3((max_tasks + 255) / 256, V), dim3(256),
                0, pts, c, boff, toff, sorted, N, max_tasks, partial);
    const double part_bytes = (double)V * (double)(nb < max_tasks ? nb : max_tasks) * sizeof(XYZZ9);  // >= one sum per bucket
    ZG_LAUNCH(ctx, "msm_var_merge", 2.0 * part_bytes, msm_var_merge_kernel, dim3((max_tasks2 + 255) / 256, V), dim3(256), 0, partial, toff,
              toff2, c, max_tasks, max_tasks2, partial2);
    ZG_LAUNCH(ctx, "msm_var_strip", part_bytes + (double)V * 2.0 * nstrips * sizeof(XYZZ9), msm_var_strip_kernel,
              dim3((nstrips + 63) / 64, V), dim3(64), 0, partial2, toff2, max_tasks2, c, nstrips, S, strip_u, strip_loc);
    ZG_LAUNCH(ctx, "msm_var_strip_sum", (double)V * (2.0 * nstrips + 1.0) * sizeof(XYZZ9), msm_var_strip_sum_kernel, dim3(V),
              dim3(VAR_SUM_LANES), 0, strip_u, strip_loc, nstrips, per, S, wsum);
    ZG_LAUNCH(ctx, "msm_var_horner", (double)V * sizeof(XYZZ9) + (double)B * sizeof(XYZZ), msm_var_horner_kernel, dim3((B + 63) / 64),
              dim3(64), 0, wsum, W, c, B, d_out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// What all three entries ask of their sizes, before anything is read or allocated.
static int msm_var_check(const char* who, size_t batch, size_t n, uint32_t window_bits) {
    ZG_REQUIRE(window_bits == 0 || (window_bits >= 2 && window_bits <= 16), ZG_ERR_INVALID_ARG, "%s: window_bits %u not 0 or in [2,16]",
               who, window_bits);
    ZG_REQUIRE(n < ((size_t)1 << 23), ZG_ERR_UNSUPPORTED, "%s: n=%zu, at most 2^23 - 1 points", who, n);
    ZG_REQUIRE(batch <= VAR_MAX_BATCH, ZG_ERR_UNSUPPORTED, "%s: batch of %zu vectors, at most %zu", who, batch, VAR_MAX_BATCH);
    return ZG_OK;
}

static int msm_var_dev(zg_ctx* ctx, const Affine* d_bases, const Fe* d_scalars, size_t stride, size_t batch, size_t n,
                       uint32_t window_bits, XYZZ* d_out) {
    if (batch == 0) return ZG_OK;
    if (n == 0) {  // no launch: the identity, copied
        std::vector<XYZZ> ids(batch, xyzz_identity());
        ZG_HIP(hipMemcpyAsync(d_out, ids.data(), batch * sizeof(XYZZ), hipMemcpyDefault, ctx->stream));
        ZG_HIP(hipStreamSynchronize(ctx->stream));
        return ZG_OK;
    }
    const uint32_t c = window_bits ? window_bits : msm_var_default_bits(n, batch);
    return msm_var_launch(ctx, d_bases, d_scalars, stride, batch, n, c, d_out);
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_msm_var_dev(zg_ctx* ctx, const void* d_bases, const void* d_scalars, size_t stride_elems, size_t batch, size_t n,
                   uint32_t window_bits, void* d_out_xyzz) {
    ZG_REQUIRE(ctx != nullptr, ZG_ERR_INVALID_ARG, "zg_msm_var_dev: ctx is null");
    ZG_TRY(msm_var_check("zg_msm_var_dev", batch, n, window_bits));
    ZG_REQUIRE(batch == 0 || d_out_xyzz, ZG_ERR_INVALID_ARG, "zg_msm_var_dev: d_out_xyzz is null");
    ZG_REQUIRE(batch == 0 || n == 0 || (d_bases && d_scalars), ZG_ERR_INVALID_ARG, "zg_msm_var_dev: null argument");
    ZG_REQUIRE(batch <= 1 || n == 0 || stride_elems >= n, ZG_ERR_INVALID_ARG, "zg_msm_var_dev: stride %zu below n = %zu", stride_elems, n);
    ZG_ENTER(ctx);
    return msm_var_dev(ctx, (const Affine*)d_bases, (const Fe*)d_scalars, stride_elems, batch, n, window_bits, (XYZZ*)d_out_xyzz);
}

int zg_msm_var_batch(zg_ctx* ctx, const zg_g1_affine* bases, const zg_fr* const* scalars, size_t batch, size_t n,
                     uint32_t window_bits, zg_g1* out) {
    ZG_REQUIRE(ctx != nullptr, ZG_ERR_INVALID_ARG, "zg_msm_var_batch: ctx is null");
    ZG_TRY(msm_var_check("zg_msm_var_batch", batch, n, window_bits));
    ZG_REQUIRE(batch == 0 || out, ZG_ERR_INVALID_ARG, "zg_msm_var_batch: out is null");
    ZG_REQUIRE(batch == 0 || n == 0 || (bases && scalars), ZG_ERR_INVALID_ARG, "zg_msm_var_batch: null argument");
    if (batch == 0) return ZG_OK;
    if (n == 0) {  // nothing to launch
        const XYZZ id = xyzz_identity();
        for (size_t b = 0; b < batch; b++) xyzz_batch_normalise(&id, 1, out + b);
        return ZG_OK;
    }
    for (size_t b = 0; b < batch; b++)
        ZG_REQUIRE(scalars[b] != nullptr, ZG_ERR_INVALID_ARG, "zg_msm_var_batch: scalars[%zu] is null", b);
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    Affine* d_bases = ws.get<Affine>(n);
    Fe* d = ws.get<Fe>(batch * n);
    XYZZ* r = ws.get<XYZZ>(batch);
    if (ws.failed) return ZG_ERR_OOM;
    ZG_HIP(hipMemcpyAsync(d_bases, bases, n * sizeof(Affine), hipMemcpyHostToDevice, ctx->stream));
    for (size_t b = 0; b < batch; b++) ZG_HIP(hipMemcpyAsync(d + b * n, scalars[b], n * 32, hipMemcpyHostToDevice, ctx->stream));
    ZG_TRY(msm_var_dev(ctx, d_bases, d, n, batch, n, window_bits, r));
    return zg_msm_finish(ctx, r, batch, out);
}

int zg_msm_var(zg_ctx* ctx, const zg_g1_affine* bases, const zg_fr* scalars, size_t n, uint32_t window_bits, zg_g1* out) {
    const zg_fr* arr[1] = {scalars};
    ZG_REQUIRE(n == 0 || scalars, ZG_ERR_INVALID_ARG, "zg_msm_var: scalars is null");
    return zg_msm_var_batch(ctx, bases, arr, 1, n, window_bits, out);
}

}  // extern "C"
