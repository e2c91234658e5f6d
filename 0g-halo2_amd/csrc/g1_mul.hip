// n independent variable-base multiplications out[i] = scalars[i] * points[i] on the GPU (zg_g1_mul_each): the step an
// SRS contribution is made of (srs_update.hip), g'[i] = t^i g[i].
//
// One lane per point, one wave per workgroup.  A scalar is walked from the top in signed windows of W = G1_MUL_W bits
// (g1_mul_digits.h: biased, so digit w needs no carry from below), against the lane's own multiples P, 2P, .. 2^(W-1) P:
//   * every lane of a wave runs the SAME W doublings and one addition per window, whatever its digits are (the binary
//     ladder of xyzz_mul_raw pays its mixed addition on almost every bit once 64 lanes share the branch);
//   * P stays in registers; the multiples from 2P on live in LDS, [entry][word][lane]: a lane reads the entry its digit
//     names at a stride that keeps the 64 lanes on distinct banks, and nothing in private memory is indexed by a
//     run-time value (no scratch).  What the table takes of LDS decides how many waves a CU holds, and that -- not the
//     number of field products -- decides the time (W = 2, 8 KB per wave);
//   * the digit's sign negates y by select, a zero digit keeps the accumulator by select;
//   * the wave shares ONE inversion for the conversion to affine: a product tree over the 64 values ZZ * ZZZ in LDS, its
//     root inverted by lane 0, the inverses handed back down the tree.  A lane whose result is the identity enters as 1.
// The rare cases of an addition (an identity operand, equal or opposite points: the first non-zero window, scalars
// within 2^(W-1) of a multiple of r) are the branches of xyzz_add; a wave that meets one pays for it, nothing else does.
#include "common.h"
#include "g1_mul_digits.h"

namespace zg {

namespace {

constexpr uint32_t G1MUL_WG = 64;  // points per workgroup = one wave
using Digits = G1MulDigits<G1_MUL_W>;
constexpr uint32_t G1MUL_ENTRIES = 1u << (G1_MUL_W - 1);  // multiples a digit can name: 1 .. 2^(W-1)
constexpr uint32_t G1MUL_ENTRY_WORDS = 32 * G1MUL_WG;  // one XYZZ per lane
static_assert((G1MUL_ENTRIES - 1) * G1MUL_ENTRY_WORDS * 4 >= 2 * 2 * G1MUL_WG * sizeof(Fe), "the inversion tree reuses the table");

__device__ __forceinline__ void tab_store(uint32_t* tab, uint32_t entry, uint32_t lane, const XYZZ& v) {
    uint32_t* p = tab + entry * G1MUL_ENTRY_WORDS + lane;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        p[(0 + j) * G1MUL_WG] = v.x.l[j];
        p[(8 + j) * G1MUL_WG] = v.y.l[j];
        p[(16 + j) * G1MUL_WG] = v.zz.l[j];
        p[(24 + j) * G1MUL_WG] = v.zzz.l[j];
    }
}

__device__ __forceinline__ XYZZ tab_load(const uint32_t* tab, uint32_t entry, uint32_t lane) {
    const uint32_t* p = tab + entry * G1MUL_ENTRY_WORDS + lane;
    XYZZ v;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        v.x.l[j] = p[(0 + j) * G1MUL_WG];
        v.y.l[j] = p[(8 + j) * G1MUL_WG];
        v.zz.l[j] = p[(16 + j) * G1MUL_WG];
        v.zzz.l[j] = p[(24 + j) * G1MUL_WG];
    }
    return v;
}

__device__ __forceinline__ Fe fe_select(bool c, const Fe& a, const Fe& b) {
    Fe o;
#pragma unroll
    for (int j = 0; j < 8; j++) o.l[j] = c ? a.l[j] : b.l[j];
    return o;
}

__global__ __launch_bounds__(G1MUL_WG) void g1_mul_each_kernel(const Affine* points, const Fe* __restrict__ scalars,
                                                               Affine* out, uint32_t n) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[(G1MUL_ENTRIES - 1) * G1MUL_ENTRY_WORDS];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x * G1MUL_WG + lane;
    const bool live = i < n;
    // a lane past the end multiplies the identity by zero: it runs the wave's steps and enters the shared inversion as 1
    Affine p;
    p.x = fe_zero();
    p.y = fe_zero();
    Fe s = fe_zero();
    if (live) {
        p = points[i];
        s = scalars[i];
    }
    const Fe raw = Fr::to_raw(s);

    const XYZZ first = xyzz_from_affine(p);
    {  // entry j - 2 = j P, j = 2 .. 2^(W-1)
        XYZZ e = xyzz_dbl_affine(p);
        tab_store(tab, 0, lane, e);
#pragma unroll 1
        for (uint32_t j = 3; j <= G1MUL_ENTRIES; j++) {
            e = xyzz_madd(e, p);
            tab_store(tab, j - 2, lane, e);
        }
    }
    // (a lane reads only what it wrote itself: no barrier between the table and the walk)
    Digits d;
    d.init(raw.l);
    XYZZ acc = xyzz_identity();
    if (d.top()) acc = first;
#pragma unroll 1
    for (uint32_t w = 0; w < Digits::WINDOWS; w++) {
#pragma unroll 1
        for (uint32_t b = 0; b < G1_MUL_W; b++) acc = xyzz_dbl(acc);
        const int dg = d.next();
        const bool neg = dg < 0;
        const uint32_t mag = (uint32_t)(neg ? -dg : dg);
        XYZZ q = tab_load(tab, mag >= 2 ? mag - 2 : 0, lane);
        const bool one = mag < 2;
        q.x = fe_select(one, first.x, q.x);
        q.y = fe_select(one, first.y, q.y);
        q.zz = fe_select(one, first.zz, q.zz);
        q.zzz = fe_select(one, first.zzz, q.zzz);
        q.y = fe_select(neg, Fq::neg(q.y), q.y);
        const XYZZ sum = xyzz_add(acc, q);
        const bool take = mag != 0;
        acc.x = fe_select(take, sum.x, acc.x);
        acc.y = fe_select(take, sum.y, acc.y);
        acc.zz = fe_select(take, sum.zz, acc.zz);
        acc.zzz = fe_select(take, sum.zzz, acc.zzz);
    }

    // one inversion for the wave: nodes 1..127 of a heap, leaves 64..127
    Fe* prod = reinterpret_cast<Fe*>(tab);
    Fe* inv = prod + 2 * G1MUL_WG;
    Fe v = Fq::mul(acc.zz, acc.zzz);
    const bool ident = fe_is_zero(v);
    if (ident) v = Fq::one();
    __syncthreads();  // every lane is done with its table
    prod[G1MUL_WG + lane] = v;
    __syncthreads();
    for (uint32_t half = G1MUL_WG / 2; half >= 1; half >>= 1) {
        if (lane < half) {
            const uint32_t node = half + lane;
            prod[node] = Fq::mul(prod[2 * node], prod[2 * node + 1]);
        }
        __syncthreads();
    }
    if (lane == 0) inv[1] = Fq::inv(prod[1]);
    __syncthreads();
    for (uint32_t half = 1; half < G1MUL_WG; half <<= 1) {
        if (lane < half) {
            const uint32_t node = half + lane;
            const Fe up = inv[node];
            inv[2 * node] = Fq::mul(up, prod[2 * node + 1]);
            inv[2 * node + 1] = Fq::mul(up, prod[2 * node]);
        }
        __syncthreads();
    }
    const Fe iv = inv[G1MUL_WG + lane];  // 1 / (ZZ * ZZZ)
    Affine o;
    o.x = Fq::mul(acc.x, Fq::mul(iv, acc.zzz));
    o.y = Fq::mul(acc.y, Fq::mul(iv, acc.zz));
    if (ident) {
        o.x = fe_zero();
        o.y = fe_zero();
    }
    if (live) out[i] = o;
}

}  // namespace

// d_points, d_out: n affine points (they may be the same array); d_scalars: n Montgomery scalars; asynchronous
int g1_mul_each_dev(zg_ctx* ctx, const Affine* d_points, const Fe* d_scalars, size_t n, Affine* d_out) {
    if (n == 0) return ZG_OK;
    const uint32_t grid = (uint32_t)((n + G1MUL_WG - 1) / G1MUL_WG);
    ZG_LAUNCH(ctx, "g1_mul_each", (double)n * 160, g1_mul_each_kernel, dim3(grid), dim3(G1MUL_WG), 0, d_points, d_scalars,
              d_out, (uint32_t)n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" int zg_g1_mul_each_dev(zg_ctx* ctx, const void* d_points, const void* d_scalars, size_t n, void* d_out) {
    ZG_REQUIRE(ctx, ZG_ERR_INVALID_ARG, "zg_g1_mul_each_dev: null context");
    if (n == 0) return ZG_OK;
    ZG_REQUIRE(d_points && d_scalars && d_out, ZG_ERR_INVALID_ARG, "zg_g1_mul_each_dev: null argument");
    ZG_REQUIRE(n < ((size_t)1 << 28), ZG_ERR_UNSUPPORTED, "zg_g1_mul_each_dev: n=%zu >= 2^28", n);
    ZG_ENTER(ctx);
    return g1_mul_each_dev(ctx, (const Affine*)d_points, (const Fe*)d_scalars, n, (Affine*)d_out);
}

extern "C" int zg_g1_mul_each(zg_ctx* ctx, const zg_g1_affine* points, const zg_fr* scalars, size_t n, zg_g1_affine* out) {
    ZG_REQUIRE(ctx, ZG_ERR_INVALID_ARG, "zg_g1_mul_each: null context");
    if (n == 0) return ZG_OK;
    ZG_REQUIRE(points && scalars && out, ZG_ERR_INVALID_ARG, "zg_g1_mul_each: null argument");
    ZG_REQUIRE(n < ((size_t)1 << 28), ZG_ERR_UNSUPPORTED, "zg_g1_mul_each: n=%zu >= 2^28", n);
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    Affine* dp = ws.get<Affine>(n);
    Fe* ds = ws.get<Fe>(n);
    if (ws.failed) return ZG_ERR_OOM;
    hipStream_t st = ctx->stream;
    ZG_HIP(hipMemcpyAsync(dp, points, n * sizeof(Affine), hipMemcpyHostToDevice, st));
    ZG_HIP(hipMemcpyAsync(ds, scalars, n * sizeof(Fe), hipMemcpyHostToDevice, st));
    ZG_TRY(g1_mul_each_dev(ctx, dp, ds, n, dp));
    ZG_HIP(hipMemcpyAsync(out, dp, n * sizeof(Affine), hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    // the scalars of a contribution are powers of its secret: they do not stay in a pooled block (best effort, as in
    // zg_params_update)
    ZG_HIP(hipMemsetAsync(ds, 0, n * sizeof(Fe), st));
    ZG_HIP(hipStreamSynchronize(st));
    return ZG_OK;
}
