// The G1 inverse FFT -- replaces halo2_proofs::poly::kzg::commitment::g_to_lagrange (halo2_proofs v2023_04_20
// src/poly/kzg/commitment.rs), as ParamsKZG::downsize and every import of an SRS that arrives as `g` alone use it:
//   g_lagrange[i] = 2^-k * sum_j omega^(-ij) g[j]          (best_fft over G1 with omega_inv, then the scaling)
// No scalar is involved: the Lagrange basis of 2^k points is derived from the first 2^k powers-of-tau points.
//
// Layout of the work (all in context workspace, 128-byte XYZZ points):
//   g1fft_twiddles  one table per call: omega_inv^j, j < n/2, as CANONICAL integers (8 x u32) -- what a scalar
//                   multiplication walks bit by bit; a pass reads entry j * (n / 2m);
//   g1fft_load      g[i] * 2^-k -> slot bitrev(i).  The scaling happens here because here the base is still affine
//                   (xyzz_mul_raw: a mixed addition per set bit), and the transform is linear;
//   g1fft_pass      k radix-2 decimation-in-time passes, one lane per butterfly: t = w b, (a, b) <- (a + t, a - t).
//                   w b is a 254-step double-and-add over an XYZZ base (xyzz_mul_raw_xyzz: a FULL addition per set bit,
//                   the points between passes are never re-normalised); the conditional addition runs under the lane's
//                   mask, the doublings are uniform.  Lanes with w = 1 (every lane of the first pass, half of the
//                   second's, ...) do not multiply at all.  a + t and a - t go through xyzz_add, which decides a = t
//                   (doubling), a = -t (identity) and an identity operand by itself;
//   g1fft_store     XYZZ -> affine, one inversion per lane as srs_kernel does; identity -> (0, 0).
// A butterfly is about one scalar multiplication (~4 000 field products); a pass is n/2 of them side by side and the
// passes are dependent, so the transform takes about (k + 2) scalar-multiplication latencies whatever k <= 17 is: a
// one-off per SRS, outside every timed region.
#include "common.h"

namespace zg {
namespace {

constexpr uint32_t G1FFT_WG = 64;  // one wave per workgroup: a pass of n/2 butterflies spreads over n/128 CUs' worth of waves

__device__ __forceinline__ XYZZ ld_xyzz_g(const XYZZ* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    XYZZ v;
    uint4* d = reinterpret_cast<uint4*>(&v);
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = q[i];
    return v;
}
__device__ __forceinline__ void st_xyzz_g(XYZZ* p, const XYZZ& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    const uint4* s = reinterpret_cast<const uint4*>(&v);
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = s[i];
}
__device__ __forceinline__ Affine ld_affine_g(const Affine* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    Affine v;
    uint4* d = reinterpret_cast<uint4*>(&v);
#pragma unroll
    for (int i = 0; i < 4; i++) d[i] = q[i];
    return v;
}
__device__ __forceinline__ void st_affine_g(Affine* p, const Affine& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    const uint4* s = reinterpret_cast<const uint4*>(&v);
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = s[i];
}

// tw[j] = omega_inv^j as a canonical integer, j < half
__global__ __launch_bounds__(G1FFT_WG) void g1fft_twiddles(Fe* __restrict__ tw, Fe omega_inv, uint32_t half) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= half) return;
    const Fe raw = Fr::to_raw(Fr::pow_u64(omega_inv, j));
    uint4* q = reinterpret_cast<uint4*>(tw + j);
    q[0] = make_uint4(raw.l[0], raw.l[1], raw.l[2], raw.l[3]);
    q[1] = make_uint4(raw.l[4], raw.l[5], raw.l[6], raw.l[7]);
}

// buf[bitrev(i)] = scale * g[i]  (scale = 2^-k as a canonical integer; k = 0: no multiplication)
__global__ __launch_bounds__(G1FFT_WG) void g1fft_load(const Affine* __restrict__ g, XYZZ* __restrict__ buf, Fe scale,
                                                       uint32_t n, uint32_t log_n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine p = ld_affine_g(g + i);
    const uint32_t r = log_n ? __brev(i) >> (32 - log_n) : 0;
    st_xyzz_g(buf + r, log_n ? xyzz_mul_raw(p, scale.l) : xyzz_from_affine(p));
}

// pass with butterflies of span m = 2^log_m: lane t < n/2 owns the pair (blk * 2m + j, ... + m), j = t mod m
__global__ __launch_bounds__(G1FFT_WG) void g1fft_pass(XYZZ* __restrict__ buf, const Fe* __restrict__ tw, uint32_t half,
                                                       uint32_t log_m, uint32_t tw_shift) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= half) return;
    const uint32_t j = t & ((1u << log_m) - 1);
    const size_t ia = ((size_t)(t >> log_m) << (log_m + 1)) + j, ib = ia + ((size_t)1 << log_m);
    XYZZ b = ld_xyzz_g(buf + ib);
    if (j != 0) {  // w = omega_inv^(j * n / 2m); j = 0: w = 1
        const uint4* q = reinterpret_cast<const uint4*>(tw + ((size_t)j << tw_shift));
        const uint4 lo = q[0], hi = q[1];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        b = xyzz_mul_raw_xyzz(b, w);
    }
    const XYZZ a = ld_xyzz_g(buf + ia);
    st_xyzz_g(buf + ia, xyzz_add(a, b));
    st_xyzz_g(buf + ib, xyzz_add(a, xyzz_neg(b)));
}

__global__ __launch_bounds__(G1FFT_WG) void g1fft_store(const XYZZ* __restrict__ buf, Affine* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st_affine_g(out + i, xyzz_to_affine(ld_xyzz_g(buf + i)));
}

}  // namespace

// d_g: 2^k affine points, d_gl: 2^k affine points out; asynchronous on the context stream
int g1_lagrange_dev(zg_ctx* ctx, uint32_t k, const Affine* d_g, Affine* d_gl) {
    const uint32_t n = 1u << k, half = n >> 1;
    WsScope ws(ctx);
    XYZZ* buf = ws.get<XYZZ>(n);
    Fe* tw = ws.get<Fe>(half ? half : 1);
    if (ws.failed) return ZG_ERR_OOM;
    const Fe omega_inv = Fr::inv(host_domain_omega(k));
    const Fe scale = Fr::to_raw(Fr::inv(Fr::from_u64(n)));
    const dim3 wg(G1FFT_WG), grid_n((n + G1FFT_WG - 1) / G1FFT_WG), grid_h((half + G1FFT_WG - 1) / G1FFT_WG);
    if (half) ZG_LAUNCH(ctx, "g1fft_twiddles", (double)half * 32, g1fft_twiddles, grid_h, wg, 0, tw, omega_inv, half);
    ZG_LAUNCH(ctx, "g1fft_load", (double)n * 192, g1fft_load, grid_n, wg, 0, d_g, buf, scale, n, k);
    for (uint32_t log_m = 0; log_m < k; log_m++)
        ZG_LAUNCH(ctx, "g1fft_pass", (double)n * 256, g1fft_pass, grid_h, wg, 0, buf, tw, half, log_m, k - 1 - log_m);
    ZG_LAUNCH(ctx, "g1fft_store", (double)n * 192, g1fft_store, grid_n, wg, 0, buf, d_gl, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" int zg_params_lagrange_dev(zg_ctx* ctx, uint32_t k, const void* d_g, void* d_g_lagrange) {
    ZG_REQUIRE(ctx && d_g && d_g_lagrange, ZG_ERR_INVALID_ARG, "zg_params_lagrange_dev: null argument");
    ZG_REQUIRE(d_g != d_g_lagrange, ZG_ERR_INVALID_ARG, "zg_params_lagrange_dev: the output may not be the input");
    ZG_REQUIRE(k <= 24, ZG_ERR_UNSUPPORTED, "zg_params_lagrange_dev: k=%u > 24", k);
    ZG_ENTER(ctx);
    return g1_lagrange_dev(ctx, k, (const Affine*)d_g, (Affine*)d_g_lagrange);
}

extern "C" int zg_params_lagrange(zg_ctx* ctx, uint32_t k, const zg_g1_affine* g, zg_g1_affine* g_lagrange) {
    ZG_REQUIRE(ctx && g && g_lagrange, ZG_ERR_INVALID_ARG, "zg_params_lagrange: null argument");
    ZG_REQUIRE(k <= 24, ZG_ERR_UNSUPPORTED, "zg_params_lagrange: k=%u > 24", k);
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    const size_t n = (size_t)1 << k;
    Affine* dg = ws.get<Affine>(n);
    Affine* dl = ws.get<Affine>(n);
    if (ws.failed) return ZG_ERR_OOM;
    ZG_HIP(hipMemcpyAsync(dg, g, n * sizeof(Affine), hipMemcpyHostToDevice, ctx->stream));
    ZG_TRY(g1_lagrange_dev(ctx, k, dg, dl));
    ZG_HIP(hipMemcpyAsync(g_lagrange, dl, n * sizeof(Affine), hipMemcpyDeviceToHost, ctx->stream));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    return ZG_OK;
}
