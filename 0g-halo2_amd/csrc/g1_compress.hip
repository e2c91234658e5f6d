// Point compression for halo2's own proof format (zg_g1_compress, zg_g1_decompress, zg_g1_decompress_dev; DESIGN.md
// section 17): GroupEncoding::to_bytes on the host, GroupEncoding::from_bytes for n encodings on the GPU.
//
// Decompression gets y back from x: y = (x^3 + 3)^((q+1)/4), one chain of 251 squarings and the multiplications of the
// exponent's set bits per point.  One lane per point, in a kernel of its own -- as g1_mul.hip does -- so that a batch
// verification (verify.hip) pays the ~30 roots of a proof on 30 lanes, not one after another in its one-wave-per-proof
// replay.  The exponent is a constant: every lane of a wave walks the same products, and data decides nothing before the
// final selects (g1_compress.h).  An invalid encoding gives (0,0) with flag 0 in ITS slot and disturbs no neighbour.
//
// The chain is a fixed 4-bit window (14 products for the lane's table t^2 .. t^15 in LDS, then 4 squarings and one
// multiplication per non-zero digit: 318 products); g1_compress.h's plain square-and-multiply (359), which the host uses, was
// 5 - 13 % slower in this kernel's place.  The output is canonical, so the bytes are the same.
#include "common.h"
#include "g1_compress.h"

namespace zg {

namespace {

constexpr uint32_t G1C_WG = 64;                  // points per workgroup = one wave
constexpr uint32_t G1C_ENTRY_WORDS = 8 * G1C_WG;  // one Fe per lane
constexpr uint32_t G1C_ENTRIES = 15;             // t^1 .. t^15

__device__ __forceinline__ void g1c_store(uint32_t* tab, uint32_t entry, uint32_t lane, const Fe& v) {
    uint32_t* p = tab + entry * G1C_ENTRY_WORDS + lane;
#pragma unroll
    for (int j = 0; j < 8; j++) p[j * G1C_WG] = v.l[j];
}
__device__ __forceinline__ Fe g1c_load(const uint32_t* tab, uint32_t entry, uint32_t lane) {
    const uint32_t* p = tab + entry * G1C_ENTRY_WORDS + lane;
    Fe v;
#pragma unroll
    for (int j = 0; j < 8; j++) v.l[j] = p[j * G1C_WG];
    return v;
}

// t^((q+1)/4) with a fixed 4-bit window over the constant exponent: the digit is the same for every lane (a scalar), the
// lane's own powers live in LDS, [entry][word][lane] -- nothing in private memory is indexed by a run-time value
__device__ Fe fq_sqrt_candidate_window(const Fe& t, uint32_t* tab, uint32_t lane) {
    constexpr uint32_t E[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    Fe pw = t;
    g1c_store(tab, 0, lane, pw);
#pragma unroll 1
    for (uint32_t j = 2; j <= G1C_ENTRIES; j++) {
        pw = Fq::mul(pw, t);
        g1c_store(tab, j - 1, lane, pw);
    }
    // (a lane reads only what it wrote itself: no barrier)
    Fe res = g1c_load(tab, 0xc - 1, lane);  // the top digit, bits 248 .. 251
#pragma unroll 1
    for (int w = 61; w >= 0; w--) {
        res = Fq::sqr(Fq::sqr(Fq::sqr(Fq::sqr(res))));
        const uint32_t d = (E[w >> 3] >> (4 * (w & 7))) & 15u;
        if (d) res = Fq::mul(res, g1c_load(tab, d - 1, lane));  // (d comes from the constant: the branch is the wave's)
    }
    return res;
}

__global__ __launch_bounds__(G1C_WG) void g1_decompress_kernel(const uint8_t* __restrict__ in, Affine* __restrict__ out,
                                                               uint8_t* __restrict__ valid, uint32_t n) {
    __shared__ uint32_t tab[G1C_ENTRIES * G1C_ENTRY_WORDS];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x * G1C_WG + lane;
    const bool live = i < n;
    // a lane past the end decodes the identity: it runs the wave's steps and stores nothing
    uint8_t b[32];
#pragma unroll
    for (int k = 0; k < 32; k++) b[k] = 0;
    if (live) {
        const uint8_t* src = in + (size_t)i * 32;
#pragma unroll
        for (int k = 0; k < 32; k++) b[k] = src[k];
    }
    // g1_decompress_one with the windowed chain in the root's place
    Fe x;
#pragma unroll
    for (int k = 0; k < 8; k++)
        x.l[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    const uint32_t sign = x.l[7] >> 31;
    x.l[7] &= 0x7fffffffu;
    uint32_t pm[8], tmp[8];
#pragma unroll
    for (int k = 0; k < 8; k++) pm[k] = FqParams::p(k);
    const bool canonical = sub8(tmp, x.l, pm) != 0;
    x = g1c_select(canonical, x, fe_zero());
    const bool identity = canonical && fe_is_zero(x) && sign == 0;
    const Fe xm = Fq::from_raw(x);
    const Fe three = Fq::add(Fq::add(Fq::one(), Fq::one()), Fq::one());
    const Fe t = Fq::add(Fq::mul(Fq::sqr(xm), xm), three);
    Fe y = fq_sqrt_candidate_window(t, tab, lane);
    const bool is_root = fe_eq(Fq::sqr(y), t);
    const Fe y_raw = Fq::to_raw(y);
    y = g1c_select((y_raw.l[0] & 1u) != sign, Fq::neg(y), y);
    const bool point = canonical && is_root;
    Affine p;
    p.x = g1c_select(point, xm, fe_zero());
    p.y = g1c_select(point, y, fe_zero());
    const bool ok = point || identity;
    if (live) {
        out[i] = p;
        valid[i] = ok ? 1 : 0;
    }
}

}  // namespace

// d_in: n encodings of 32 bytes; d_out: n affine points; d_valid: n flags; asynchronous.  d_out may not alias d_in.
int g1_decompress_dev(zg_ctx* ctx, const uint8_t* d_in, size_t n, Affine* d_out, uint8_t* d_valid) {
    if (n == 0) return ZG_OK;
    const uint32_t grid = (uint32_t)((n + G1C_WG - 1) / G1C_WG);
    ZG_LAUNCH(ctx, "g1_decompress", (double)n * 97, g1_decompress_kernel, dim3(grid), dim3(G1C_WG), 0, d_in, d_out, d_valid, (uint32_t)n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" int zg_g1_compress(const zg_g1_affine* points, size_t n, zg_g1_compressed* out) {
    if (n == 0) return ZG_OK;
    ZG_REQUIRE(points && out, ZG_ERR_INVALID_ARG, "zg_g1_compress: null argument");
    for (size_t i = 0; i < n; i++) {
        Affine p;
        std::memcpy(&p, &points[i], sizeof(p));
        g1_compress_one(p, out[i].b);
    }
    return ZG_OK;
}

extern "C" int zg_g1_decompress_dev(zg_ctx* ctx, const void* d_in, size_t n, void* d_out, void* d_valid) {
    ZG_REQUIRE(ctx, ZG_ERR_INVALID_ARG, "zg_g1_decompress_dev: null context");
    if (n == 0) return ZG_OK;
    ZG_REQUIRE(d_in && d_out && d_valid, ZG_ERR_INVALID_ARG, "zg_g1_decompress_dev: null argument");
    ZG_REQUIRE(n < ((size_t)1 << 28), ZG_ERR_UNSUPPORTED, "zg_g1_decompress_dev: n=%zu >= 2^28", n);
    ZG_ENTER(ctx);
    return g1_decompress_dev(ctx, (const uint8_t*)d_in, n, (Affine*)d_out, (uint8_t*)d_valid);
}

extern "C" int zg_g1_decompress(zg_ctx* ctx, const zg_g1_compressed* in, size_t n, zg_g1_affine* out, uint8_t* valid) {
    ZG_REQUIRE(ctx, ZG_ERR_INVALID_ARG, "zg_g1_decompress: null context");
    if (n == 0) return ZG_OK;
    ZG_REQUIRE(in && out && valid, ZG_ERR_INVALID_ARG, "zg_g1_decompress: null argument");
    ZG_REQUIRE(n < ((size_t)1 << 28), ZG_ERR_UNSUPPORTED, "zg_g1_decompress: n=%zu >= 2^28", n);
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    uint8_t* di = ws.get<uint8_t>(n * 32);
    Affine* dp = ws.get<Affine>(n);
    uint8_t* dv = ws.get<uint8_t>(n);
    if (ws.failed) return ZG_ERR_OOM;
    hipStream_t st = ctx->stream;
    ZG_HIP(hipMemcpyAsync(di, in, n * 32, hipMemcpyHostToDevice, st));
    ZG_TRY(g1_decompress_dev(ctx, di, n, dp, dv));
    ZG_HIP(hipMemcpyAsync(out, dp, n * sizeof(Affine), hipMemcpyDeviceToHost, st));
    ZG_HIP(hipMemcpyAsync(valid, dv, n, hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    return ZG_OK;
}
