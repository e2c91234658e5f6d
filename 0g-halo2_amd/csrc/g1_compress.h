// The 32-byte GroupEncoding of a BN254 G1 point as halo2curves 0.3.3 writes it (G1Affine::to_bytes / from_bytes):
// x.to_repr() -- 32 little-endian bytes of the canonical integer -- with the low bit of y in bit 7 of byte 31; bit 6 is
// always 0 (q < 2^254); the identity is 32 zero bytes.  One body for the host (zg_g1_compress, the transcript writer, the
// host test program) and for the device (g1_decompress_kernel in g1_compress.hip: one lane per point).
//
// Written from the published sources, not compiled against the crate.
#pragma once

#include "curve.h"

namespace zg {

__host__ __device__ inline void fe_to_le_bytes_raw(const Fe& r, uint8_t out[32]) {
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(r.l[i] >> (8 * j));
}

// the encoding of an affine point in Montgomery form ((0,0): the identity, 32 zero bytes); no validation
__host__ __device__ inline void g1_compress_one(const Affine& p, uint8_t out[32]) {
    const Fe x = Fq::to_raw(p.x), y = Fq::to_raw(p.y);
    fe_to_le_bytes_raw(x, out);
    out[31] |= (uint8_t)((y.l[0] & 1u) << 7);
}

__host__ __device__ __forceinline__ Fe g1c_select(bool c, const Fe& a, const Fe& b) {
    Fe o;
#pragma unroll
    for (int j = 0; j < 8; j++) o.l[j] = c ? a.l[j] : b.l[j];
    return o;
}

// t^((q+1)/4): the square root of a residue t, as q = 3 (mod 4).  The exponent is a constant, so every lane of a wave
// walks the same squarings and multiplications (the branch below is on the exponent, never on data).
__host__ __device__ inline Fe fq_sqrt_candidate(const Fe& t) {
    // (q + 1) / 4 = 0x0c19139cb84c680a6e14116da060561765e05aa45a1c72a34f082305b61f3f52, little-endian words
    constexpr uint32_t E[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    Fe res = t;  // bit 251, the top one
#pragma unroll 1
    for (int b = 250; b >= 0; b--) {
        res = Fq::sqr(res);
        if ((E[b >> 5] >> (b & 31)) & 1u) res = Fq::mul(res, t);
    }
    return res;
}

// GroupEncoding::from_bytes.  Returns the validity flag; `out` is the point in Montgomery form, (0,0) for the identity
// encoding (valid) and for every invalid one: an x not below q (a set bit 6 included), an x whose x^3 + 3 has no root
// (x = 0 with the sign set is one: 3 is a non-residue).  No branch on data before the final selects.
__host__ __device__ inline bool g1_decompress_one(const uint8_t b[32], Affine& out) {
    Fe x;
#pragma unroll
    for (int i = 0; i < 8; i++)
        x.l[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
    const uint32_t sign = x.l[7] >> 31;
    x.l[7] &= 0x7fffffffu;
    uint32_t pm[8], tmp[8];
#pragma unroll
    for (int i = 0; i < 8; i++) pm[i] = FqParams::p(i);
    const bool canonical = sub8(tmp, x.l, pm) != 0;  // x - q borrows: x < q
    x = g1c_select(canonical, x, fe_zero());
    const bool identity = canonical && fe_is_zero(x) && sign == 0;
    const Fe xm = Fq::from_raw(x);
    const Fe three = Fq::add(Fq::add(Fq::one(), Fq::one()), Fq::one());
    const Fe t = Fq::add(Fq::mul(Fq::sqr(xm), xm), three);
    Fe y = fq_sqrt_candidate(t);
    const bool is_root = fe_eq(Fq::sqr(y), t);
    const Fe y_raw = Fq::to_raw(y);
    y = g1c_select((y_raw.l[0] & 1u) != sign, Fq::neg(y), y);
    const bool point = canonical && is_root;  // (x = 0: t = 3 has no root, so the identity never passes for a point)
    out.x = g1c_select(point, xm, fe_zero());
    out.y = g1c_select(point, y, fe_zero());
    return point || identity;
}

}  // namespace zg
