// BLAKE2b (RFC 7693) as halo2's own transcript uses it -- Blake2bWrite / Blake2bRead with Challenge255, halo2_proofs
// v2023_04_20 src/transcript/blake2b.rs: 64-byte digest, no key, personalisation "Halo2-Transcript" -- shared by the two
// sides of the format: the host writer (transcript.h) and the device reader that replays a proof (verify.hip).
//
// The state streams: bytes go into a 128-byte block, and a block that is exactly full is NOT compressed until another byte
// arrives, because BLAKE2b marks its last block and a squeeze may finalise right there.  A squeeze finalises a COPY; the
// live state goes on (the transcript never resets its hash).
//
// Written from the published sources, not compiled against the crates (DESIGN.md section 17 lists what remains to be
// verified when they are at hand).
#pragma once

#include "field.h"

namespace zg {

struct Blake2b {
    uint64_t h[8];
    uint64_t m[16];  // the pending block, little-endian words
    uint64_t t;      // bytes compressed so far (a transcript stays far below 2^64)
    uint32_t pos;    // bytes pending in m, 0 .. 128
};

__host__ __device__ __forceinline__ uint64_t b2_ror(uint64_t x, uint32_t s) { return (x >> s) | (x << (64 - s)); }

__host__ __device__ inline void b2_compress(Blake2b& s, uint64_t t, bool last) {
    constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    constexpr uint8_t SIGMA[10][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
    uint64_t v[16];
    for (int i = 0; i < 8; i++) {
        v[i] = s.h[i];
        v[8 + i] = IV[i];
    }
    v[12] ^= t;  // (the high word of the counter stays 0)
    if (last) v[14] = ~v[14];
#define ZG_B2_G(a, b, c, d, x, y)      \
    v[a] = v[a] + v[b] + (x);          \
    v[d] = b2_ror(v[d] ^ v[a], 32);    \
    v[c] = v[c] + v[d];                \
    v[b] = b2_ror(v[b] ^ v[c], 24);    \
    v[a] = v[a] + v[b] + (y);          \
    v[d] = b2_ror(v[d] ^ v[a], 16);    \
    v[c] = v[c] + v[d];                \
    v[b] = b2_ror(v[b] ^ v[c], 63)
#pragma unroll 1
    for (int r = 0; r < 12; r++) {
        const uint8_t* g = SIGMA[r % 10];
        ZG_B2_G(0, 4, 8, 12, s.m[g[0]], s.m[g[1]]);
        ZG_B2_G(1, 5, 9, 13, s.m[g[2]], s.m[g[3]]);
        ZG_B2_G(2, 6, 10, 14, s.m[g[4]], s.m[g[5]]);
        ZG_B2_G(3, 7, 11, 15, s.m[g[6]], s.m[g[7]]);
        ZG_B2_G(0, 5, 10, 15, s.m[g[8]], s.m[g[9]]);
        ZG_B2_G(1, 6, 11, 12, s.m[g[10]], s.m[g[11]]);
        ZG_B2_G(2, 7, 8, 13, s.m[g[12]], s.m[g[13]]);
        ZG_B2_G(3, 4, 9, 14, s.m[g[14]], s.m[g[15]]);
    }
#undef ZG_B2_G
    for (int i = 0; i < 8; i++) s.h[i] ^= v[i] ^ v[8 + i];
}

// digest length 64, no key, fanout = depth = 1, no salt, the 16 bytes of personalisation in the last two parameter words
__host__ __device__ inline void b2_init(Blake2b& s, uint64_t person_lo, uint64_t person_hi) {
    constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
    for (int i = 0; i < 8; i++) s.h[i] = IV[i];
    s.h[0] ^= 0x01010040ULL;
    s.h[6] ^= person_lo;
    s.h[7] ^= person_hi;
    for (int i = 0; i < 16; i++) s.m[i] = 0;
    s.t = 0;
    s.pos = 0;
}
// "Halo2-Transcript" as two little-endian words
constexpr uint64_t B2_HALO2_LO = 0x72542d326f6c6148ULL;  // "Halo2-Tr"
constexpr uint64_t B2_HALO2_HI = 0x7470697263736e61ULL;  // "anscript"
__host__ __device__ inline void b2_init_halo2(Blake2b& s) { b2_init(s, B2_HALO2_LO, B2_HALO2_HI); }

__host__ __device__ inline void b2_byte(Blake2b& s, uint32_t b) {
    if (s.pos == 128) {  // the full block was not the last one after all
        s.t += 128;
        b2_compress(s, s.t, false);
        for (int i = 0; i < 16; i++) s.m[i] = 0;
        s.pos = 0;
    }
    s.m[s.pos >> 3] |= (uint64_t)(b & 0xff) << (8 * (s.pos & 7));
    s.pos++;
}
__host__ __device__ inline void b2_update(Blake2b& s, const uint8_t* data, size_t len) {
    for (size_t i = 0; i < len; i++) b2_byte(s, data[i]);
}
// the digest of everything absorbed so far; the state itself is untouched (clone and finalise)
__host__ __device__ inline void b2_digest(const Blake2b& s, uint8_t out[64]) {
    Blake2b c = s;  // (the bytes of m past pos are zero: b2_byte clears a block before it refills it)
    b2_compress(c, c.t + c.pos, true);
    for (int k = 0; k < 64; k++) out[k] = (uint8_t)(c.h[k >> 3] >> (8 * (k & 7)));
}

// 32 little-endian bytes of a canonical integer (8 LE u32 limbs): to_repr()
__host__ __device__ inline void b2_int(Blake2b& s, const Fe& raw) {
    for (int k = 0; k < 32; k++) b2_byte(s, raw.l[k >> 2] >> (8 * (k & 3)));
}

// Challenge255::new: the 64-byte digest as a little-endian integer, reduced mod r (Fr::from_bytes_wide).
// lo + 2^256 hi with both halves first brought below r (at most five subtractions each: 2^256 < 6r); 2^256 = R, whose
// Montgomery form is R^2 mod r.
__host__ __device__ inline Fe challenge_from_wide(const uint8_t d[64]) {
    Fe half[2];
    uint32_t pm[8], t[8];
    for (int i = 0; i < 8; i++) pm[i] = FrParams::p(i);
    for (int w = 0; w < 2; w++) {
        Fe& v = half[w];
        for (int i = 0; i < 8; i++)
            v.l[i] = (uint32_t)d[32 * w + 4 * i] | ((uint32_t)d[32 * w + 4 * i + 1] << 8) | ((uint32_t)d[32 * w + 4 * i + 2] << 16) |
                     ((uint32_t)d[32 * w + 4 * i + 3] << 24);
        for (int r = 0; r < 6; r++) {
            if (sub8(t, v.l, pm)) break;
            for (int i = 0; i < 8; i++) v.l[i] = t[i];
        }
    }
    return Fr::add(Fr::from_raw(half[0]), Fr::mul(Fr::from_raw(half[1]), FrParams::r2()));
}

// squeeze_challenge: absorb 0x00, finalise a clone, reduce; the live state keeps the byte and goes on
__host__ __device__ inline Fe b2_squeeze(Blake2b& s) {
    b2_byte(s, 0);
    uint8_t d[64];
    b2_digest(s, d);
    return challenge_from_wide(d);
}

}  // namespace zg
