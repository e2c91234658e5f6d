// Keccak-f[1600], Keccak-256, EvmTranscript's challenge rule and its streaming sponge, shared by the two sides of the
// transcript format: the host writer (transcript.h, used by prove_batch.hip) and the device reader that replays a proof
// (verify.hip, which holds no hash code of its own).
#pragma once

#include <cstring>

#include "field.h"

namespace zg {

__host__ __device__ __forceinline__ uint64_t keccak_rol(uint64_t x, uint32_t s) {
    return s ? (x << s) | (x >> (64 - s)) : x;
}

__host__ __device__ inline void keccak_f1600(uint64_t a[25]) {
    constexpr uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
        0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
        0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
        0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
        0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
        0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    // rho offsets indexed [x + 5y]
    constexpr uint32_t RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    for (int round = 0; round < 24; round++) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ keccak_rol(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
        }
        // rho + pi: b[y, 2x+3y] = rot(a[x, y])
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rol(a[x + 5 * y], RHO[x + 5 * y]);
#pragma unroll
        for (int y = 0; y < 5; y++)
#pragma unroll
            for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= RC[round];
    }
}

constexpr uint32_t KECCAK_RATE = 136;  // bytes per absorbed block of Keccak-256

// Keccak-256 (original padding) on the host
inline void keccak256(const uint8_t* data, size_t len, uint8_t out[32]) {
    constexpr size_t rate = KECCAK_RATE;
    uint64_t st[25] = {0};
    auto absorb = [&](const uint8_t* blk) {
        for (size_t i = 0; i < rate / 8; i++) {
            uint64_t w = 0;
            for (int j = 0; j < 8; j++) w |= (uint64_t)blk[8 * i + j] << (8 * j);
            st[i] ^= w;
        }
        keccak_f1600(st);
    };
    while (len >= rate) {
        absorb(data);
        data += rate;
        len -= rate;
    }
    uint8_t last[rate];
    memset(last, 0, rate);
    memcpy(last, data, len);
    last[len] ^= 0x01;
    last[rate - 1] ^= 0x80;
    absorb(last);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 8; j++) out[8 * i + j] = (uint8_t)(st[i] >> (8 * j));
}

// EvmTranscript squeezes keccak256(buffer ++ [1]) when the buffer is exactly the previous 32-byte state (nothing was
// absorbed since), keccak256(buffer) otherwise
__host__ __device__ __forceinline__ bool squeeze_appends_one(size_t buffered) { return buffered == 32; }

// the challenge: the 32-byte hash as a big-endian integer, reduced mod r (at most five subtractions: 2^256 < 6r)
__host__ __device__ inline Fe challenge_from_hash(const uint8_t h[32]) {
    Fe v;
    for (int i = 0; i < 8; i++)
        v.l[i] = (uint32_t)h[31 - 4 * i] | ((uint32_t)h[30 - 4 * i] << 8) | ((uint32_t)h[29 - 4 * i] << 16) |
                 ((uint32_t)h[28 - 4 * i] << 24);
    uint32_t pm[8], t[8];
    for (int i = 0; i < 8; i++) pm[i] = FrParams::p(i);
    for (int r = 0; r < 6; r++) {
        if (sub8(t, v.l, pm)) break;
        for (int i = 0; i < 8; i++) v.l[i] = t[i];
    }
    return Fr::from_raw(v);
}

// EvmTranscript's hash state for a reader that streams: the bytes absorbed since the last squeeze go into the sponge as
// they come (transcript.h's writer keeps them in a buffer and hashes it whole)
struct Sponge {
    uint64_t st[25];
    uint32_t pos, len;
};
__host__ __device__ inline void sp_reset(Sponge& s) {
    for (int i = 0; i < 25; i++) s.st[i] = 0;
    s.pos = 0;
    s.len = 0;
}
__host__ __device__ inline void sp_byte(Sponge& s, uint32_t b) {
    s.st[s.pos >> 3] ^= (uint64_t)(b & 0xff) << (8 * (s.pos & 7));
    s.len++;
    if (++s.pos == KECCAK_RATE) {
        keccak_f1600(s.st);
        s.pos = 0;
    }
}
// 32 big-endian bytes of a canonical integer (8 LE u32 limbs)
__host__ __device__ inline void sp_int(Sponge& s, const Fe& raw) {
    for (int k = 0; k < 32; k++) sp_byte(s, raw.l[(31 - k) >> 2] >> (8 * ((31 - k) & 3)));
}
// the squeeze of transcript.h's EvmTranscript, on the streamed sponge; the state becomes the hash
__host__ __device__ inline Fe sp_squeeze(Sponge& s) {
    if (squeeze_appends_one(s.len)) sp_byte(s, 1);
    s.st[s.pos >> 3] ^= 0x01ull << (8 * (s.pos & 7));
    s.st[KECCAK_RATE / 8 - 1] ^= 0x80ull << 56;
    keccak_f1600(s.st);
    uint8_t h[32];
    for (int k = 0; k < 32; k++) h[k] = (uint8_t)(s.st[k >> 3] >> (8 * (k & 7)));
    sp_reset(s);
    for (int k = 0; k < 32; k++) sp_byte(s, h[k]);
    return challenge_from_hash(h);
}

}  // namespace zg
