// Scalar recoding of the per-point G1 multiplication (g1_mul.hip).  Plain C++ for host and device, no other header of
// the library: tests/abi/g1_mul_probe.hip runs it on the CPU against Python integers.
//
// The kernel walks a scalar from its TOP window down, one lane per scalar, so it needs digit w without the carries of
// the windows below it (the recoding of msm_var_digits.h runs bottom-up and would have to keep every digit of a lane: an
// array indexed by the loop counter, which on the device lives in scratch).  Biasing removes the carry chain: with
//     K = sum_{w < WINDOWS} 2^(W-1) 2^(W w)      and      T = s + K  (no overflow of 256 bits for s < 2^254)
// window w of T, taken as an unsigned W-bit number T_w, gives the signed digit d_w = T_w - 2^(W-1):
//     s = T - K = top 2^(W WINDOWS) + sum_w d_w 2^(W w),      -2^(W-1) <= d_w <= 2^(W-1) - 1,
// where top = T >> (W WINDOWS) is what is left of the 256 bits above the windows (TOP_BITS of them, unbiased; 0 or 1).
// The value sits in eight limbs picked by constant index and is shifted left W bits per digit: no runtime-indexed array.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ZG_G1MUL_HD __host__ __device__ inline
#else
#define ZG_G1MUL_HD inline
#endif

namespace zg {

template <uint32_t W>
struct G1MulDigits {
    static constexpr uint32_t WINDOWS = (255u + W - 1u) / W;  // covers a scalar below r < 2^254 with its bias
    static constexpr uint32_t TOP_BITS = 256u - W * WINDOWS;
    static constexpr int HALF = 1 << (W - 1);
    static_assert(W >= 2 && W <= 5, "window width");
    static_assert(W * WINDOWS <= 256u && TOP_BITS <= 1u, "the windows and at most one bit above them fill the 256 bits");

    uint32_t t[8];

    static constexpr uint32_t bias_limb(uint32_t i) {
        uint32_t v = 0;
        for (uint32_t w = 0; w < WINDOWS; w++) {
            const uint32_t bit = W * w + (W - 1u);
            if (bit / 32u == i) v |= 1u << (bit % 32u);
        }
        return v;
    }

    // s: the canonical integer below 2^254, little-endian limbs
    ZG_G1MUL_HD void init(const uint32_t s[8]) {
        constexpr uint32_t K[8] = {bias_limb(0), bias_limb(1), bias_limb(2), bias_limb(3),
                                   bias_limb(4), bias_limb(5), bias_limb(6), bias_limb(7)};
        uint64_t c = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 8; i++) {
            c += (uint64_t)s[i] + K[i];
            t[i] = (uint32_t)c;
            c >>= 32;
        }
    }

    template <uint32_t C>
    ZG_G1MUL_HD uint32_t pop() {  // the top C bits; the rest moves up
        if (C == 0) return 0;
        const uint32_t v = t[7] >> ((32u - C) & 31u);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 7; i >= 1; i--) t[i] = (t[i] << (C & 31u)) | (t[i - 1] >> ((32u - C) & 31u));
        t[0] <<= (C & 31u);
        return v;
    }

    ZG_G1MUL_HD uint32_t top() { return pop<TOP_BITS>(); }          // call once, first
    ZG_G1MUL_HD int next() { return (int)pop<W>() - HALF; }        // then WINDOWS times: d_(WINDOWS-1) ... d_0
};

constexpr uint32_t G1_MUL_W = 2;  // the width g1_mul.hip is built with

}  // namespace zg
