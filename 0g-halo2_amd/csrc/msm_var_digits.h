// Scalar recoding and window choice of the variable-base MSM (msm_var.hip).  Plain C++ for host and device, no other
// header of the library: tests/abi/msm_var_probe.hip runs it on the CPU against Python integers.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ZG_VAR_HD __host__ __device__ inline
#else
#define ZG_VAR_HD inline
#endif

namespace zg {

// windows of c bits that cover a scalar below r < 2^254 AND leave the top digit non-negative: W c >= 255
ZG_VAR_HD uint32_t msm_var_windows(uint32_t c) { return (255u + c - 1u) / c; }

// Signed c-bit digits of the integer s = sum_j s[j] 2^(32 j) < 2^254 (2 <= c <= 16, windows = msm_var_windows(c)):
//     s = sum_w d_w 2^(c w),   |d_w| <= 2^(c-1),   d_(windows-1) >= 0
// (a window value above 2^(c-1) becomes value - 2^c and carries one into the next window; the top window holds at most
// 254 - c (W - 1) <= c - 1 bits of s, so with the carry it stays at 2^(c-1) or below and nothing carries out).
// Digit w goes to out[w * stride] as |d| | sign << 31; 0 = no entry.  Every window owns its bucket set here, so the
// s + t r balancing of msm_digits_kernel has no use.
// The value is walked with a 64-bit sliding register, the limbs picked by constant index: no runtime-indexed array,
// which on the device would live in scratch.
ZG_VAR_HD void msm_var_recode(const uint32_t s[8], uint32_t c, uint32_t windows, uint32_t* out, size_t stride) {
    const uint32_t half = 1u << (c - 1), mask = (1u << c) - 1u;
    uint64_t bits = (uint64_t)s[0] | ((uint64_t)s[1] << 32);
    uint32_t have = 64, next = 2, carry = 0;
    for (uint32_t w = 0; w < windows; w++) {
        if (have < c && next < 8) {  // refill: have < c <= 16, so 32 fresh bits fit above what is left
            const uint32_t limb = next == 2 ? s[2] : next == 3 ? s[3] : next == 4 ? s[4] : next == 5 ? s[5] : next == 6 ? s[6] : s[7];
            bits |= (uint64_t)limb << have;
            have += 32;
            next++;
        }
        const uint32_t d = ((uint32_t)bits & mask) + carry;  // 0 .. 2^c
        bits >>= c;
        have = have >= c ? have - c : 0;
        carry = d > half ? 1u : 0u;
        const uint32_t k = carry ? (mask + 1u) - d : d;
        out[(size_t)w * stride] = k ? (k | (carry << 31)) : 0u;
    }
}

// Window width at window_bits = 0.  One vector costs about W (n + a 2^(c-1)) accumulated points: every window adds its n
// points into buckets and then reduces 2^(c-1) buckets; a = 4 is what a bucket costs the reduction of msm_var.hip in units
// of one accumulated point (a 10-product mixed addition): two full additions of 14 products in msm_var_strip (run += B,
// loc += run) and the bucket's share of merging task sums and of msm_var_strip_sum.  The smallest such cost wins; it
// stays at 2 or 3 below n = 32, as halo2's own rule (c = 3 below 32 points) does.  The batch only bounds memory: the
// width drops while batch * W * 2^(c-1) bucket slots exceed 2^24 (2.4 GB of 144-byte sums).
inline uint32_t msm_var_default_bits(size_t n, size_t batch) {
    const uint64_t a = 4;
    uint32_t best = 2;
    uint64_t best_cost = ~0ull;
    for (uint32_t c = 2; c <= 16; c++) {
        const uint64_t cost = (uint64_t)msm_var_windows(c) * ((uint64_t)n + (a << (c - 1)));
        if (cost < best_cost) {
            best_cost = cost;
            best = c;
        }
    }
    while (best > 2 && (uint64_t)batch * msm_var_windows(best) * (1ull << (best - 1)) > (1ull << 24)) best--;
    return best;
}

}  // namespace zg
