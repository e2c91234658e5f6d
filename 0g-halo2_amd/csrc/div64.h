// Division by a 64-bit divisor fixed ahead of time: Moeller & Granlund, "Improved Division by Invariant Integers" (IEEE
// Trans. Comp. 2011), algorithm 4 -- d = divisor << s has its top bit set, v = floor((2^128 - 1) / d) - 2^64.  Two 64 x 64
// products and two conditional corrections, where the compiler's own 128-bit `%` is a shift-and-subtract loop over every
// bit.  Plain integer code for host and device: tests/abi/div64_probe.cpp holds it against `unsigned __int128` on the host.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ZG_DIV_HD __host__ __device__ __forceinline__
#else
#define ZG_DIV_HD inline
#endif

namespace zg {

struct Div64 {
    uint64_t d, v;
    uint32_t s;
};

inline Div64 make_div(uint64_t divisor) {  // divisor != 0
    Div64 k;
    k.s = (uint32_t)__builtin_clzll(divisor);
    k.d = divisor << k.s;
    k.v = (uint64_t)(~(unsigned __int128)0 / k.d - ((unsigned __int128)1 << 64));
    return k;
}

ZG_DIV_HD uint64_t mul_hi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// (u1, u0) / k.d with u1 < k.d: the remainder; *q = the quotient
ZG_DIV_HD uint64_t div_2by1(uint64_t u1, uint64_t u0, const Div64& k, uint64_t* q) {
    uint64_t q0 = k.v * u1, q1 = mul_hi64(k.v, u1);
    q0 += u0;
    q1 += u1 + (q0 < u0) + 1;
    uint64_t r = u0 - q1 * k.d;
    if (r > q0) { q1--; r += k.d; }
    if (r >= k.d) { q1++; r -= k.d; }
    *q = q1;
    return r;
}

// a * b mod p for a, b < p (so the high word of the product is below p)
ZG_DIV_HD uint64_t mul_mod(uint64_t a, uint64_t b, const Div64& p) {
    const uint64_t lo = a * b, hi = mul_hi64(a, b);
    uint64_t q;
    const uint64_t u1 = p.s ? (hi << p.s) | (lo >> (64 - p.s)) : hi;
    return div_2by1(u1, lo << p.s, p, &q) >> p.s;
}

// h mod divisor; *q = h / divisor
ZG_DIV_HD uint64_t div_mod(uint64_t h, const Div64& k, uint64_t* q) {
    return div_2by1(k.s ? h >> (64 - k.s) : 0, h << k.s, k, q) >> k.s;
}

}  // namespace zg
