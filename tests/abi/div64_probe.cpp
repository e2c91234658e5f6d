// Host check of csrc/div64.h (the invariant-divisor arithmetic of the WNN hash, csrc/wnn.hip) against unsigned __int128:
// div_mod and mul_mod for edge and seeded random divisors and operands; prints how often each correction step of
// div_2by1 was needed, so that the test can see both were reached.  Built and run by tests/test_wnn_div_host.py.
#include <cstdio>
#include <cstdint>

#include "div64.h"

typedef unsigned __int128 u128;
using namespace zg;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static long first_fix = 0, second_fix = 0;
// div_2by1 restated with counters: which corrections does an operand pair take?
static void count_fixes(uint64_t u1, uint64_t u0, const Div64& k) {
    uint64_t q0 = k.v * u1, q1 = mul_hi64(k.v, u1);
    q0 += u0;
    q1 += u1 + (q0 < u0) + 1;
    uint64_t r = u0 - q1 * k.d;
    if (r > q0) { first_fix++; r += k.d; }
    if (r >= k.d) second_fix++;
}

int main() {
    const uint64_t fixed[] = {1, 2, 3, 5, 7, 13, 100, 251, 256, 8192, 65536, (1ull << 32) - 1, 1ull << 32, (1ull << 53) - 111,
                              (1ull << 61) - 1, 1ull << 63, (1ull << 63) + 1, 0x8000000000000001ull, 0xFFFFFFFFFFFFFFC5ull, ~0ull};
    const int n_fixed = sizeof(fixed) / sizeof(fixed[0]);
    long checked = 0, bad = 0;
    for (int r = 0; r < 200; r++) {
        const uint64_t d = r < n_fixed ? fixed[r] : ((rnd() >> (rnd() % 64)) | 1);
        const Div64 k = make_div(d);
        const uint64_t edge[] = {0, 1, d - 1, d, d + 1, ~0ull, ~0ull - 1, 1ull << 63, d << 1, (d << 1) - 1};
        // div_2by1 itself at the corners of its domain (u1 < k.d): (k.d - 2, 2^64 - 1) takes the second correction
        const uint64_t hi[] = {0, 1, k.d >> 1, k.d - 2, k.d - 1}, lo[] = {0, 1, k.d, ~0ull - 1, ~0ull};
        for (uint64_t u1 : hi)
            for (uint64_t u0 : lo) {
                uint64_t q;
                const u128 u = (u128)u1 << 64 | u0;
                if (div_2by1(u1, u0, k, &q) != (uint64_t)(u % k.d) || q != (uint64_t)(u / k.d)) bad++;
                count_fixes(u1, u0, k);
                checked++;
            }
        for (int i = 0; i < 20000; i++) {
            const uint64_t x = i < 10 ? edge[i] : rnd() >> (rnd() % 64);
            uint64_t q;
            const uint64_t rem = div_mod(x, k, &q);
            if (rem != x % d || q != x / d) bad++;
            count_fixes(k.s ? x >> (64 - k.s) : 0, x << k.s, k);
            uint64_t a = x % d, b = (rnd() >> (rnd() % 64)) % d;
            if (i < 4) a = b = d - 1;
            if (mul_mod(a, b, k) != (uint64_t)((u128)a * b % d)) bad++;
            const u128 prod = (u128)a * b << k.s;  // (below d * 2^64: a, b < divisor)
            count_fixes((uint64_t)(prod >> 64), (uint64_t)prod, k);
            checked += 2;
        }
    }
    printf("checked %ld bad %ld first_correction %ld second_correction %ld\n", checked, bad, first_fix, second_fix);
    return bad != 0;
}
