// Host probe of csrc/msm_var_digits.h (tests/test_msm_var_host.py): the recoding of the variable-base MSM on the CPU.
//   msm_var_probe digits FILE   every line of FILE is "c hex": prints "W d_0 d_1 ... d_(W-1)" (signed decimal digits)
//   msm_var_probe width FILE    every line of FILE is "n batch": prints the window width chosen at window_bits = 0
// Nothing here touches a device.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../0g-halo2_amd/csrc/msm_var_digits.h"

static int hexval(char ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    if (ch >= 'A' && ch <= 'F') return ch - 'A' + 10;
    return -1;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s digits|width FILE\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[2], "r");
    if (!f) {
        perror(argv[2]);
        return 2;
    }
    char line[256];
    if (strcmp(argv[1], "width") == 0) {
        while (fgets(line, sizeof line, f)) {
            unsigned long long n = 0, batch = 0;
            if (sscanf(line, "%llu %llu", &n, &batch) != 2) return 3;
            printf("%u\n", zg::msm_var_default_bits((size_t)n, (size_t)batch));
        }
        fclose(f);
        return 0;
    }
    if (strcmp(argv[1], "digits") != 0) return 2;
    while (fgets(line, sizeof line, f)) {
        unsigned c = 0;
        char hex[128];
        if (sscanf(line, "%u %100s", &c, hex) != 2 || c < 2 || c > 16) return 3;
        const size_t len = strlen(hex);
        if (len == 0 || len > 64) return 3;
        uint32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < len; i++) {  // hex[len - 1 - i] is nibble i
            const int v = hexval(hex[len - 1 - i]);
            if (v < 0) return 3;
            s[i / 8] |= (uint32_t)v << (4 * (i % 8));
        }
        const uint32_t W = zg::msm_var_windows(c);
        // sentinel-framed, strided output: the recoding must write exactly W words, `stride` apart
        const size_t stride = 3;
        std::vector<uint32_t> out((size_t)W * stride + 2 * stride, 0xdeadbeefu);
        zg::msm_var_recode(s, c, W, out.data() + stride, stride);
        for (size_t i = 0; i < out.size(); i++) {
            const bool written = i >= stride && i < stride + (size_t)W * stride && (i - stride) % stride == 0;
            if (!written && out[i] != 0xdeadbeefu) {
                fprintf(stderr, "word %zu outside the digits was written\n", i);
                return 4;
            }
        }
        printf("%u", W);
        for (uint32_t w = 0; w < W; w++) {
            const uint32_t e = out[stride + (size_t)w * stride];
            const long long mag = (long long)(e & 0x7fffffffu);
            printf(" %lld", (e >> 31) ? -mag : mag);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
