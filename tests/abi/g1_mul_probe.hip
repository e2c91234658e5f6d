// Host probe of csrc/g1_mul_digits.h (tests/test_srs_update_host.py): the recoding of the per-point G1 multiplication on
// the CPU.
//   g1_mul_probe FILE   every line of FILE is "W hex": prints "WINDOWS top d_(WINDOWS-1) ... d_0" (signed decimal digits,
//                       in the order the kernel meets them)
//   g1_mul_probe width  prints the width the kernel is built with
// Nothing here touches a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../0g-halo2_amd/csrc/g1_mul_digits.h"

static int hexval(char ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    if (ch >= 'A' && ch <= 'F') return ch - 'A' + 10;
    return -1;
}

template <uint32_t W>
static void digits(const uint32_t s[8]) {
    zg::G1MulDigits<W> d;
    d.init(s);
    printf("%u %u", zg::G1MulDigits<W>::WINDOWS, d.top());
    for (uint32_t w = 0; w < zg::G1MulDigits<W>::WINDOWS; w++) printf(" %d", d.next());
    for (int i = 0; i < 8; i++)
        if (d.t[i] != 0) {  // every bit of s + K has been handed out
            fprintf(stderr, "bits left after the last digit\n");
            exit(4);
        }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILE | width\n", argv[0]);
        return 2;
    }
    if (strcmp(argv[1], "width") == 0) {
        printf("%u\n", zg::G1_MUL_W);
        return 0;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char line[256];
    while (fgets(line, sizeof line, f)) {
        unsigned c = 0;
        char hex[128];
        if (sscanf(line, "%u %100s", &c, hex) != 2) return 3;
        const size_t len = strlen(hex);
        if (len == 0 || len > 64) return 3;
        uint32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < len; i++) {  // hex[len - 1 - i] is nibble i
            const int v = hexval(hex[len - 1 - i]);
            if (v < 0) return 3;
            s[i / 8] |= (uint32_t)v << (4 * (i % 8));
        }
        switch (c) {
            case 2: digits<2>(s); break;
            case 3: digits<3>(s); break;
            case 4: digits<4>(s); break;
            case 5: digits<5>(s); break;
            default: return 3;
        }
    }
    fclose(f);
    return 0;
}
