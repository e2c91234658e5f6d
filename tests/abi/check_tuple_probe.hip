// Host probe of csrc/check_tuple.h (tests/test_check_tuple_host.py): the (tuple, row) order the witness check sorts a
// shuffle side's rows in, on the CPU -- the header is the text the kernels of csrc/check.hip compile.
//   check_tuple_probe FILE   FILE: "n usable width", then n lines of `width` hex values (canonical integers below 2^256,
//                            row by row).  Prints the n row indices in the order of row_after, one per line, then one line
//                            "cmp" with row_tuple_cmp of every neighbouring pair of that order among the usable rows.
// Nothing here touches a device.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../0g-halo2_amd/csrc/check_tuple.h"

static int hexval(char ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    if (ch >= 'A' && ch <= 'F') return ch - 'A' + 10;
    return -1;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FILE\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    unsigned n = 0, usable = 0, width = 0;
    if (fscanf(f, "%u %u %u", &n, &usable, &width) != 3 || n == 0 || n > (1u << 20) || usable > n || width == 0 || width > 4) return 3;
    std::vector<uint32_t> v((size_t)width * n * 8, 0);
    for (unsigned r = 0; r < n; r++) {
        for (unsigned e = 0; e < width; e++) {
            char hex[128];
            if (fscanf(f, "%100s", hex) != 1) return 3;
            const size_t len = strlen(hex);
            if (len == 0 || len > 64) return 3;
            uint32_t* s = v.data() + ((size_t)e * n + r) * 8;
            for (size_t i = 0; i < len; i++) {  // hex[len - 1 - i] is nibble i
                const int d = hexval(hex[len - 1 - i]);
                if (d < 0) return 3;
                s[i / 8] |= (uint32_t)d << (4 * (i % 8));
            }
        }
    }
    fclose(f);
    const zg::RowTuples t{v.data(), n, usable, width};
    std::vector<uint32_t> idx(n);
    for (unsigned r = 0; r < n; r++) idx[r] = r;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return a != b && zg::row_after(t, b, a); });
    for (unsigned i = 0; i < n; i++) printf("%u\n", idx[i]);
    printf("cmp");
    for (unsigned i = 0; i + 1 < usable; i++) printf(" %d", zg::row_tuple_cmp(t, idx[i], t, idx[i + 1]));
    printf("\n");
    return 0;
}
