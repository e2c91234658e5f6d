// The order the witness check sorts the rows of a shuffle side in (check.hip), for host and device:
// the kernels and tests/abi/check_tuple_probe.hip compile this very text.
//
// A side's tuples are CANONICAL integers (not Montgomery limbs): component e of row r is the eight little-endian 32-bit
// limbs at v + (e * n + r) * 8.  Rows order by (tuple, row): tuples lexicographically, component 0 first, each component
// as one 256-bit integer; the row index is the last key, so the order is total.  Rows from `usable` on are no rows of the
// argument: they come last, whatever they hold.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZG_TUP_HD __host__ __device__ __forceinline__

namespace zg {

struct RowTuples {
    const uint32_t* v;  // [width][n][8]
    uint32_t n, usable, width;
};

// eight limbs as one integer: -1 / 0 / +1
ZG_TUP_HD int limbs_cmp(const uint32_t* a, const uint32_t* b) {
    for (int i = 7; i >= 0; i--) {
        if (a[i] < b[i]) return -1;
        if (a[i] > b[i]) return 1;
    }
    return 0;
}

// sign of (row i's tuple in a) - (row j's tuple in b); both of a.width components
ZG_TUP_HD int row_tuple_cmp(const RowTuples& a, uint32_t i, const RowTuples& b, uint32_t j) {
    for (uint32_t e = 0; e < a.width; e++) {
        const int s = limbs_cmp(a.v + ((size_t)e * a.n + i) * 8, b.v + ((size_t)e * b.n + j) * 8);
        if (s) return s;
    }
    return 0;
}

// does row i come after row j?  (i != j: a strict total order)
ZG_TUP_HD bool row_after(const RowTuples& t, uint32_t i, uint32_t j) {
    const bool oi = i >= t.usable, oj = j >= t.usable;
    if (oi || oj) return oi != oj ? oi : i > j;
    const int s = row_tuple_cmp(t, i, t, j);
    return s ? s > 0 : i > j;
}

}  // namespace zg
