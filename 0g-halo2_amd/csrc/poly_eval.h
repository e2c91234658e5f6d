// Device helpers shared by the row-parallel kernels of poly.hip and check.hip: 32-byte loads / stores and the
// expression interpreter over HBM-resident columns.
#pragma once

#include "poly.h"

namespace zg {

__device__ __forceinline__ Fe ldg(const Fe* p) {
    Fe r;
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 a = q[0], b = q[1];
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}
__device__ __forceinline__ void stg(Fe* p, const Fe& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// ------------------------------------------------------------------ expression interpreter
// (Load: how a cell is read -- ldg as it stands, or with the slabs' factor taken off: poly.hip's shuffle pass over h)
struct LoadPlain {
    __device__ __forceinline__ Fe operator()(const Fe* p) const { return ldg(p); }
};
template <class Load>
__device__ __forceinline__ Fe eval_poly_with(const DevCircuit& c, const Cols& cols, zg_poly p, uint32_t row, const Load& ld) {
    const uint32_t mask = (1u << cols.log_size) - 1u;
    Fe acc = fe_zero();
    for (uint32_t m = p.first; m < p.first + p.count; m++) {
        const DMono* mo = c.monos + m;
        const uint32_t nf = mo->n_factors;
        Fe prod;
        uint32_t f = 0;
        if (mo->coeff_is_one == 1 && nf > 0) {
            const zg_query q = c.queries[mo->factors[0]];
            const Fe* base = q.kind == ZG_FIXED ? cols.fixed : q.kind == ZG_ADVICE ? cols.advice : cols.instance;
            uint32_t idx = (row + (uint32_t)(q.rotation * cols.rot_scale)) & mask;
            prod = ld(base + ((size_t)q.column << cols.log_size) + idx);
            f = 1;
        } else {
            prod = mo->coeff;
        }
        for (; f < nf; f++) {
            const zg_query q = c.queries[mo->factors[f]];
            const Fe* base = q.kind == ZG_FIXED ? cols.fixed : q.kind == ZG_ADVICE ? cols.advice : cols.instance;
            uint32_t idx = (row + (uint32_t)(q.rotation * cols.rot_scale)) & mask;
            prod = Fr::mul(prod, ld(base + ((size_t)q.column << cols.log_size) + idx));
        }
        acc = Fr::add(acc, prod);
    }
    return acc;
}
__device__ __forceinline__ Fe eval_poly(const DevCircuit& c, const Cols& cols, zg_poly p, uint32_t row) {
    return eval_poly_with(c, cols, p, row, LoadPlain{});
}

__device__ __forceinline__ Cols cols_of(const Cols& c, uint32_t b) {  // proof b's view of a batch's columns
    Cols r = c;
    r.advice += (size_t)b * c.adv_bs;
    r.instance += (size_t)b * c.inst_bs;
    return r;
}

}  // namespace zg
