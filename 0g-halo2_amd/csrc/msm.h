// What msm.hip offers the rest of the library: one entry for an MSM launch sequence, and the tables of a base set.
#pragma once

#include "common.h"

namespace zg {

// One MSM launch sequence: `batch` scalar vectors of `n` elements each, multiplied against the first n points of a base
// set; vector v's sum goes to out[v] (XYZZ).  The batch may be batch / per groups of `per` vectors (the same commitments
// of several proofs): vector v = group * per + j lives at scalars + group * outer + j * stride.
struct MsmJob {
    const zg_bases* bases = nullptr;    // what vectors j < split of every group are multiplied against
    const zg_bases* bases_b = nullptr;  // ... and vectors j >= split (same length and window size, e.g. ParamsKZG::g_lagrange
                                        // and ::g in ONE launch sequence); null: every vector against `bases`
    size_t split = 0;
    const Fe* scalars = nullptr;
    size_t stride = 0;
    size_t per = 0, outer = 0;  // per = 0: one group (v = j)
    size_t batch = 0, n = 0;
    XYZZ* out = nullptr;        // device memory, or host memory mapped into the device's address space
    uint64_t run_mask = 0;      // bit j (j < 64): vector j of every group is multiplied in the run form (msm_digits_kernel);
                                // its base set must have its running-sum table (bases_enable_runs)
    uint32_t naf_width = 0;     // digit width against a bit-position table, 0 = the width the table was made for
};
int msm_dev(zg_ctx* ctx, const MsmJob& job);

int bases_enable_runs(zg_ctx* ctx, zg_bases* b);  // running-sum table for the run form (idempotent)
// b->dense: one row per bit position, odd w-bit digits (strict: refuse a table made for another default width)
int bases_enable_naf(zg_ctx* ctx, zg_bases* b, uint32_t w, bool strict = false);
int bases_register_dev(zg_ctx* ctx, const Affine* d_bases, size_t n, uint32_t window_bits, zg_bases** out);
// digit tables of the latency form (every multiple of every window; window_bits 0 = from n and the free memory, which may
// decide on none); with_runs: for the running sums too (the set must have its running-sum table)
int bases_enable_full(zg_ctx* ctx, zg_bases* b, uint32_t window_bits, bool with_runs);
uint32_t default_full_bits(size_t n, double budget_bytes);  // 0 = no digit tables at this size / budget
void xyzz_batch_normalise(const XYZZ* in, size_t count, zg_g1* out);

}  // namespace zg
