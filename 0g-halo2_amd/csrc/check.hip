// Witness check for gfx950: halo2_proofs::dev::MockProver::verify on the data of this ABI (halo2_proofs v2023_04_20
// src/dev.rs; reached from Wnn::mock_proof, /root/reference/src/wnn.rs:203-210) for a lock-step batch of witnesses.
//
// Everything runs on the 2^k ROWS of the columns as they stand in the prover's slots -- no transform, no commitment:
//   gates    one lane per (row, gate, witness): the expression interpreter of evaluate_h's 8-limb form (eval_poly);
//   lookups  EXACT tuple membership.  The table side is made searchable by sorting its rows lexicographically by
//            tuple (a bitonic network over row indices in LDS whose comparator reads the tuples) and gathering the
//            tuples in that order; an input row then binary-searches with a component-by-component comparison.  No
//            theta-fold is involved, so no verdict can depend on one.  Tables that read fixed columns only are
//            prepared once per proving key, tables that read advice or instance cells per witness;
//   copies   one lane per (permutation column, row): its cell against the cell the mapping names, the mapping being
//            recovered on the host from the sigma values, once per proving key.
// A failing lane sets its bit in a per-witness bitmap [constraint][n / 64] (one wave ballot = one 64-bit word, plain
// vector stores) and a workgroup with failures bumps its witness's counter of that kind once.  The host reads the
// count x 3 totals; only a witness with failures has its bitmap read back and walked into ordered records.
//
// zg_prover_check_circuit*  add, through the same check_batch_impl:
//   challenges  the caller's values, one constant pseudo-column each behind the instance columns, read through Cols as
//               any column is;
//   shuffles    EXACT multiset equality.  Both sides' tuples are evaluated to canonical integers, each side's rows are
//               sorted by (tuple, row) with the index network of the lookup tables under the comparator of
//               check_tuple.h, and position by position the two orders are compared: the input row at a position whose
//               tuple differs from the shuffle row's at that position fails, and names that row.  A fourth total.
#include "prover.h"
#include "poly_eval.h"
#include "check_tuple.h"

#include <algorithm>

namespace zg {

constexpr uint32_t CK_MAX_LOOKUPS = 60;  // (zg_prover_create's limit)

// lookup l's sorted table ([width][n] elements, the first `usable` of each row meaningful) starts off[l] elements into
// the proving key's array, or, when bit l of var_mask is set, into its witness's
struct LkTabs {
    uint32_t off[CK_MAX_LOOKUPS];
    uint64_t var_mask;
};
// table preparation: slot s works on lookup lookup[s], its tuples at off[s]
struct TabSlots {
    uint32_t lookup[CK_MAX_LOOKUPS];
    uint32_t off[CK_MAX_LOOKUPS];
};

// limbs as one integer: -1 / 0 / +1 (any total order serves: both sides hold canonical Montgomery representatives)
__device__ __forceinline__ int fe_cmp(const Fe& a, const Fe& b) {
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        if (a.l[i] < b.l[i]) return -1;
        if (a.l[i] > b.l[i]) return 1;
    }
    return 0;
}

// Every lane of the workgroup calls this (256 lanes, lane t = row blockIdx.x * 256 + t): the wave's verdicts become one
// 64-bit word of the constraint's bitmap row, the workgroup's failures one addition to the witness's counter.
__device__ __forceinline__ void flag_rows(bool bad, uint32_t row, uint32_t n, unsigned long long* words, uint32_t* total) {
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63u) == 0 && row < n) words[row >> 6] = m;
    const int cnt = __syncthreads_count(bad);
    if (threadIdx.x == 0 && cnt) atomicAdd(total, (uint32_t)cnt);
}

__global__ __launch_bounds__(256) void check_gates_kernel(DevCircuit c, Cols cols_all, uint32_t n, uint32_t usable,
                                                          unsigned long long* __restrict__ bm, uint32_t nc, uint32_t w,
                                                          uint32_t* __restrict__ totals) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, b = blockIdx.z;
    bool bad = false;
    if (row < usable) {
        const Cols cols = cols_of(cols_all, b);
        bad = !fe_is_zero(eval_poly(c, cols, c.gates[g], row));
    }
    flag_rows(bad, row, n, bm + ((size_t)b * nc + g) * w, totals + 3 * b + ZG_FAIL_GATE);
}

// sign of (table tuple at sorted position `at`) - (input tuple)
__device__ __forceinline__ int tuple_cmp(const Fe* __restrict__ tab, uint32_t n, uint32_t at, const Fe* in, uint32_t width) {
#pragma unroll
    for (uint32_t e = 0; e < ZG_MAX_LOOKUP_WIDTH; e++) {
        if (e < width) {
            const int s = fe_cmp(ldg(tab + (size_t)e * n + at), in[e]);
            if (s) return s;
        }
    }
    return 0;
}

__global__ __launch_bounds__(256) void check_lookups_kernel(DevCircuit c, Cols cols_all, LkTabs tabs, const Fe* __restrict__ key_sorted,
                                                            const Fe* __restrict__ var_sorted, size_t var_bs, uint32_t n,
                                                            uint32_t usable, unsigned long long* __restrict__ bm, uint32_t nc,
                                                            uint32_t w, uint32_t* __restrict__ totals) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, b = blockIdx.z;
    bool bad = false;
    if (row < usable) {
        const Cols cols = cols_of(cols_all, b);
        const DLookup* lk = c.lookups + l;
        const uint32_t width = lk->width;
        Fe in[ZG_MAX_LOOKUP_WIDTH];
#pragma unroll
        for (uint32_t e = 0; e < ZG_MAX_LOOKUP_WIDTH; e++)
            if (e < width) in[e] = eval_poly(c, cols, lk->inputs[e], row);
        const Fe* tab = ((tabs.var_mask >> l) & 1ull) ? var_sorted + (size_t)b * var_bs + tabs.off[l] : key_sorted + tabs.off[l];
        uint32_t lo = 0, hi = usable;
        bool found = false;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const int s = tuple_cmp(tab, n, mid, in, width);
            if (s == 0) {
                found = true;
                break;
            }
            if (s < 0) lo = mid + 1;
            else hi = mid;
        }
        bad = !found;
    }
    flag_rows(bad, row, n, bm + ((size_t)b * nc + c.n_gates + l) * w, totals + 3 * b + ZG_FAIL_LOOKUP);
}

__device__ __forceinline__ const Fe* perm_cell(const DevCircuit& c, const Cols& cols, uint32_t pc, uint32_t row) {
    const zg_query q = c.perm_cols[pc];
    const Fe* base = q.kind == ZG_FIXED ? cols.fixed : q.kind == ZG_ADVICE ? cols.advice : cols.instance;
    return base + ((size_t)q.column << cols.log_size) + row;
}

// next: [n_perm][n] packed (column, row) of the cell that follows in the permutation cycle
__global__ __launch_bounds__(256) void check_copies_kernel(DevCircuit c, Cols cols_all, const uint2* __restrict__ next, uint32_t n,
                                                           unsigned long long* __restrict__ bm, uint32_t nc, uint32_t w,
                                                           uint32_t* __restrict__ totals) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x, pc = blockIdx.y, b = blockIdx.z;
    bool bad = false;
    if (row < n) {
        const Cols cols = cols_of(cols_all, b);
        const uint2 to = next[(size_t)pc * n + row];
        if (to.x != pc || to.y != row) bad = !fe_eq(ldg(perm_cell(c, cols, pc, row)), ldg(perm_cell(c, cols, to.x, to.y)));
    }
    flag_rows(bad, row, n, bm + ((size_t)b * nc + c.n_gates + c.n_lookups + pc) * w, totals + 3 * b + ZG_FAIL_COPY);
}

// permutation::keygen::Assembly::build_pk's values, one lane per cell: sigma[i] = delta^next_col[i] * omega^next_row[i]
// (dpow[c] = delta^c, tw[r] = omega^r: the resident twiddle table).  A cell whose indices name no label gets 0 and the
// smallest such cell index is left in *bad (0xffffffff: none).
__global__ __launch_bounds__(256) void permutation_sigma_kernel(const uint32_t* __restrict__ next_col, const uint32_t* __restrict__ next_row,
                                                                const Fe* __restrict__ tw, const Fe* __restrict__ dpow, uint32_t n,
                                                                uint32_t n_perm, uint32_t cells, Fe* __restrict__ sigma,
                                                                uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const uint32_t c = next_col[i], r = next_row[i];
    if (c >= n_perm || r >= n) {
        atomicMin(bad, i);
        sigma[i] = fe_zero();
        return;
    }
    sigma[i] = Fr::mul(ldg(dpow + c), ldg(tw + r));
}

// ------------------------------------------------------------------ the table side of the lookups
// vals + b * vals_bs + off[s] + e * n + row = table polynomial e of slot s's lookup at `row`
__global__ __launch_bounds__(256) void check_table_eval_kernel(DevCircuit c, Cols cols_all, TabSlots sl, Fe* __restrict__ vals,
                                                               size_t vals_bs, uint32_t n) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    if (row >= n) return;
    const Cols cols = cols_of(cols_all, b);
    const DLookup* lk = c.lookups + sl.lookup[s];
    Fe* out = vals + (size_t)b * vals_bs + sl.off[s] + row;
    for (uint32_t e = 0; e < lk->width; e++) stg(out + (size_t)e * n, eval_poly(c, cols, lk->tables[e], row));
}

struct TupView {
    const Fe* v;  // [width][n]
    uint32_t n, usable, width;
};
// row i's tuple after row j's?  Rows from `usable` on are no table rows: they sort last, equal among themselves.
__device__ __forceinline__ bool tup_greater(const TupView& t, uint32_t i, uint32_t j) {
    if (i >= t.usable || j >= t.usable) return i >= t.usable && j < t.usable;
    for (uint32_t e = 0; e < t.width; e++) {
        const int s = fe_cmp(ldg(t.v + (size_t)e * t.n + i), ldg(t.v + (size_t)e * t.n + j));
        if (s) return s > 0;
    }
    return false;
}

constexpr uint32_t CS_CH = 1024;  // row indices per LDS chunk
constexpr uint32_t CS_NT = 512;

// what the index network orders by: a lookup table's tuples, or a shuffle side's (tuple, row)
__device__ __forceinline__ bool row_greater(const TupView& t, uint32_t i, uint32_t j) { return tup_greater(t, i, j); }
__device__ __forceinline__ bool row_greater(const RowTuples& t, uint32_t i, uint32_t j) { return row_after(t, i, j); }

template <class View>
__device__ __forceinline__ void idx_cmpx(uint32_t* sh, const View& t, uint32_t i, uint32_t j, bool ascending) {
    const uint32_t a = sh[i], b = sh[j];
    if (row_greater(t, a, b) == ascending) {
        sh[i] = b;
        sh[j] = a;
    }
}

// The bitonic network of sort.hip over ROW INDICES (the keys stay where they are; a comparison gathers them), one
// workgroup of CS_NT lanes on the chunk of `len` indices at `base`, position g0 of its row.
// merge_size = 0: the indices are created here (idx[i] = i) and every chunk becomes a sorted run, direction alternating
// with bit CS_CH of its position; otherwise the strides below CS_CH of merge level `merge_size`.
template <class View>
__device__ __forceinline__ void idx_sort_local(uint32_t* sh, uint32_t* __restrict__ base, const View& t, uint32_t g0, uint32_t len,
                                               uint32_t merge_size) {
    for (uint32_t e = threadIdx.x; e < len; e += CS_NT) sh[e] = merge_size ? base[e] : g0 + e;
    __syncthreads();
    if (!merge_size) {
        for (uint32_t size = 2; size <= len; size <<= 1) {
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t q = threadIdx.x; q < len / 2; q += CS_NT) {
                    const uint32_t i = 2 * q - (q & (stride - 1));
                    idx_cmpx(sh, t, i, i + stride, ((g0 + i) & size) == 0);
                }
                __syncthreads();
            }
        }
    } else {
        const bool asc = (g0 & merge_size) == 0;
        for (uint32_t stride = CS_CH >> 1; stride > 0; stride >>= 1) {
            for (uint32_t q = threadIdx.x; q < CS_CH / 2; q += CS_NT) {
                const uint32_t i = 2 * q - (q & (stride - 1));
                idx_cmpx(sh, t, i, i + stride, asc);
            }
            __syncthreads();
        }
    }
    for (uint32_t e = threadIdx.x; e < len; e += CS_NT) base[e] = sh[e];
}

// one compare-exchange of the pass with stride >= CS_CH: pair q of the row of n indices at `base`
template <class View>
__device__ __forceinline__ void idx_sort_global(uint32_t* __restrict__ base, const View& t, uint32_t q, uint32_t size, uint32_t stride) {
    const uint32_t i = 2 * q - (q & (stride - 1)), j = i + stride;
    const uint32_t a = base[i], bb = base[j];
    if (row_greater(t, a, bb) == ((i & size) == 0)) {
        base[i] = bb;
        base[j] = a;
    }
}

__global__ __launch_bounds__(CS_NT) void check_sort_local_kernel(uint32_t* __restrict__ idx, size_t idx_bs, const Fe* __restrict__ vals,
                                                                 size_t vals_bs, DevCircuit c, TabSlots sl, uint32_t n,
                                                                 uint32_t usable, uint32_t merge_size) {
    __shared__ uint32_t sh[CS_CH];
    const uint32_t s = blockIdx.y, b = blockIdx.z;
    const uint32_t g0 = blockIdx.x * CS_CH;
    const TupView t{vals + (size_t)b * vals_bs + sl.off[s], n, usable, c.lookups[sl.lookup[s]].width};
    idx_sort_local(sh, idx + (size_t)b * idx_bs + (size_t)s * n + g0, t, g0, n < CS_CH ? n : CS_CH, merge_size);
}

__global__ __launch_bounds__(256) void check_sort_global_kernel(uint32_t* __restrict__ idx, size_t idx_bs, const Fe* __restrict__ vals,
                                                                size_t vals_bs, DevCircuit c, TabSlots sl, uint32_t n, uint32_t usable,
                                                                uint32_t size, uint32_t stride) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    if (q >= n / 2) return;
    const TupView t{vals + (size_t)b * vals_bs + sl.off[s], n, usable, c.lookups[sl.lookup[s]].width};
    idx_sort_global(idx + (size_t)b * idx_bs + (size_t)s * n, t, q, size, stride);
}

// sorted[.. + e * n + i] = vals[.. + e * n + idx[i]], i < usable
__global__ __launch_bounds__(256) void check_table_gather_kernel(const uint32_t* __restrict__ idx, size_t idx_bs,
                                                                 const Fe* __restrict__ vals, size_t vals_bs, Fe* __restrict__ sorted,
                                                                 size_t sorted_bs, DevCircuit c, TabSlots sl, uint32_t n, uint32_t usable) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    if (i >= usable) return;
    const uint32_t from = idx[(size_t)b * idx_bs + (size_t)s * n + i];
    if (from >= usable) return;  // (cannot happen: the usable rows sort first)
    const uint32_t width = c.lookups[sl.lookup[s]].width;
    const Fe* in = vals + (size_t)b * vals_bs + sl.off[s];
    Fe* out = sorted + (size_t)b * sorted_bs + sl.off[s];
    for (uint32_t e = 0; e < width; e++) stg(out + (size_t)e * n + i, ldg(in + (size_t)e * n + from));
}

// Tables of the `ns` lookups in sl, for nb witnesses: vals / sorted [nb][*_bs] elements, idx [nb][ns * n] words.
static int prepare_tables(zg_ctx* ctx, const DevCircuit& dc, const Cols& cols, const TabSlots& sl, uint32_t ns, uint32_t nb,
                          Fe* vals, size_t vals_bs, Fe* sorted, size_t sorted_bs, uint32_t* idx, uint32_t n, uint32_t usable) {
    if (!ns || !nb) return ZG_OK;
    const size_t idx_bs = (size_t)ns * n;
    const double cells = (double)nb * (double)vals_bs;
    ZG_LAUNCH(ctx, "check_table_eval", cells * 64, check_table_eval_kernel, dim3((n + 255) / 256, ns, nb), dim3(256), 0, dc, cols, sl,
              vals, vals_bs, n);
    const uint32_t chunks = n <= CS_CH ? 1 : n / CS_CH;
    const dim3 gl(chunks, ns, nb), gg((n / 2 + 255) / 256, ns, nb);
    ZG_LAUNCH(ctx, "check_sort_local", cells * 32, check_sort_local_kernel, gl, dim3(CS_NT), 0, idx, idx_bs, vals, vals_bs, dc, sl, n,
              usable, 0u);
    for (uint32_t size = 2 * CS_CH; size <= n; size <<= 1) {
        for (uint32_t stride = size >> 1; stride >= CS_CH; stride >>= 1)
            ZG_LAUNCH(ctx, "check_sort_global", cells * 32, check_sort_global_kernel, gg, dim3(256), 0, idx, idx_bs, vals, vals_bs, dc, sl,
                      n, usable, size, stride);
        ZG_LAUNCH(ctx, "check_sort_local", cells * 32, check_sort_local_kernel, gl, dim3(CS_NT), 0, idx, idx_bs, vals, vals_bs, dc, sl, n,
                  usable, size);
    }
    ZG_LAUNCH(ctx, "check_table_gather", cells * 64, check_table_gather_kernel, dim3((usable + 255) / 256, ns, nb), dim3(256), 0, idx,
              idx_bs, vals, vals_bs, sorted, sorted_bs, dc, sl, n, usable);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ challenges and shuffles (zg_prover_check_circuit*)
// inst + b * inst_bs + (col0 + j) * n + row = challenge j of witness b, on all n rows
__global__ __launch_bounds__(256) void check_challenge_fill_kernel(Fe* __restrict__ inst, size_t inst_bs, const Fe* __restrict__ chal,
                                                                   uint32_t col0, uint32_t n_chal, uint32_t n) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, b = blockIdx.z;
    if (row >= n) return;
    stg(inst + (size_t)b * inst_bs + (size_t)(col0 + j) * n + row, ldg(chal + (size_t)b * n_chal + j));
}

constexpr uint32_t CK_NO_PARTNER = 0xffffffffu;

// shuffle j's values of a witness, [side][width][n] canonical integers (side 0: the input expressions), start off[j]
// elements into the witness's; grid.y of the kernels below = 2 j + side, or j
struct ShufSlots {
    const DLookup* sh;
    uint32_t off[ZG_MAX_SHUFFLES];
};
__device__ __forceinline__ RowTuples shuf_side(const ShufSlots& a, const Fe* vals, uint32_t j, uint32_t side, uint32_t n, uint32_t usable) {
    const uint32_t width = a.sh[j].width;
    return RowTuples{reinterpret_cast<const uint32_t*>(vals + a.off[j] + (size_t)side * width * n), n, usable, width};
}

__global__ __launch_bounds__(256) void check_shuffle_eval_kernel(DevCircuit c, Cols cols_all, ShufSlots a, Fe* __restrict__ vals,
                                                                 size_t vals_bs, uint32_t n) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y >> 1, side = blockIdx.y & 1u, b = blockIdx.z;
    if (row >= n) return;
    const Cols cols = cols_of(cols_all, b);
    const DLookup* sf = a.sh + j;
    const zg_poly* ex = side ? sf->tables : sf->inputs;
    Fe* out = vals + (size_t)b * vals_bs + a.off[j] + (size_t)side * sf->width * n + row;
    for (uint32_t e = 0; e < sf->width; e++) stg(out + (size_t)e * n, Fr::to_raw(eval_poly(c, cols, ex[e], row)));
}

// idx: [nb][2 NS][n] row indices, row 2 j + side
__global__ __launch_bounds__(CS_NT) void check_shuffle_sort_local_kernel(uint32_t* __restrict__ idx, size_t idx_bs,
                                                                         const Fe* __restrict__ vals, size_t vals_bs, ShufSlots a,
                                                                         uint32_t n, uint32_t usable, uint32_t merge_size) {
    __shared__ uint32_t sh[CS_CH];
    const uint32_t s = blockIdx.y, b = blockIdx.z;
    const uint32_t g0 = blockIdx.x * CS_CH;
    const RowTuples t = shuf_side(a, vals + (size_t)b * vals_bs, s >> 1, s & 1u, n, usable);
    idx_sort_local(sh, idx + (size_t)b * idx_bs + (size_t)s * n + g0, t, g0, n < CS_CH ? n : CS_CH, merge_size);
}

__global__ __launch_bounds__(256) void check_shuffle_sort_global_kernel(uint32_t* __restrict__ idx, size_t idx_bs,
                                                                        const Fe* __restrict__ vals, size_t vals_bs, ShufSlots a,
                                                                        uint32_t n, uint32_t usable, uint32_t size, uint32_t stride) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    if (q >= n / 2) return;
    const RowTuples t = shuf_side(a, vals + (size_t)b * vals_bs, s >> 1, s & 1u, n, usable);
    idx_sort_global(idx + (size_t)b * idx_bs + (size_t)s * n, t, q, size, stride);
}

// Position i of the two orders: the input row there against the shuffle row there.  partner: [nb][NS][n]; the usable rows
// sort first on both sides, so every input row below `usable` is written exactly once and no other word is written.
__global__ __launch_bounds__(256) void check_shuffle_compare_kernel(ShufSlots a, const uint32_t* __restrict__ idx, size_t idx_bs,
                                                                    const Fe* __restrict__ vals, size_t vals_bs,
                                                                    uint32_t* __restrict__ partner, size_t partner_bs, uint32_t n,
                                                                    uint32_t usable) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, b = blockIdx.z;
    if (i >= usable) return;
    const uint32_t* rows = idx + (size_t)b * idx_bs + (size_t)2 * j * n;
    const uint32_t ra = rows[i], rb = rows[n + i];
    if (ra >= usable || rb >= usable) return;  // (cannot happen: the usable rows sort first)
    const Fe* v = vals + (size_t)b * vals_bs;
    const RowTuples in = shuf_side(a, v, j, 0, n, usable), sf = shuf_side(a, v, j, 1, n, usable);
    partner[(size_t)b * partner_bs + (size_t)j * n + ra] = row_tuple_cmp(in, ra, sf, rb) ? rb : CK_NO_PARTNER;
}

// the shuffles' rows of the bitmap (constraints first .. first + NS - 1) and the witness's shuffle total
__global__ __launch_bounds__(256) void check_shuffle_flag_kernel(const uint32_t* __restrict__ partner, size_t partner_bs, uint32_t n,
                                                                 uint32_t usable, unsigned long long* __restrict__ bm, uint32_t nc,
                                                                 uint32_t first, uint32_t w, uint32_t* __restrict__ totals) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, b = blockIdx.z;
    const bool bad = row < usable && partner[(size_t)b * partner_bs + (size_t)j * n + row] != CK_NO_PARTNER;
    flag_rows(bad, row, n, bm + ((size_t)b * nc + first + j) * w, totals + b);
}

// The shuffles of nb witnesses: vals [nb][vals_bs] elements, idx [nb][2 NS][n], partner [nb][NS][n] words; tot4: [nb].
static int check_shuffles(zg_ctx* ctx, const PkDev& v, const Cols& cols, uint32_t nb, Fe* vals, size_t vals_bs, uint32_t* idx,
                          uint32_t* partner, unsigned long long* bm, uint32_t nc, uint32_t w, uint32_t* tot4) {
    const uint32_t n = v.n, usable = v.usable, NS = v.NS;
    ShufSlots sl{};
    sl.sh = v.d_shuffles;
    size_t at = 0;
    for (uint32_t j = 0; j < NS; j++) {
        sl.off[j] = (uint32_t)at;
        at += (size_t)2 * v.shuffles[j].width * n;
    }
    const size_t idx_bs = (size_t)2 * NS * n, partner_bs = (size_t)NS * n;
    const double cells = (double)nb * (double)vals_bs;
    ZG_LAUNCH(ctx, "check_shuffle_eval", cells * 64, check_shuffle_eval_kernel, dim3((n + 255) / 256, 2 * NS, nb), dim3(256), 0, v.dc, cols,
              sl, vals, vals_bs, n);
    const uint32_t chunks = n <= CS_CH ? 1 : n / CS_CH;
    const dim3 gl(chunks, 2 * NS, nb), gg((n / 2 + 255) / 256, 2 * NS, nb);
    ZG_LAUNCH(ctx, "check_shuffle_sort_local", cells * 32, check_shuffle_sort_local_kernel, gl, dim3(CS_NT), 0, idx, idx_bs, vals, vals_bs,
              sl, n, usable, 0u);
    for (uint32_t size = 2 * CS_CH; size <= n; size <<= 1) {
        for (uint32_t stride = size >> 1; stride >= CS_CH; stride >>= 1)
            ZG_LAUNCH(ctx, "check_shuffle_sort_global", cells * 32, check_shuffle_sort_global_kernel, gg, dim3(256), 0, idx, idx_bs, vals,
                      vals_bs, sl, n, usable, size, stride);
        ZG_LAUNCH(ctx, "check_shuffle_sort_local", cells * 32, check_shuffle_sort_local_kernel, gl, dim3(CS_NT), 0, idx, idx_bs, vals,
                  vals_bs, sl, n, usable, size);
    }
    ZG_LAUNCH(ctx, "check_shuffle_compare", cells * 32, check_shuffle_compare_kernel, dim3((usable + 255) / 256, NS, nb), dim3(256), 0, sl,
              idx, idx_bs, vals, vals_bs, partner, partner_bs, n, usable);
    ZG_LAUNCH(ctx, "check_shuffle_flag", (double)nb * NS * n * 4, check_shuffle_flag_kernel, dim3((n + 255) / 256, NS, nb), dim3(256), 0,
              partner, partner_bs, n, usable, bm, nc, v.NG + v.NL + v.P, w, tot4);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ the permutation mapping (host)
namespace {
struct Label {
    Fe v;
    uint32_t cell;  // column * n + row
};
inline bool fe_less(const Fe& a, const Fe& b) {
    for (int i = 7; i >= 0; i--)
        if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
    return false;
}
}  // namespace

// next[c * n + r] = c' * n + r' with sigma[c][r] = delta^c' * omega^r'
static int recover_mapping(uint32_t k, uint32_t n_perm, const Fe* sigma, std::vector<uint32_t>& next) {
    const uint32_t n = 1u << k;
    const size_t cells = (size_t)n_perm * n;
    ZG_REQUIRE(cells < (1ull << 32), ZG_ERR_UNSUPPORTED, "permutation mapping: %u columns of 2^%u rows", n_perm, k);
    std::vector<Label> labels(cells);
    const Fe omega = host_domain_omega(k), delta = fr_delta();
    Fe dc = Fr::one();
    for (uint32_t c = 0; c < n_perm; c++) {
        Fe x = dc;
        for (uint32_t r = 0; r < n; r++) {
            labels[(size_t)c * n + r] = Label{x, c * n + r};
            x = Fr::mul(x, omega);
        }
        dc = Fr::mul(dc, delta);
    }
    std::sort(labels.begin(), labels.end(), [](const Label& a, const Label& b) { return fe_less(a.v, b.v); });
    next.resize(cells);
    for (size_t i = 0; i < cells; i++) {
        const Fe& v = sigma[i];
        auto it = std::lower_bound(labels.begin(), labels.end(), v, [](const Label& a, const Fe& b) { return fe_less(a.v, b); });
        ZG_REQUIRE(it != labels.end() && fe_eq(it->v, v), ZG_ERR_INVALID_ARG,
                   "permutation mapping: sigma value of column %zu, row %zu is no delta^c * omega^r (c < %u)", i / n, i % n, n_perm);
        next[i] = it->cell;
    }
    return ZG_OK;
}

// ------------------------------------------------------------------ per-key data
struct CheckKey {
    int device = 0;
    int status = ZG_OK;          // what building it came to (a key whose sigma values are no labels stays unusable)
    std::string error;
    std::vector<uint32_t> next;  // host: c * n + r -> c' * n + r'
    uint2* d_next = nullptr;     // [P][n] (column, row)
    Fe* key_sorted = nullptr;    // sorted tuples of the fixed-only tables
    LkTabs tabs{};
    TabSlots var_slots{};        // the lookups whose tables are made per witness
    uint32_t n_var = 0;
    size_t var_elems = 0;        // elements per witness of their tuples
    ~CheckKey() {
        (void)hipSetDevice(device);
        if (d_next) (void)hipFree(d_next);
        if (key_sorted) (void)hipFree(key_sorted);
    }
};

static int build_check_key(zg_ctx* ctx, const PkDev& v, CheckKey& ck) {
    const uint32_t n = v.n;
    ck.device = v.device;
    // ---- the mapping, from the sigma values the key holds in HBM
    if (v.P) {
        std::vector<Fe> sigma((size_t)v.P * n);
        ZG_HIP(hipMemcpyAsync(sigma.data(), v.sigma_val, sigma.size() * sizeof(Fe), hipMemcpyDeviceToHost, ctx->stream));
        ZG_HIP(hipStreamSynchronize(ctx->stream));
        ZG_TRY(recover_mapping(v.k, v.P, sigma.data(), ck.next));
        std::vector<uint2> packed(ck.next.size());
        for (size_t i = 0; i < packed.size(); i++) packed[i] = make_uint2(ck.next[i] / n, ck.next[i] % n);
        ZG_HIP(hipMalloc((void**)&ck.d_next, packed.size() * sizeof(uint2)));
        ZG_HIP(hipMemcpyAsync(ck.d_next, packed.data(), packed.size() * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream));
        ZG_HIP(hipStreamSynchronize(ctx->stream));
    }
    // ---- the lookups' tables: which are the key's, which a witness's
    TabSlots key_slots{};
    uint32_t n_key = 0;
    size_t key_elems = 0;
    for (uint32_t l = 0; l < v.NL; l++) {
        const size_t sz = (size_t)v.ck.lookup_width[l] * n;
        if (v.ck.table_var[l]) {
            ck.tabs.var_mask |= 1ull << l;
            ck.tabs.off[l] = (uint32_t)ck.var_elems;
            ck.var_slots.lookup[ck.n_var] = l;
            ck.var_slots.off[ck.n_var++] = (uint32_t)ck.var_elems;
            ck.var_elems += sz;
        } else {
            ck.tabs.off[l] = (uint32_t)key_elems;
            key_slots.lookup[n_key] = l;
            key_slots.off[n_key++] = (uint32_t)key_elems;
            key_elems += sz;
        }
    }
    ZG_REQUIRE(key_elems < (1ull << 32) && ck.var_elems < (1ull << 32), ZG_ERR_UNSUPPORTED, "witness check: lookup tables too large");
    if (n_key) {
        ZG_HIP(hipMalloc((void**)&ck.key_sorted, key_elems * sizeof(Fe)));
        WsScope ws(ctx);
        Fe* vals = ws.get<Fe>(key_elems);
        uint32_t* idx = ws.get<uint32_t>((size_t)n_key * n);
        if (ws.failed) return ZG_ERR_OOM;
        Cols cols{};
        cols.fixed = v.fixed_val;  // (these tables query nothing else)
        cols.log_size = v.k;
        cols.rot_scale = 1;
        ZG_TRY(prepare_tables(ctx, v.dc, cols, key_slots, n_key, 1, vals, key_elems, ck.key_sorted, key_elems, idx, n, v.usable));
        ZG_HIP(hipStreamSynchronize(ctx->stream));  // (forks on other streams read it from now on)
    }
    return ZG_OK;
}

// the key data of this prover, made on first use
static int check_key(zg_ctx* ctx, PkDev& v, std::shared_ptr<CheckKey>& out) {
    std::lock_guard<std::mutex> lock(v.ck.mu);
    if (!v.ck.key) {
        std::shared_ptr<CheckKey> ck = std::make_shared<CheckKey>();
        ck->status = build_check_key(ctx, v, *ck);
        if (ck->status != ZG_OK) ck->error = zg_last_error();
        v.ck.key = ck;
    }
    out = v.ck.key;
    if (out->status != ZG_OK) set_error("%s", out->error.c_str());
    return out->status;
}

// ------------------------------------------------------------------ the check
// What every entry shares.  nk: totals per witness -- 3 (zg_prover_check_batch*: their refusals are decided in front of
// this) or 4 (zg_prover_check_circuit*: a shuffle total, and `challenges` [count][n_chal] for the challenges' columns).
static int check_batch_impl(const char* who, zg_prover* p, size_t count, const zg_fr* const* advice_host, void* const* advice_dev,
                            const zg_fr* const* instance, size_t instance_len, const zg_fr* challenges, uint32_t nk,
                            zg_failure* failures, size_t cap, uint32_t* totals) {
    ZG_REQUIRE(p && totals, ZG_ERR_INVALID_ARG, "%s: null argument", who);
    ZG_REQUIRE(failures || cap == 0, ZG_ERR_INVALID_ARG, "%s: room for %zu failures per witness but no array", who, cap);
    zg_ctx* ctx = p->ctx;
    ZG_ENTER(ctx);
    PkDev& v = *p->pk;  // (the key: the circuit's shape, its tables, the fixed and sigma values)
    const uint32_t NS = nk == 4 ? v.NS : 0;
    // (the challenges' columns exist for every entry; only zg_prover_check_circuit* has values for them)
    const uint32_t n_chal = std::max<uint32_t>(v.NC, (uint32_t)p->challenge_phase.size());
    ZG_REQUIRE(nk != 4 || !v.NC || challenges, ZG_ERR_INVALID_ARG, "%s: the circuit has %u challenges but challenges is null", who, v.NC);
    ZG_TRY(batch_args_ok(who, "witnesses", p, count, instance, instance_len));
    if (v.IU && instance_len)
        for (size_t b = 0; b < count; b++) ZG_REQUIRE(instance[b], ZG_ERR_INVALID_ARG, "%s: instance %zu is null", who, b);
    if (p->in_flight) ZG_TRY(prover_drain(p));  // (a batch left through an error return may still read the slots)
    std::shared_ptr<CheckKey> ck;
    ZG_TRY(check_key(ctx, v, ck));

    hipStream_t st = ctx->stream;
    const uint32_t nb = (uint32_t)count, n = v.n;
    const size_t adv_bs = (size_t)v.A * n, inst_bs = (size_t)v.I * n;
    size_t shuf_bs = 0;  // a witness's shuffle values: [side][width][n] per shuffle
    for (uint32_t j = 0; j < NS; j++) shuf_bs += (size_t)2 * v.shuffles[j].width * n;
    ZG_REQUIRE(shuf_bs < (1ull << 32), ZG_ERR_UNSUPPORTED, "%s: shuffles too large", who);
    ZG_TRY(advice_into_slots(p, nb, advice_host, advice_dev));
    const uint32_t nc = v.NG + v.NL + v.P + NS, w = (n + 63) / 64;
    const bool fill_chal = nk == 4 && v.NC;
    WsScope ws(ctx);
    Fe* inst = ws.get<Fe>((size_t)nb * inst_bs);  // the prover's own instance columns belong to its proofs
    unsigned long long* bm = ws.get<unsigned long long>((size_t)nb * nc * w);
    uint32_t* d_tot = ws.get<uint32_t>((size_t)nb * 4);  // [nb][3] by kind, then [nb] shuffle totals
    Fe *var_vals = nullptr, *var_sorted = nullptr;
    uint32_t* var_idx = nullptr;
    if (ck->n_var) {
        var_vals = ws.get<Fe>((size_t)nb * ck->var_elems);
        var_sorted = ws.get<Fe>((size_t)nb * ck->var_elems);
        var_idx = ws.get<uint32_t>((size_t)nb * ck->n_var * n);
    }
    Fe *d_chal = nullptr, *shuf_vals = nullptr;
    uint32_t *shuf_idx = nullptr, *partner = nullptr;
    if (fill_chal) d_chal = ws.get<Fe>((size_t)nb * v.NC);
    if (NS) {
        shuf_vals = ws.get<Fe>((size_t)nb * shuf_bs);
        shuf_idx = ws.get<uint32_t>((size_t)nb * 2 * NS * n);
        partner = ws.get<uint32_t>((size_t)nb * NS * n);
    }
    if (ws.failed) return ZG_ERR_OOM;
    const size_t col_bytes = instance_len * 32, in_bytes = (size_t)nb * v.IU * col_bytes, chal_off = (in_bytes + 63) & ~size_t(63);
    const size_t chal_bytes = fill_chal ? (size_t)nb * v.NC * 32 : 0, tot_off = (chal_off + chal_bytes + 63) & ~size_t(63);
    ZG_TRY(pinned_reserve(ctx, tot_off + (size_t)nb * 4 * 4 + 64));
    ZG_HIP(hipMemsetAsync(d_tot, 0, (size_t)nb * 4 * 4, st));
    if (v.I) {
        ZG_HIP(hipMemsetAsync(inst, 0, (size_t)nb * inst_bs * 32, st));
        if (v.IU && instance_len) {
            for (uint32_t b = 0; b < nb; b++) memcpy((char*)ctx->pinned + (size_t)b * v.IU * col_bytes, instance[b], (size_t)v.IU * col_bytes);
            if (v.I == v.IU) {
                ZG_HIP(hipMemcpy2DAsync(inst, (size_t)n * 32, ctx->pinned, col_bytes, col_bytes, (size_t)nb * v.IU, hipMemcpyHostToDevice, st));
            } else {  // (the challenges' columns stand between one witness's instance columns and the next's)
                for (uint32_t b = 0; b < nb; b++)
                    ZG_HIP(hipMemcpy2DAsync(inst + (size_t)b * inst_bs, (size_t)n * 32, (char*)ctx->pinned + (size_t)b * v.IU * col_bytes,
                                            col_bytes, col_bytes, v.IU, hipMemcpyHostToDevice, st));
            }
        }
    }
    const dim3 blk(256);
    const uint32_t rb = (n + 255) / 256;
    const double rows = (double)nb * n;
    if (fill_chal) {
        char* h_chal = (char*)ctx->pinned + chal_off;
        for (uint32_t b = 0; b < nb; b++) memcpy(h_chal + (size_t)b * v.NC * 32, (const char*)challenges + (size_t)b * n_chal * 32, (size_t)v.NC * 32);
        ZG_HIP(hipMemcpyAsync(d_chal, h_chal, chal_bytes, hipMemcpyHostToDevice, st));
        ZG_LAUNCH(ctx, "check_challenge_fill", rows * v.NC * 32, check_challenge_fill_kernel, dim3(rb, v.NC, nb), blk, 0, inst, inst_bs, d_chal,
                  v.IU, v.NC, n);
    }
    Cols cols{};
    cols.fixed = v.fixed_val; cols.advice = p->adv_val; cols.instance = inst;
    cols.log_size = v.k; cols.rot_scale = 1;
    cols.adv_bs = adv_bs; cols.inst_bs = inst_bs;
    if (v.NG)
        ZG_LAUNCH(ctx, "check_gates", rows * (v.F + v.A + v.I) * 32, check_gates_kernel, dim3(rb, v.NG, nb), blk, 0, v.dc, cols, n, v.usable,
                  bm, nc, w, d_tot);
    if (v.NL) {
        ZG_TRY(prepare_tables(ctx, v.dc, cols, ck->var_slots, ck->n_var, nb, var_vals, ck->var_elems, var_sorted, ck->var_elems, var_idx, n,
                              v.usable));
        ZG_LAUNCH(ctx, "check_lookups", rows * v.NL * 64, check_lookups_kernel, dim3(rb, v.NL, nb), blk, 0, v.dc, cols, ck->tabs,
                  ck->key_sorted, var_sorted, ck->var_elems, n, v.usable, bm, nc, w, d_tot);
    }
    if (v.P)
        ZG_LAUNCH(ctx, "check_copies", rows * v.P * 72, check_copies_kernel, dim3(rb, v.P, nb), blk, 0, v.dc, cols, ck->d_next, n, bm, nc, w,
                  d_tot);
    if (NS) ZG_TRY(check_shuffles(ctx, v, cols, nb, shuf_vals, shuf_bs, shuf_idx, partner, bm, nc, w, d_tot + (size_t)nb * 3));
    ZG_HIP(hipGetLastError());
    uint32_t* h_tot = reinterpret_cast<uint32_t*>((char*)ctx->pinned + tot_off);
    ZG_HIP(hipMemcpyAsync(h_tot, d_tot, (size_t)nb * 4 * 4, hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    for (uint32_t b = 0; b < nb; b++) {
        memcpy(totals + (size_t)nk * b, h_tot + 3 * b, 3 * 4);
        if (nk == 4) totals[(size_t)nk * b + ZG_FAIL_SHUFFLE] = h_tot[(size_t)nb * 3 + b];
    }

    // ---- the report: only a witness with failures has its bitmap walked, constraint by constraint, row by row
    std::vector<unsigned long long> hbm;
    std::vector<uint32_t> hpart;
    const uint32_t first_shuffle = v.NG + v.NL + v.P;
    for (uint32_t b = 0; b < nb && cap; b++) {
        uint64_t total = 0;
        for (uint32_t kd = 0; kd < nk; kd++) total += totals[(size_t)nk * b + kd];
        if (!total) continue;
        hbm.resize((size_t)nc * w);
        ZG_HIP(hipMemcpyAsync(hbm.data(), bm + (size_t)b * nc * w, hbm.size() * 8, hipMemcpyDeviceToHost, st));
        if (nk == 4 && totals[(size_t)nk * b + ZG_FAIL_SHUFFLE]) {  // (whom each failing row met)
            hpart.resize((size_t)NS * n);
            ZG_HIP(hipMemcpyAsync(hpart.data(), partner + (size_t)b * NS * n, hpart.size() * 4, hipMemcpyDeviceToHost, st));
        }
        ZG_HIP(hipStreamSynchronize(st));
        zg_failure* out = failures + (size_t)b * cap;
        size_t at = 0;
        for (uint32_t ci = 0; ci < nc && at < cap; ci++) {
            const uint32_t kind = ci < v.NG ? ZG_FAIL_GATE : ci < v.NG + v.NL ? ZG_FAIL_LOOKUP : ci < first_shuffle ? ZG_FAIL_COPY : ZG_FAIL_SHUFFLE;
            const uint32_t index = kind == ZG_FAIL_GATE ? ci : kind == ZG_FAIL_LOOKUP ? ci - v.NG : kind == ZG_FAIL_COPY ? ci - v.NG - v.NL
                                                                                                                          : ci - first_shuffle;
            for (uint32_t wi = 0; wi < w && at < cap; wi++) {
                unsigned long long m = hbm[(size_t)ci * w + wi];
                while (m && at < cap) {
                    const uint32_t row = wi * 64 + (uint32_t)__builtin_ctzll(m);
                    m &= m - 1;
                    zg_failure f{kind, index, row, 0, 0};
                    if (kind == ZG_FAIL_COPY) {
                        const uint32_t to = ck->next[(size_t)index * n + row];
                        f.other_index = to / n;
                        f.other_row = to % n;
                    } else if (kind == ZG_FAIL_SHUFFLE) {
                        f.other_row = hpart[(size_t)index * n + row];
                    }
                    out[at++] = f;
                }
            }
        }
    }
    return ZG_OK;
}

// zg_prover_check_batch* and zg_prover_check_images know three kinds and no challenge values
static int check_three_kinds(const zg_prover* p) {
    ZG_REQUIRE(!p || !p->phased(), ZG_ERR_UNSUPPORTED, "zg_prover_check: not for a circuit with challenges or advice phases (the check knows no challenge values)");
    ZG_REQUIRE(!p || p->pk->NS == 0, ZG_ERR_UNSUPPORTED, "zg_prover_check: not for a circuit with shuffles (the totals have no place for a shuffle's)");
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_prover_check_batch(zg_prover* p, size_t count, const zg_fr* const* advice, const zg_fr* const* instance, size_t instance_len,
                          zg_failure* failures, size_t cap, uint32_t* totals) {
    ZG_TRY(check_three_kinds(p));
    return check_batch_impl("zg_prover_check", p, count, advice, nullptr, instance, instance_len, nullptr, 3, failures, cap, totals);
}

int zg_prover_check_batch_dev(zg_prover* p, size_t count, void* const* d_advice, const zg_fr* const* instance, size_t instance_len,
                              zg_failure* failures, size_t cap, uint32_t* totals) {
    ZG_TRY(check_three_kinds(p));
    return check_batch_impl("zg_prover_check", p, count, nullptr, d_advice, instance, instance_len, nullptr, 3, failures, cap, totals);
}

int zg_prover_check_circuit(zg_prover* p, size_t count, const zg_fr* const* advice, const zg_fr* const* instance, size_t instance_len,
                            const zg_fr* challenges, zg_failure* failures, size_t cap, uint32_t* totals) {
    return check_batch_impl("zg_prover_check_circuit", p, count, advice, nullptr, instance, instance_len, challenges, 4, failures, cap, totals);
}

int zg_prover_check_circuit_dev(zg_prover* p, size_t count, void* const* d_advice, const zg_fr* const* instance, size_t instance_len,
                                const zg_fr* challenges, zg_failure* failures, size_t cap, uint32_t* totals) {
    return check_batch_impl("zg_prover_check_circuit", p, count, nullptr, d_advice, instance, instance_len, challenges, 4, failures, cap,
                            totals);
}

int zg_permutation_mapping(uint32_t k, uint32_t n_perm, const zg_fr* sigma_values, uint32_t* next_col, uint32_t* next_row) {
    ZG_REQUIRE(k >= 1 && k <= FR_S, ZG_ERR_INVALID_ARG, "zg_permutation_mapping: k=%u", k);
    ZG_REQUIRE(n_perm == 0 || (sigma_values && next_col && next_row), ZG_ERR_INVALID_ARG, "zg_permutation_mapping: null argument");
    if (!n_perm) return ZG_OK;
    const uint32_t n = 1u << k;
    std::vector<Fe> sigma((size_t)n_perm * n);  // (the caller's array need not have Fe's alignment)
    memcpy(sigma.data(), sigma_values, sigma.size() * sizeof(Fe));
    std::vector<uint32_t> next;
    ZG_TRY(recover_mapping(k, n_perm, sigma.data(), next));
    for (size_t i = 0; i < next.size(); i++) {
        next_col[i] = next[i] / n;
        next_row[i] = next[i] % n;
    }
    return ZG_OK;
}

int zg_permutation_sigma(zg_ctx* ctx, uint32_t k, uint32_t n_perm, const uint32_t* next_col, const uint32_t* next_row,
                         zg_fr* sigma_out) {
    ZG_REQUIRE(ctx, ZG_ERR_INVALID_ARG, "zg_permutation_sigma: ctx is null");
    ZG_REQUIRE(k >= 1 && k <= 22, ZG_ERR_INVALID_ARG, "zg_permutation_sigma: k=%u", k);
    ZG_REQUIRE(n_perm == 0 || (next_col && next_row && sigma_out), ZG_ERR_INVALID_ARG, "zg_permutation_sigma: null argument");
    if (!n_perm) return ZG_OK;
    const uint32_t n = 1u << k;
    ZG_REQUIRE((uint64_t)n_perm * n < (1ull << 32) - 1, ZG_ERR_UNSUPPORTED, "zg_permutation_sigma: %u columns of 2^%u rows", n_perm, k);
    const uint32_t cells = n_perm * n;
    ZG_ENTER(ctx);
    hipStream_t st = ctx->stream;
    Fe* tw = nullptr;
    ZG_TRY(get_twiddles(ctx, k, host_domain_omega(k), &tw));
    std::vector<Fe> dpow(n_perm);
    Fe d = Fr::one();
    for (uint32_t c = 0; c < n_perm; c++) {
        dpow[c] = d;
        d = Fr::mul(d, fr_delta());
    }
    WsScope ws(ctx);
    uint32_t* d_next = ws.get<uint32_t>((size_t)2 * cells + 1);  // columns, rows, the error word
    Fe* d_dpow = ws.get<Fe>(n_perm);
    Fe* d_sigma = ws.get<Fe>(cells);
    if (ws.failed) return ZG_ERR_OOM;
    uint32_t* d_bad = d_next + (size_t)2 * cells;
    uint32_t bad = 0xffffffffu;
    ZG_HIP(hipMemcpyAsync(d_next, next_col, (size_t)cells * 4, hipMemcpyHostToDevice, st));
    ZG_HIP(hipMemcpyAsync(d_next + cells, next_row, (size_t)cells * 4, hipMemcpyHostToDevice, st));
    ZG_HIP(hipMemcpyAsync(d_bad, &bad, 4, hipMemcpyHostToDevice, st));
    ZG_HIP(hipMemcpyAsync(d_dpow, dpow.data(), (size_t)n_perm * sizeof(Fe), hipMemcpyHostToDevice, st));
    ZG_LAUNCH(ctx, "permutation_sigma", (double)cells * 40.0, permutation_sigma_kernel, dim3((cells + 255) / 256), dim3(256), 0, d_next,
              d_next + cells, tw, d_dpow, n, n_perm, cells, d_sigma, d_bad);
    ZG_HIP(hipGetLastError());
    ZG_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));  // (the host arrays above are read until here)
    ZG_REQUIRE(bad == 0xffffffffu, ZG_ERR_INVALID_ARG, "zg_permutation_sigma: column %u, row %u maps to (%u, %u), outside %u columns of %u rows",
               bad / n, bad % n, next_col[bad], next_row[bad], n_perm, n);
    ZG_HIP(hipMemcpy(sigma_out, d_sigma, (size_t)cells * sizeof(Fe), hipMemcpyDeviceToHost));
    return ZG_OK;
}

}  // extern "C"
