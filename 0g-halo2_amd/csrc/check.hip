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
#include "prover.h"
#include "poly_eval.h"

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

__device__ __forceinline__ void idx_cmpx(uint32_t* sh, const TupView& t, uint32_t i, uint32_t j, bool ascending) {
    const uint32_t a = sh[i], b = sh[j];
    if (tup_greater(t, a, b) == ascending) {
        sh[i] = b;
        sh[j] = a;
    }
}

// The bitonic network of sort.hip over ROW INDICES (the keys stay where they are; a comparison gathers them).
// merge_size = 0: the indices are created here (idx[i] = i) and every chunk becomes a sorted run, direction alternating
// with bit CS_CH of its position; otherwise the strides below CS_CH of merge level `merge_size`.
__global__ __launch_bounds__(CS_NT) void check_sort_local_kernel(uint32_t* __restrict__ idx, size_t idx_bs, const Fe* __restrict__ vals,
                                                                 size_t vals_bs, DevCircuit c, TabSlots sl, uint32_t n,
                                                                 uint32_t usable, uint32_t merge_size) {
    __shared__ uint32_t sh[CS_CH];
    const uint32_t s = blockIdx.y, b = blockIdx.z;
    const uint32_t g0 = blockIdx.x * CS_CH;
    const uint32_t len = n < CS_CH ? n : CS_CH;
    uint32_t* base = idx + (size_t)b * idx_bs + (size_t)s * n + g0;
    const TupView t{vals + (size_t)b * vals_bs + sl.off[s], n, usable, c.lookups[sl.lookup[s]].width};
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

// one compare-exchange pass with stride >= CS_CH
__global__ __launch_bounds__(256) void check_sort_global_kernel(uint32_t* __restrict__ idx, size_t idx_bs, const Fe* __restrict__ vals,
                                                                size_t vals_bs, DevCircuit c, TabSlots sl, uint32_t n, uint32_t usable,
                                                                uint32_t size, uint32_t stride) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    if (q >= n / 2) return;
    uint32_t* base = idx + (size_t)b * idx_bs + (size_t)s * n;
    const TupView t{vals + (size_t)b * vals_bs + sl.off[s], n, usable, c.lookups[sl.lookup[s]].width};
    const uint32_t i = 2 * q - (q & (stride - 1)), j = i + stride;
    const uint32_t a = base[i], bb = base[j];
    if (tup_greater(t, a, bb) == ((i & size) == 0)) {
        base[i] = bb;
        base[j] = a;
    }
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
static int check_batch_impl(zg_prover* p, size_t count, const zg_fr* const* advice_host, void* const* advice_dev,
                            const zg_fr* const* instance, size_t instance_len, zg_failure* failures, size_t cap, uint32_t* totals) {
    ZG_REQUIRE(p && totals, ZG_ERR_INVALID_ARG, "zg_prover_check: null argument");
    ZG_REQUIRE(failures || cap == 0, ZG_ERR_INVALID_ARG, "zg_prover_check: room for %zu failures per witness but no array", cap);
    zg_ctx* ctx = p->ctx;
    ZG_ENTER(ctx);
    PkDev& v = *p->pk;  // (the key: the circuit's shape, its tables, the fixed and sigma values)
    ZG_REQUIRE(!p->phased(), ZG_ERR_UNSUPPORTED, "zg_prover_check: not for a circuit with challenges or advice phases (the check knows no challenge values)");
    ZG_REQUIRE(p->pk->NS == 0, ZG_ERR_UNSUPPORTED, "zg_prover_check: not for a circuit with shuffles (the totals have no place for a shuffle's)");
    ZG_TRY(batch_args_ok("zg_prover_check", "witnesses", p, count, instance, instance_len));
    if (v.I && instance_len)
        for (size_t b = 0; b < count; b++) ZG_REQUIRE(instance[b], ZG_ERR_INVALID_ARG, "zg_prover_check: instance %zu is null", b);
    if (p->in_flight) ZG_TRY(prover_drain(p));  // (a batch left through an error return may still read the slots)
    std::shared_ptr<CheckKey> ck;
    ZG_TRY(check_key(ctx, v, ck));

    hipStream_t st = ctx->stream;
    const uint32_t nb = (uint32_t)count, n = v.n;
    const size_t adv_bs = (size_t)v.A * n, inst_bs = (size_t)v.I * n;
    ZG_TRY(advice_into_slots(p, nb, advice_host, advice_dev));
    const uint32_t nc = v.NG + v.NL + v.P, w = (n + 63) / 64;
    WsScope ws(ctx);
    Fe* inst = ws.get<Fe>((size_t)nb * inst_bs);  // the prover's own instance columns belong to its proofs
    unsigned long long* bm = ws.get<unsigned long long>((size_t)nb * nc * w);
    uint32_t* d_tot = ws.get<uint32_t>((size_t)nb * 3);
    Fe *var_vals = nullptr, *var_sorted = nullptr;
    uint32_t* var_idx = nullptr;
    if (ck->n_var) {
        var_vals = ws.get<Fe>((size_t)nb * ck->var_elems);
        var_sorted = ws.get<Fe>((size_t)nb * ck->var_elems);
        var_idx = ws.get<uint32_t>((size_t)nb * ck->n_var * n);
    }
    if (ws.failed) return ZG_ERR_OOM;
    const size_t in_bytes = (size_t)nb * v.I * instance_len * 32, tot_off = (in_bytes + 63) & ~size_t(63);
    ZG_TRY(pinned_reserve(ctx, tot_off + (size_t)nb * 3 * 4 + 64));
    ZG_HIP(hipMemsetAsync(d_tot, 0, (size_t)nb * 3 * 4, st));
    if (v.I) {
        ZG_HIP(hipMemsetAsync(inst, 0, (size_t)nb * inst_bs * 32, st));
        if (instance_len) {
            for (uint32_t b = 0; b < nb; b++)
                memcpy((char*)ctx->pinned + (size_t)b * v.I * instance_len * 32, instance[b], (size_t)v.I * instance_len * 32);
            ZG_HIP(hipMemcpy2DAsync(inst, (size_t)n * 32, ctx->pinned, instance_len * 32, instance_len * 32, (size_t)nb * v.I,
                                    hipMemcpyHostToDevice, st));
        }
    }
    Cols cols{};
    cols.fixed = v.fixed_val; cols.advice = p->adv_val; cols.instance = inst;
    cols.log_size = v.k; cols.rot_scale = 1;
    cols.adv_bs = adv_bs; cols.inst_bs = inst_bs;
    const dim3 blk(256);
    const uint32_t rb = (n + 255) / 256;
    const double rows = (double)nb * n;
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
    ZG_HIP(hipGetLastError());
    uint32_t* h_tot = reinterpret_cast<uint32_t*>((char*)ctx->pinned + tot_off);
    ZG_HIP(hipMemcpyAsync(h_tot, d_tot, (size_t)nb * 3 * 4, hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    memcpy(totals, h_tot, (size_t)nb * 3 * 4);

    // ---- the report: only a witness with failures has its bitmap walked, constraint by constraint, row by row
    std::vector<unsigned long long> hbm;
    for (uint32_t b = 0; b < nb && cap; b++) {
        const uint64_t total = (uint64_t)totals[3 * b] + totals[3 * b + 1] + totals[3 * b + 2];
        if (!total) continue;
        hbm.resize((size_t)nc * w);
        ZG_HIP(hipMemcpyAsync(hbm.data(), bm + (size_t)b * nc * w, hbm.size() * 8, hipMemcpyDeviceToHost, st));
        ZG_HIP(hipStreamSynchronize(st));
        zg_failure* out = failures + (size_t)b * cap;
        size_t at = 0;
        for (uint32_t ci = 0; ci < nc && at < cap; ci++) {
            const uint32_t kind = ci < v.NG ? ZG_FAIL_GATE : ci < v.NG + v.NL ? ZG_FAIL_LOOKUP : ZG_FAIL_COPY;
            const uint32_t index = kind == ZG_FAIL_GATE ? ci : kind == ZG_FAIL_LOOKUP ? ci - v.NG : ci - v.NG - v.NL;
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
                    }
                    out[at++] = f;
                }
            }
        }
    }
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" {

int zg_prover_check_batch(zg_prover* p, size_t count, const zg_fr* const* advice, const zg_fr* const* instance, size_t instance_len,
                          zg_failure* failures, size_t cap, uint32_t* totals) {
    return check_batch_impl(p, count, advice, nullptr, instance, instance_len, failures, cap, totals);
}

int zg_prover_check_batch_dev(zg_prover* p, size_t count, void* const* d_advice, const zg_fr* const* instance, size_t instance_len,
                              zg_failure* failures, size_t cap, uint32_t* totals) {
    return check_batch_impl(p, count, nullptr, d_advice, instance, instance_len, failures, cap, totals);
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
