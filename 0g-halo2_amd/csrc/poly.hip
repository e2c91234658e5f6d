// Polynomial-side kernels of create_proof for gfx950: blinding, lookup compression, grand products
// (lookup::prover::commit_product, permutation::prover::commit), Evaluator::evaluate_h, eval_polynomial,
// the GWC linear combinations and kate_division (halo2_proofs v2023_04_20 src/plonk/{evaluation,
// lookup/prover, permutation/prover, vanishing/prover}.rs, src/poly/kzg/multiopen/gwc/prover.rs,
// src/arithmetic.rs; reached from /root/reference/src/wnn.rs:242-259).
//
// All of it is row-parallel 254-bit modular arithmetic over HBM-resident columns: one lane per row,
// coalesced 32-B loads, wave-uniform circuit tables read through the scalar cache.  The two sequential
// recurrences upstream runs on one core -- the running products z[i+1] = z[i]*num/den and the
// synthetic division by (X - z) -- become block-level scans (1024 lanes x a strip each).
#include "poly.h"
#include "poly_eval.h"
#include "field9.h"

namespace zg {

// ------------------------------------------------------------------ blinding scalars
// rand_fr(key, tag, index): ChaCha20 (RFC 7539: 32-byte key, 32-bit block counter, 96-bit nonce) keystream with
// nonce = (tag, index_lo, index_hi) and block counter = attempt; a 64-byte block offers two 254-bit candidates
// (words 0-7, then 8-15, top word masked to 30 bits); the first one below r is taken.  Upstream draws these
// scalars from OsRng (/root/reference/src/wnn.rs:256): a caller that passes 32 fresh random bytes per proof gets
// 256-bit keyed blinding; the test checker restates the same function for byte parity.
__host__ __device__ __forceinline__ uint32_t rotl32(uint32_t x, int sft) { return (x << sft) | (x >> (32 - sft)); }
#define ZG_QR(a, b, c, d)                       \
    do {                                        \
        a += b; d ^= a; d = rotl32(d, 16);      \
        c += d; b ^= c; b = rotl32(b, 12);      \
        a += b; d ^= a; d = rotl32(d, 8);       \
        c += d; b ^= c; b = rotl32(b, 7);       \
    } while (0)

__host__ __device__ inline Fe rand_fr(const uint32_t* key, uint32_t tag, uint64_t index) {
    Fe v;
    for (uint32_t attempt = 0;; attempt++) {
        uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
        uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3], x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
        uint32_t x12 = attempt, x13 = tag, x14 = (uint32_t)index, x15 = (uint32_t)(index >> 32);
        for (int r = 0; r < 10; r++) {
            ZG_QR(x0, x4, x8, x12);
            ZG_QR(x1, x5, x9, x13);
            ZG_QR(x2, x6, x10, x14);
            ZG_QR(x3, x7, x11, x15);
            ZG_QR(x0, x5, x10, x15);
            ZG_QR(x1, x6, x11, x12);
            ZG_QR(x2, x7, x8, x13);
            ZG_QR(x3, x4, x9, x14);
        }
        for (int half = 0; half < 2; half++) {
            if (half == 0) {
                v.l[0] = x0 + 0x61707865u; v.l[1] = x1 + 0x3320646eu; v.l[2] = x2 + 0x79622d32u; v.l[3] = x3 + 0x6b206574u;
                v.l[4] = x4 + key[0]; v.l[5] = x5 + key[1]; v.l[6] = x6 + key[2]; v.l[7] = x7 + key[3];
            } else {
                v.l[0] = x8 + key[4]; v.l[1] = x9 + key[5]; v.l[2] = x10 + key[6]; v.l[3] = x11 + key[7];
                v.l[4] = x12 + attempt; v.l[5] = x13 + tag; v.l[6] = x14 + (uint32_t)index; v.l[7] = x15 + (uint32_t)(index >> 32);
            }
            v.l[7] &= 0x3fffffffu;
            bool lt = false;
            for (int i = 7; i >= 0; i--) {
                uint32_t p = FrParams::p(i);
                if (v.l[i] < p) { lt = true; break; }
                if (v.l[i] > p) break;
            }
            if (lt) return Fr::from_raw(v);
        }
    }
}
Fe rand_fr_host(const uint32_t* key, uint32_t tag, uint64_t index) { return rand_fr(key, tag, index); }

// proof b = blockIdx.y: columns [0, ncols0) draw from tag0 (index c * nrows + j), columns [ncols0, ncols) from tag1
// (index restarts)
__global__ void blind_rows_kernel(const ProofConst* __restrict__ pc, Fe* base, size_t base_bs, size_t col_stride,
                                  uint32_t ncols, uint32_t row0, uint32_t nrows, uint32_t tag0, uint32_t ncols0, uint32_t tag1) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = blockIdx.y;
    if (t >= ncols * nrows) return;
    uint32_t c = t / nrows, j = t % nrows;
    const bool second = c >= ncols0;
    stg(base + (size_t)b * base_bs + (size_t)c * col_stride + row0 + j,
        rand_fr(pc[b].key, second ? tag1 : tag0, (uint64_t)(second ? c - ncols0 : c) * nrows + j));
}

int poly_blind_rows2(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, Fe* base, size_t base_bs, size_t col_stride,
                     uint32_t ncols0, uint32_t tag0, uint32_t ncols1, uint32_t tag1, uint32_t row0, uint32_t nrows) {
    uint32_t total = (ncols0 + ncols1) * nrows;
    if (total == 0 || nb == 0) return ZG_OK;
    ZG_LAUNCH(ctx, "blind_rows", 0, blind_rows_kernel, dim3((total + 63) / 64, nb), dim3(64), 0, pc, base, base_bs, col_stride,
              ncols0 + ncols1, row0, nrows, tag0, ncols0, tag1);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

struct RandKey {  // a ChaCha20 key passed by value in kernel arguments
    uint32_t w[8];
};
__global__ void rand_fill_kernel(RandKey key, uint32_t tag, Fe* out, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) stg(out + i, rand_fr(key.w, tag, i));
}
int poly_rand_fill(zg_ctx* ctx, const uint32_t key[8], uint32_t tag, Fe* out, uint32_t count) {
    if (count == 0) return ZG_OK;
    RandKey rk;
    memcpy(rk.w, key, sizeof(rk.w));
    ZG_LAUNCH(ctx, "rand_fill", (double)count * 32, rand_fill_kernel, dim3((count + 255) / 256), dim3(256), 0, rk, tag, out, count);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// The two draws a proof starts with, in one launch: the vanishing argument's random polynomial (n values,
// written to out and out2) and the blinding rows of the advice columns.  Proof b = blockIdx.y.
__global__ void random_and_blind_kernel(const ProofConst* __restrict__ pc, Fe* out, size_t out_bs, Fe* out2, size_t out2_bs,
                                        uint32_t n, uint32_t tag, Fe* base, size_t base_bs, size_t col_stride, uint32_t ncols,
                                        uint32_t row0, uint32_t nrows, uint32_t blind_tag) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = blockIdx.y;
    if (i < n) {
        const Fe v = rand_fr(pc[b].key, tag, i);
        stg(out + (size_t)b * out_bs + i, v);
        if (out2) stg(out2 + (size_t)b * out2_bs + i, v);
        return;
    }
    i -= n;
    if (i >= ncols * nrows) return;
    const uint32_t c = i / nrows, j = i % nrows;
    stg(base + (size_t)b * base_bs + (size_t)c * col_stride + row0 + j, rand_fr(pc[b].key, blind_tag, (uint64_t)c * nrows + j));
}
int poly_random_and_blind(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, Fe* out, size_t out_bs, Fe* out2, size_t out2_bs,
                          uint32_t n, uint32_t tag, Fe* base, size_t base_bs, size_t col_stride, uint32_t ncols,
                          uint32_t row0, uint32_t nrows, uint32_t blind_tag) {
    const uint32_t total = n + ncols * nrows;
    if (nb == 0) return ZG_OK;
    ZG_LAUNCH(ctx, "random_poly", (double)nb * n * 32, random_and_blind_kernel, dim3((total + 255) / 256, nb), dim3(256), 0, pc,
              out, out_bs, out2, out2_bs, n, tag, base, base_bs, col_stride, ncols, row0, nrows, blind_tag);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// lookup::Argument::commit_permuted `compress_expressions`: theta-fold of the input / table tuples
// raw_in / raw_tab (optional): the same values as canonical integers -- the sort keys of permute_expression_pair --
// with the all-ones sentinel on the rows from `usable` on (sorts last; real keys are < r < 2^254)
__global__ __launch_bounds__(256) void lookup_compress_kernel(DevCircuit c, Cols cols_all, const ProofConst* __restrict__ pc,
                                                              Fe* cin, Fe* ctab, uint32_t n, Fe* raw_in, Fe* raw_tab,
                                                              uint32_t usable) {
    uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = blockIdx.z;
    uint32_t l = blockIdx.y;
    if (row >= n) return;
    const Cols cols = cols_of(cols_all, b);
    const Fe theta = pc[b].theta;
    const DLookup* lk = c.lookups + l;
    l += b * c.n_lookups;  // (outputs: lookup l of proof b)
    Fe ai = fe_zero(), ti = fe_zero();
    for (uint32_t e = 0; e < lk->width; e++) {  // (the first expression enters as it is: evaluate_h9_kernel's `compress`)
        const Fe in = eval_poly(c, cols, lk->inputs[e], row), tb = eval_poly(c, cols, lk->tables[e], row);
        ai = e ? Fr::add(Fr::mul(ai, theta), in) : in;
        ti = e ? Fr::add(Fr::mul(ti, theta), tb) : tb;
    }
    stg(cin + (size_t)l * n + row, ai);
    stg(ctab + (size_t)l * n + row, ti);
    if (raw_in) {
        Fe ra, rt;
        if (row < usable) {
            ra = Fr::to_raw(ai);
            rt = Fr::to_raw(ti);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) ra.l[j] = rt.l[j] = 0xffffffffu;
        }
        stg(raw_in + (size_t)l * n + row, ra);
        stg(raw_tab + (size_t)l * n + row, rt);
    }
}

int poly_lookup_compress(zg_ctx* ctx, const DevCircuit& c, const Cols& cols, const ProofConst* pc, uint32_t nb, Fe* cin,
                         Fe* ctab, uint32_t n, Fe* raw_in, Fe* raw_tab, uint32_t usable) {
    if (c.n_lookups == 0 || nb == 0) return ZG_OK;
    ZG_LAUNCH(ctx, "lookup_compress", (double)nb * c.n_lookups * n * 64, lookup_compress_kernel,
              dim3((n + 255) / 256, c.n_lookups, nb), dim3(256), 0, c, cols, pc, cin, ctab, n, raw_in, raw_tab, usable);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

__global__ void to_raw_kernel(const Fe* in, Fe* out, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) stg(out + i, Fr::to_raw(ldg(in + i)));
}
__global__ void from_raw_kernel(const Fe* in, Fe* out, size_t count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) stg(out + i, Fr::from_raw(ldg(in + i)));
}
// rows of `len` elements: dst[r*dst_stride + i] = from_raw(src[r*src_stride + i])
__global__ void from_raw_rows_kernel(const Fe* src, size_t src_stride, Fe* dst, size_t dst_stride, uint32_t len) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (i < len) stg(dst + (size_t)r * dst_stride + i, Fr::from_raw(ldg(src + (size_t)r * src_stride + i)));
}
int poly_from_raw_rows(zg_ctx* ctx, const Fe* src, size_t src_stride, Fe* dst, size_t dst_stride, uint32_t rows,
                       uint32_t len) {
    if (!rows || !len) return ZG_OK;
    ZG_LAUNCH(ctx, "from_raw", (double)rows * len * 64, from_raw_rows_kernel, dim3((len + 255) / 256, rows), dim3(256), 0, src,
              src_stride, dst, dst_stride, len);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// lookup commit_permuted's last step in one launch: perm[2l] = a'_l, perm[2l+1] = s'_l (Montgomery form) on
// the usable rows [0, usable), blinding scalars on the rows after them (tag_in / tag_tab, index = l * nblind + j)
__global__ __launch_bounds__(256) void permuted_finish_kernel(const ProofConst* __restrict__ pc, const Fe* __restrict__ raw_in,
                                                              const Fe* __restrict__ raw_tab, Fe* __restrict__ perm, size_t perm_bs,
                                                              uint32_t n, uint32_t usable, uint32_t nblind, uint32_t tag_in,
                                                              uint32_t tag_tab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y, b = blockIdx.z;
    if (i >= usable + nblind) return;
    Fe* a = perm + (size_t)b * perm_bs + (size_t)(2 * l) * n;
    Fe* t = a + n;
    const size_t src = (size_t)(b * gridDim.y + l) * n;  // (raw rows: lookup l of proof b)
    if (i < usable) {
        stg(a + i, Fr::from_raw(ldg(raw_in + src + i)));
        stg(t + i, Fr::from_raw(ldg(raw_tab + src + i)));
    } else {
        const uint64_t idx = (uint64_t)l * nblind + (i - usable);
        stg(a + i, rand_fr(pc[b].key, tag_in, idx));
        stg(t + i, rand_fr(pc[b].key, tag_tab, idx));
    }
}
int poly_permuted_finish(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, const Fe* raw_in, const Fe* raw_tab, Fe* perm,
                         size_t perm_bs, uint32_t n, uint32_t usable, uint32_t nblind, uint32_t n_lookups, uint32_t tag_in,
                         uint32_t tag_tab) {
    if (!n_lookups || !nb) return ZG_OK;
    ZG_REQUIRE(usable + nblind <= n, ZG_ERR_INVALID_ARG, "poly_permuted_finish: %u + %u rows of %u", usable, nblind, n);
    ZG_LAUNCH(ctx, "permuted_finish", (double)nb * n_lookups * n * 128, permuted_finish_kernel,
              dim3((usable + nblind + 255) / 256, n_lookups, nb), dim3(256), 0, pc, raw_in, raw_tab, perm, perm_bs, n, usable,
              nblind, tag_in, tag_tab);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int poly_to_raw(zg_ctx* ctx, const Fe* in, Fe* out, size_t count) {
    if (!count) return ZG_OK;
    ZG_LAUNCH(ctx, "to_raw", (double)count * 64, to_raw_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, in, out, count);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}
int poly_from_raw(zg_ctx* ctx, const Fe* in, Fe* out, size_t count) {
    if (!count) return ZG_OK;
    ZG_LAUNCH(ctx, "from_raw", (double)count * 64, from_raw_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, in, out, count);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ grand-product terms
// lookup commit_product: den = (a' + beta)(s' + gamma), num = (A + beta)(S + gamma)
// (lookup l = blockIdx.y of proof b = blockIdx.z: compressed columns at (b * n_lookups + l) * n, permuted columns at
//  b * perm_bs + l * perm_stride, outputs at product (b * per + first + l) * n)
__global__ __launch_bounds__(256) void lookup_terms_kernel(const ProofConst* __restrict__ pc, const Fe* cin, const Fe* ctab,
                                                           const Fe* pin, const Fe* ptab, size_t perm_stride, size_t perm_bs,
                                                           Fe* num, Fe* den, uint32_t per, uint32_t first, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t l = blockIdx.y, b = blockIdx.z;
    if (i >= n) return;
    const Fe beta = pc[b].beta, gamma = pc[b].gamma;
    const size_t ci = (size_t)(b * gridDim.y + l) * n + i, po = (size_t)b * perm_bs + (size_t)l * perm_stride + i;
    const size_t o = (size_t)(b * per + first + l) * n + i;
    stg(den + o, Fr::mul(Fr::add(ldg(pin + po), beta), Fr::add(ldg(ptab + po), gamma)));
    stg(num + o, Fr::mul(Fr::add(ldg(cin + ci), beta), Fr::add(ldg(ctab + ci), gamma)));
}

int poly_lookup_terms(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, const Fe* cin, const Fe* ctab, const Fe* pin,
                      const Fe* ptab, size_t perm_stride, size_t perm_bs, Fe* num, Fe* den, uint32_t per, uint32_t first,
                      uint32_t n, uint32_t n_lookups) {
    if (!n_lookups || !nb) return ZG_OK;
    ZG_LAUNCH(ctx, "lookup_terms", (double)nb * n_lookups * n * 192, lookup_terms_kernel, dim3((n + 255) / 256, n_lookups, nb),
              dim3(256), 0, pc, cin, ctab, pin, ptab, perm_stride, perm_bs, num, den, per, first, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// shuffle commit_product: num = a + gamma, den = s + gamma, a and s the theta-folds of the input and the shuffle tuple
// (shuffle j = blockIdx.y of proof b = blockIdx.z, outputs at product (b * ns + j) * n: poly_grand_product's batch layout)
__global__ __launch_bounds__(256) void shuffle_terms_kernel(DevCircuit c, const DLookup* __restrict__ shuffles, Cols cols_all,
                                                            const ProofConst* __restrict__ pc, Fe* num, Fe* den, uint32_t n) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = blockIdx.y, b = blockIdx.z;
    if (row >= n) return;
    const Cols cols = cols_of(cols_all, b);
    const Fe theta = pc[b].theta, gamma = pc[b].gamma;
    const DLookup* sf = shuffles + j;
    Fe ai = fe_zero(), si = fe_zero();
    for (uint32_t e = 0; e < sf->width; e++) {  // (the first expression enters as it is, as the lookups' does)
        const Fe in = eval_poly(c, cols, sf->inputs[e], row), sh = eval_poly(c, cols, sf->tables[e], row);
        ai = e ? Fr::add(Fr::mul(ai, theta), in) : in;
        si = e ? Fr::add(Fr::mul(si, theta), sh) : sh;
    }
    const size_t o = (size_t)(b * gridDim.y + j) * n + row;
    stg(num + o, Fr::add(ai, gamma));
    stg(den + o, Fr::add(si, gamma));
}

int poly_shuffle_terms(zg_ctx* ctx, const DevCircuit& c, const DLookup* shuffles, uint32_t ns, const Cols& cols, const ProofConst* pc,
                       uint32_t nb, Fe* num, Fe* den, uint32_t n) {
    if (!ns || !nb) return ZG_OK;
    ZG_REQUIRE(shuffles && pc && num && den, ZG_ERR_INVALID_ARG, "shuffle_terms: null argument");
    ZG_LAUNCH(ctx, "shuffle_terms", (double)nb * ns * n * 128, shuffle_terms_kernel, dim3((n + 255) / 256, ns, nb), dim3(256), 0, c,
              shuffles, cols, pc, num, den, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// permutation commit, one set per blockIdx.y:
//   den = prod_c (v_c + beta*sigma_c + gamma),  num = prod_c (v_c + delta^c * omega^i * beta + gamma)
// (set0: the column set blockIdx.y = 0 stands for -- the stand-alone entry asks for ONE set, written as product 0)
__global__ __launch_bounds__(256) void perm_terms_kernel(DevCircuit c, Cols cols_all, const ProofConst* __restrict__ pc,
                                                         const Fe* sigma_val, const Fe* omega_tw, Fe* num, Fe* den,
                                                         uint32_t per, uint32_t n, uint32_t set0) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s = blockIdx.y + set0;
    const uint32_t b = blockIdx.z;
    if (i >= n) return;
    const Cols cols = cols_of(cols_all, b);
    const Fe beta = pc[b].beta, gamma = pc[b].gamma;
    uint32_t c0 = s * c.chunk, c1 = c0 + c.chunk;
    if (c1 > c.n_perm) c1 = c.n_perm;
    Fe d = Fr::one(), m = Fr::one();
    Fe dw = Fr::mul(Fr::mul(Fr::pow_u64(fr_delta(), c0), ldg(omega_tw + i)), beta);  // delta^c omega^i beta
    for (uint32_t col = c0; col < c1; col++) {
        const zg_query q = c.perm_cols[col];
        const Fe* base = q.kind == ZG_FIXED ? cols.fixed : q.kind == ZG_ADVICE ? cols.advice : cols.instance;
        Fe v = ldg(base + ((size_t)q.column << cols.log_size) + i);
        Fe sg = ldg(sigma_val + (size_t)col * n + i);
        d = Fr::mul(d, Fr::add(Fr::add(Fr::mul(beta, sg), gamma), v));
        m = Fr::mul(m, Fr::add(Fr::add(dw, gamma), v));
        dw = Fr::mul(dw, fr_delta());
    }
    stg(den + (size_t)(b * per + blockIdx.y) * n + i, d);
    stg(num + (size_t)(b * per + blockIdx.y) * n + i, m);
}

int poly_perm_terms(zg_ctx* ctx, const DevCircuit& c, const Cols& cols, const ProofConst* pc, uint32_t nb,
                    const Fe* sigma_val, const Fe* omega_tw, Fe* num, Fe* den, uint32_t per, uint32_t n, int only_set) {
    if (!c.n_sets || !nb) return ZG_OK;
    const uint32_t sets = only_set < 0 ? c.n_sets : 1u, set0 = only_set < 0 ? 0u : (uint32_t)only_set;
    ZG_LAUNCH(ctx, "perm_terms", nb * ((double)c.n_perm * n * 64 + (double)c.n_sets * n * 64), perm_terms_kernel,
              dim3((n + 255) / 256, sets, nb), dim3(256), 0, c, cols, pc, sigma_val, omega_tw, num, den, per, n, set0);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ grand product
// z[0] = z0, z[i+1] = z[i] * num[i] / den[i], as z[i] = z0 * N(i-1) * D'(i) / T with
//   N(i)  = prod_{j<=i} num'_j          (prefix products)
//   D'(i) = prod_{j>=i} den'_j          (suffix products),  T = prod_j den'_j
// where a zero denominator counts as den' = 1, num' = 0 (halo2's BatchInvert leaves zeros alone, so
// that ratio is 0): ONE field inversion per product instead of one per row.  Strip form, two launches for ALL
// products of a batch, one workgroup of GP_LANES lanes per product, lane l owning rows [l S, (l + 1) S):
//   gp_strip_scan   the strip's num' product and its den' suffix products (kept in HBM, one per row), then prefix /
//                   suffix scans of the strip products over the lanes (Hillis-Steele through LDS), 1 / T, and the
//                   product's value at row `last` for z0 = 1 (feeds the chain);
//   gp_strip_apply  z_i = k_l * (num' prefix inside the strip) * (den' suffix inside the strip) with the lane constant
//                   k_l = z0 * chain / T * N(before the strip) * D'(after the strip): two products per row.
// About 6.5 products per row where the block-scan form (three launches) spent 21.  `chain` leading products of a group
// are chained like the permutation sets: z0 of product j is product j-1's value at row `last`.
// ---- latency form (a lone proof: zg_ctx_set_msm_latency / zg_prover_set_overlap(1)): block-local Hillis-Steele scans,
// coalesced accesses, three short launches -- more products per row (21), but a lone proof waits for dependent chains
// and for memory latency, not for issue slots: 41 us against the strip form's 170 us for the six products of a proof.
constexpr uint32_t GP_BLOCK = 256;

__global__ __launch_bounds__(GP_BLOCK) void gp_local_kernel(const Fe* __restrict__ num, const Fe* __restrict__ den,
                                                             Fe* __restrict__ locn, Fe* __restrict__ locd,
                                                             Fe* __restrict__ totn, Fe* __restrict__ totd, uint32_t n,
                                                             uint32_t nblk) {
    __shared__ Fe shn[GP_BLOCK], shd[GP_BLOCK];
    const uint32_t tid = threadIdx.x, blk = blockIdx.x, b = blockIdx.y;
    const uint32_t i = blk * GP_BLOCK + tid;
    Fe nv = Fr::one(), dv = Fr::one();
    if (i < n) {
        Fe d = ldg(den + (size_t)b * n + i);
        if (fe_is_zero(d)) {
            nv = fe_zero();
        } else {
            nv = ldg(num + (size_t)b * n + i);
            dv = d;
        }
    }
    shn[tid] = nv;
    shd[tid] = dv;
    __syncthreads();
    for (uint32_t off = 1; off < GP_BLOCK; off <<= 1) {
        Fe pn = Fr::one(), pd = Fr::one();
        const bool hn = tid >= off, hd = tid + off < GP_BLOCK;
        if (hn) pn = shn[tid - off];
        if (hd) pd = shd[tid + off];
        __syncthreads();
        if (hn) shn[tid] = Fr::mul(shn[tid], pn);
        if (hd) shd[tid] = Fr::mul(shd[tid], pd);
        __syncthreads();
    }
    if (i < n) {
        stg(locn + (size_t)b * n + i, shn[tid]);  // inclusive prefix inside the block
        stg(locd + (size_t)b * n + i, shd[tid]);  // inclusive suffix inside the block
    }
    if (tid == 0) {
        stg(totn + (size_t)b * nblk + blk, shn[GP_BLOCK - 1]);
        stg(totd + (size_t)b * nblk + blk, shd[0]);
    }
}

// per product: exclusive prefix of the block totals of num', exclusive suffix of those of den', 1/T,
// and the product's value at row `last` for z0 = 1 (feeds the chain)
__global__ __launch_bounds__(1024) void gp_totals_kernel(Fe* __restrict__ totn, Fe* __restrict__ totd,
                                                         const Fe* __restrict__ locn, const Fe* __restrict__ locd,
                                                         Fe* __restrict__ tinv, Fe* __restrict__ zlast, uint32_t n,
                                                         uint32_t nblk, uint32_t last, uint32_t defer_inverse) {
    __shared__ Fe shn[1024], shd[1024];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    Fe* tn = totn + (size_t)b * nblk;
    Fe* td = totd + (size_t)b * nblk;
    Fe vn = Fr::one(), vd = Fr::one();
    if (tid < nblk) {
        vn = ldg(tn + tid);
        vd = ldg(td + tid);
    }
    shn[tid] = vn;
    shd[tid] = vd;
    __syncthreads();
    // (entries at and beyond nblk are ones: the scan only has to span the block totals)
    uint32_t span = 64;
    while (span < nblk) span <<= 1;
    for (uint32_t off = 1; off < span; off <<= 1) {
        Fe pn = Fr::one(), pd = Fr::one();
        const bool hn = tid >= off && tid < span, hd = tid + off < span;
        if (hn) pn = shn[tid - off];
        if (hd) pd = shd[tid + off];
        __syncthreads();
        if (hn) shn[tid] = Fr::mul(shn[tid], pn);
        if (hd) shd[tid] = Fr::mul(shd[tid], pd);
        __syncthreads();
    }
    // exclusive forms
    Fe en = tid > 0 ? shn[tid - 1] : Fr::one();
    Fe ed = tid + 1 < 1024 ? shd[tid + 1] : Fr::one();
    Fe total_d = shd[0];
    __syncthreads();
    if (tid < nblk) {
        stg(tn + tid, en);
        stg(td + tid, ed);
    }
    shn[tid] = en;
    shd[tid] = ed;
    __syncthreads();
    if (tid == 0) {
        // defer_inverse: the host inverts T (tinv[b] <- T, zlast[b] <- the product without 1/T); a lone lane
        // spends ~0.1 ms on it, the host a few microseconds -- worth a round trip when one proof is all there is
        Fe ti = defer_inverse ? total_d : Fr::inv(total_d);
        stg(tinv + b, ti);
        // z(last) for z0 = 1: N(last-1) * D'(last) / T
        Fe v = defer_inverse ? Fr::one() : ti;
        if (last < n) {
            uint32_t lb = last / GP_BLOCK;
            v = Fr::mul(v, Fr::mul(ldg(locd + (size_t)b * n + last), shd[lb]));
            if (last > 0) {
                uint32_t pb = (last - 1) / GP_BLOCK;
                v = Fr::mul(v, Fr::mul(ldg(locn + (size_t)b * n + last - 1), shn[pb]));
            }
        }
        stg(zlast + b, v);
    }
}

__global__ __launch_bounds__(GP_BLOCK) void gp_apply_kernel(const Fe* __restrict__ locn, const Fe* __restrict__ locd,
                                                            const Fe* __restrict__ totn, const Fe* __restrict__ totd,
                                                            const Fe* __restrict__ tinv, const Fe* __restrict__ zlast,
                                                            const Fe* __restrict__ z0, Fe* __restrict__ z, uint32_t n,
                                                            uint32_t nblk, uint32_t chain, FeSet host_tinv, uint32_t use_host,
                                                            uint32_t per, size_t z_outer) {
    const uint32_t tid = threadIdx.x, blk = blockIdx.x, b = blockIdx.y;
    const uint32_t i = blk * GP_BLOCK + tid;
    if (i >= n) return;
    const uint32_t j = b % per, g0 = b - j;  // product j of its group; the group's first product
    // start value: z0[b] (if given) times the chained last values of the group's products before this one
    // (use_host: 1/T arrives in the kernel arguments and zlast still lacks that factor; one group only)
    Fe c = z0 ? ldg(z0 + b) : Fr::one();
    if (j < chain)
        for (uint32_t s = 0; s < j; s++) {
            c = Fr::mul(c, ldg(zlast + g0 + s));
            if (use_host) c = Fr::mul(c, host_tinv.v[s]);
        }
    Fe v = Fr::mul(c, use_host ? host_tinv.v[b] : ldg(tinv + b));
    v = Fr::mul(v, Fr::mul(ldg(locd + (size_t)b * n + i), ldg(totd + (size_t)b * nblk + blk)));
    if (i > 0) {
        uint32_t pb = (i - 1) / GP_BLOCK;
        v = Fr::mul(v, Fr::mul(ldg(locn + (size_t)b * n + i - 1), ldg(totn + (size_t)b * nblk + pb)));
    }
    stg(z + (size_t)(b / per) * z_outer + (size_t)j * n + i, v);
}

// ---- throughput form
constexpr uint32_t GP_LANES = 1024;

__device__ __forceinline__ void gp_load(const Fe* num, const Fe* den, size_t at, Fe& nv, Fe& dv) {
    dv = ldg(den + at);
    if (fe_is_zero(dv)) {
        nv = fe_zero();
        dv = Fr::one();
    } else {
        nv = ldg(num + at);
    }
}

// aux per product: [lanes] N before the strip, [lanes] D' after the strip
__global__ __launch_bounds__(GP_LANES) void gp_strip_scan_kernel(const Fe* __restrict__ num, const Fe* __restrict__ den,
                                                                 Fe* __restrict__ locd, Fe* __restrict__ aux,
                                                                 Fe* __restrict__ tinv, Fe* __restrict__ zlast, uint32_t n,
                                                                 uint32_t lanes, uint32_t strip, uint32_t last,
                                                                 uint32_t defer_inverse) {
    __shared__ Fe shn[GP_LANES], shd[GP_LANES];
    __shared__ Fe s_n_last, s_d_last;
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const size_t base = (size_t)b * n;
    const uint32_t i0 = tid * strip;
    const uint32_t i1 = tid < lanes ? (i0 + strip < n ? i0 + strip : n) : i0;
    // ascending: the strip's num' product (and its value up to row last - 1, if that row is here)
    Fe pn = Fr::one(), n_at_last = Fr::one();
    for (uint32_t i = i0; i < i1; i++) {
        Fe nv, dv;
        gp_load(num, den, base + i, nv, dv);
        pn = Fr::mul(pn, nv);
        if (i + 1 == last) n_at_last = pn;
    }
    // descending: den' suffix products inside the strip, one per row
    Fe sd = Fr::one(), d_at_last = Fr::one();
    for (uint32_t i = i1; i-- > i0;) {
        Fe dv = ldg(den + base + i);
        if (!fe_is_zero(dv)) sd = Fr::mul(sd, dv);
        stg(locd + base + i, sd);
        if (i == last) d_at_last = sd;
    }
    shn[tid] = pn;
    shd[tid] = sd;
    __syncthreads();
    for (uint32_t off = 1; off < GP_LANES; off <<= 1) {
        Fe a = Fr::one(), d = Fr::one();
        const bool hn = tid >= off, hd = tid + off < GP_LANES;
        if (hn) a = shn[tid - off];
        if (hd) d = shd[tid + off];
        __syncthreads();
        if (hn) shn[tid] = Fr::mul(shn[tid], a);
        if (hd) shd[tid] = Fr::mul(shd[tid], d);
        __syncthreads();
    }
    const Fe n_before = tid > 0 ? shn[tid - 1] : Fr::one();
    const Fe d_after = tid + 1 < GP_LANES ? shd[tid + 1] : Fr::one();
    if (tid < lanes) {
        stg(aux + (size_t)b * 2 * lanes + tid, n_before);
        stg(aux + (size_t)b * 2 * lanes + lanes + tid, d_after);
    }
    // the value at row `last` for z0 = 1: N(last - 1) * D'(last) / T, pieces from the lanes that own those rows
    if (tid == 0) {
        s_n_last = Fr::one();
        s_d_last = Fr::one();
    }
    __syncthreads();
    if (last < n) {
        if (last > 0 && last - 1 >= i0 && last - 1 < i1) s_n_last = Fr::mul(n_before, n_at_last);
        if (last >= i0 && last < i1) s_d_last = Fr::mul(d_after, d_at_last);
    }
    __syncthreads();
    if (tid == 0) {
        // defer_inverse: the host inverts T (tinv[b] <- T, zlast[b] <- the product without 1/T); a lone lane
        // spends ~0.1 ms on it, the host a few microseconds -- worth a round trip when one proof is all there is
        const Fe total_d = shd[0];
        const Fe ti = defer_inverse ? total_d : Fr::inv(total_d);
        stg(tinv + b, ti);
        Fe v = defer_inverse ? Fr::one() : ti;
        if (last < n) v = Fr::mul(v, Fr::mul(s_n_last, s_d_last));
        stg(zlast + b, v);
    }
}

__global__ __launch_bounds__(256) void gp_strip_apply_kernel(const Fe* __restrict__ num, const Fe* __restrict__ den,
                                                             const Fe* __restrict__ locd, const Fe* __restrict__ aux,
                                                             const Fe* __restrict__ tinv, const Fe* __restrict__ zlast,
                                                             const Fe* __restrict__ z0, Fe* __restrict__ z, uint32_t n,
                                                             uint32_t lanes, uint32_t strip, uint32_t chain, FeSet host_tinv,
                                                             uint32_t use_host, uint32_t per, size_t z_outer) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (l >= lanes) return;
    const uint32_t j = b % per, g0 = b - j;  // product j of its group; the group's first product
    // start value: z0[b] (if given) times the chained last values of the group's products before this one
    // (use_host: 1/T arrives in the kernel arguments and zlast still lacks that factor; one group only)
    Fe c = z0 ? ldg(z0 + b) : Fr::one();
    if (j < chain)
        for (uint32_t s = 0; s < j; s++) {
            c = Fr::mul(c, ldg(zlast + g0 + s));
            if (use_host) c = Fr::mul(c, host_tinv.v[s]);
        }
    Fe run = Fr::mul(c, use_host ? host_tinv.v[b] : ldg(tinv + b));
    run = Fr::mul(run, Fr::mul(ldg(aux + (size_t)b * 2 * lanes + l), ldg(aux + (size_t)b * 2 * lanes + lanes + l)));
    const size_t base = (size_t)b * n;
    Fe* zo = z + (size_t)(b / per) * z_outer + (size_t)j * n;
    const uint32_t i0 = l * strip, i1 = i0 + strip < n ? i0 + strip : n;
    for (uint32_t i = i0; i < i1; i++) {
        stg(zo + i, Fr::mul(run, ldg(locd + base + i)));  // k_l * N(strip start .. i-1) * D'(i .. strip end)
        Fe nv, dv;
        gp_load(num, den, base + i, nv, dv);
        run = Fr::mul(run, nv);
    }
}

// tmp: batch*n (den' suffixes) + 2*batch*GP_LANES (lane constants) + 2*batch elements
size_t poly_grand_product_tmp_elems(uint32_t n, uint32_t batch) {  // (room for either form)
    const size_t nblk = (n + GP_BLOCK - 1) / GP_BLOCK;
    const size_t strips = (size_t)batch * n + (size_t)2 * batch * GP_LANES + (size_t)2 * batch;
    const size_t blocks = (size_t)2 * batch * n + (size_t)2 * batch * nblk + (size_t)2 * batch;
    return strips > blocks ? strips : blocks;
}

// the host's shared inversion of up to FESET_MAX grand-product totals -- Montgomery's trick: prefix products, one inversion,
// walk back (a zero total inverts to zero, as Fr::inv does)
static void invert_totals(const Fe* h, uint32_t batch, FeSet& inv_set) {
    Fe pre[FESET_MAX], acc = Fr::one();
    for (uint32_t b = 0; b < batch; b++) {
        pre[b] = acc;
        if (!fe_is_zero(h[b])) acc = Fr::mul(acc, h[b]);
    }
    acc = Fr::inv(acc);
    for (uint32_t b = batch; b-- > 0;) {
        if (fe_is_zero(h[b])) {
            inv_set.v[b] = fe_zero();
            continue;
        }
        inv_set.v[b] = Fr::mul(acc, pre[b]);
        acc = Fr::mul(acc, h[b]);
    }
}

// the latency form's launch sequence (tmp: 2*batch*n + 2*batch*nblk + 2*batch elements)
static int grand_product_blocks(zg_ctx* ctx, const Fe* num, const Fe* den, const Fe* d_z0, Fe* z, Fe* tmp, uint32_t n,
                                uint32_t batch, uint32_t chain, uint32_t last, uint32_t per, size_t z_outer, int half) {
    const uint32_t nblk = (n + GP_BLOCK - 1) / GP_BLOCK;
    ZG_REQUIRE(nblk <= 1024, ZG_ERR_UNSUPPORTED, "grand product: n=%u > 2^18 not built", n);
    Fe* locn = tmp;
    Fe* locd = locn + (size_t)batch * n;
    Fe* totn = locd + (size_t)batch * n;
    Fe* totd = totn + (size_t)batch * nblk;
    Fe* tinv = totd + (size_t)batch * nblk;
    Fe* zlast = tinv + batch;
    // the UNIT: one running product = num, den in, z out = 3 n * 32 B, carried by the apply kernel; each
    // kernel's own streams beside it (the block-local products cross HBM between the launches)
    const double bytes = (double)batch * n * 96;
    if (half != 2)
        ZG_LAUNCH(ctx, "grand_product_local", (double)batch * n * 128, gp_local_kernel, dim3(nblk, batch), dim3(GP_BLOCK), 0, num, den, locn,
                  locd, totn, totd, n, nblk);
    // latency configuration: the host inverts the totals (one shared inversion) between the two launches
    const bool host_inv = ctx->msm_pair && batch <= FESET_MAX && batch == per;
    // (... which the totals kernel writes straight into the context's pinned, mapped host buffer: no copy command between
    //  the kernel and the host's wait)
    Fe* h = nullptr;
    void* h_dev = nullptr;
    if (host_inv) {
        ZG_TRY(pinned_reserve(ctx, 4096));
        h = reinterpret_cast<Fe*>(ctx->pinned);
        ZG_HIP(hipHostGetDevicePointer(&h_dev, ctx->pinned, 0));
    }
    if (half != 2)
        ZG_LAUNCH(ctx, "grand_product_totals", (double)batch * nblk * 128, gp_totals_kernel, dim3(batch), dim3(1024), 0, totn, totd, locn, locd,
                  host_inv ? reinterpret_cast<Fe*>(h_dev) : tinv, zlast, n, nblk, last, host_inv ? 1u : 0u);
    if (half == 1) {
        ZG_HIP(hipGetLastError());
        return ZG_OK;
    }
    FeSet inv_set;
    memset(&inv_set, 0, sizeof(inv_set));
    if (host_inv) {
        ZG_HIP(hipStreamSynchronize(ctx->stream));
        invert_totals(h, batch, inv_set);
    }
    ZG_LAUNCH_U(ctx, "grand_product_apply", bytes, bytes, gp_apply_kernel, dim3(nblk, batch), dim3(GP_BLOCK), 0, locn, locd, totn,
              totd, tinv, zlast, d_z0, z, n, nblk, chain, inv_set, host_inv ? 1u : 0u, per, z_outer);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}


int poly_grand_product(zg_ctx* ctx, const Fe* num, const Fe* den, const Fe* d_z0, Fe* z, Fe* tmp, uint32_t n,
                       uint32_t batch, uint32_t chain, uint32_t last, uint32_t per, size_t z_outer, int half) {
    if (!batch || !n) return ZG_OK;
    if (per == 0) {  // one group, results back to back
        per = batch;
        z_outer = 0;
    }
    ZG_REQUIRE(batch % per == 0, ZG_ERR_INVALID_ARG, "grand product: %u products in groups of %u", batch, per);
    if (batch == per) z_outer = 0;
    if (ctx->msm_pair && n <= (1u << 18)) return grand_product_blocks(ctx, num, den, d_z0, z, tmp, n, batch, chain, last, per, z_outer, half);
    const uint32_t lanes = n < GP_LANES ? n : GP_LANES;
    const uint32_t strip = (n + lanes - 1) / lanes;
    Fe* locd = tmp;
    Fe* aux = locd + (size_t)batch * n;
    Fe* tinv = aux + (size_t)2 * batch * GP_LANES;
    Fe* zlast = tinv + batch;
    const double bytes = (double)batch * n * 96;
    // latency configuration: the host inverts the totals (one shared inversion) between the two launches
    const bool host_inv = ctx->msm_pair && batch <= FESET_MAX && batch == per;
    if (half != 2)
        ZG_LAUNCH(ctx, "grand_product_scan", bytes, gp_strip_scan_kernel, dim3(batch), dim3(GP_LANES), 0, num, den, locd, aux, tinv,
                  zlast, n, lanes, strip, last, host_inv ? 1u : 0u);
    if (host_inv) ZG_TRY(pinned_reserve(ctx, 4096));
    Fe* h = reinterpret_cast<Fe*>(ctx->pinned);
    if (host_inv && half != 2) ZG_HIP(hipMemcpyAsync(h, tinv, batch * sizeof(Fe), hipMemcpyDeviceToHost, ctx->stream));
    if (half == 1) {
        ZG_HIP(hipGetLastError());
        return ZG_OK;
    }
    FeSet inv_set;
    memset(&inv_set, 0, sizeof(inv_set));
    if (host_inv) {
        ZG_HIP(hipStreamSynchronize(ctx->stream));
        invert_totals(h, batch, inv_set);
    }
    ZG_LAUNCH_U(ctx, "grand_product_apply", (double)batch * n * 128, bytes, gp_strip_apply_kernel, dim3((lanes + 255) / 256, batch), dim3(256), 0, num, den,
              locd, aux, tinv, zlast, d_z0, z, n, lanes, strip, chain, inv_set, host_inv ? 1u : 0u, per, z_outer);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ evaluate_h
// Evaluator::evaluate_h for one circuit instance: gates, permutation argument, lookup arguments folded
// by y on every point of the extended coset; the division by (X^n - 1) of vanishing::construct is
// fused into the store (t_eval has period 2^(ext_k - k)).
// One proof of a lock-step batch per grid row: its scalars, coset slabs and output (both kernels below).
struct EvalHProof {
    const ProofConst* pc;
    Cols cols;
    const Fe *pz_cos, *lz_cos, *pin_cos, *ptab_cos;
    Fe* h;
};
__device__ __forceinline__ EvalHProof evalh_proof(const EvalHArgs& a, uint32_t b) {
    EvalHProof r;
    r.pc = a.pc + b;
    r.cols = cols_of(a.cols, b);
    const size_t o = (size_t)b * a.cos_bs;
    r.pz_cos = a.pz_cos + o;
    r.lz_cos = a.lz_cos + o;
    r.pin_cos = a.pin_cos + o;
    r.ptab_cos = a.ptab_cos + o;
    r.h = a.h + (size_t)b * a.h_bs;
    return r;
}

__global__ __launch_bounds__(256) void evaluate_h_kernel(EvalHArgs a, uint32_t en) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= en) return;
    const EvalHProof pr = evalh_proof(a, blockIdx.y);
    const Fe y = pr.pc->eh_y, beta = pr.pc->eh_beta, gamma = pr.pc->eh_gamma, theta = pr.pc->eh_theta;
    const DevCircuit& c = a.c;
    const uint32_t mask = en - 1;
    const uint32_t rs = (uint32_t)a.cols.rot_scale;
    const uint32_t r_next = (idx + rs) & mask;
    const uint32_t r_prev = (idx - rs) & mask;
    const uint32_t r_last = (idx + (uint32_t)(a.last_rot * (int32_t)rs)) & mask;
    Fe value = fe_zero();
    for (uint32_t g = 0; g < c.n_gates; g++)
        value = Fr::add(Fr::mul(value, y), eval_poly(c, pr.cols, c.gates[g], idx));

    const Fe l0 = ldg(a.l0 + idx), llast = ldg(a.llast + idx), lactive = ldg(a.lactive + idx);
    if (c.n_sets > 0) {
        const Fe zf = ldg(pr.pz_cos + idx);
        const Fe zl = ldg(pr.pz_cos + (size_t)(c.n_sets - 1) * en + idx);
        value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::sub(Fr::one(), zf), l0));
        value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::sub(Fr::sqr(zl), zl), llast));
        for (uint32_t s = 1; s < c.n_sets; s++) {
            Fe t = Fr::sub(ldg(pr.pz_cos + (size_t)s * en + idx), ldg(pr.pz_cos + (size_t)(s - 1) * en + r_last));
            value = Fr::add(Fr::mul(value, y), Fr::mul(t, l0));
        }
        Fe current_delta = Fr::mul(pr.pc->eh_delta_start[a.zpow - 1], ldg(a.ext_tw + idx));
        for (uint32_t s = 0; s < c.n_sets; s++) {
            uint32_t c0 = s * c.chunk, c1 = c0 + c.chunk;
            if (c1 > c.n_perm) c1 = c.n_perm;
            Fe left = ldg(pr.pz_cos + (size_t)s * en + r_next);
            Fe right = ldg(pr.pz_cos + (size_t)s * en + idx);
            for (uint32_t col = c0; col < c1; col++) {
                const zg_query q = c.perm_cols[col];
                const Fe* base = q.kind == ZG_FIXED ? pr.cols.fixed : q.kind == ZG_ADVICE ? pr.cols.advice : pr.cols.instance;
                Fe v = ldg(base + ((size_t)q.column << a.cols.log_size) + idx);
                Fe sg = ldg(a.sigma_cos + (size_t)col * en + idx);
                left = Fr::mul(left, Fr::add(Fr::add(Fr::mul(beta, sg), v), gamma));
                right = Fr::mul(right, Fr::add(Fr::add(v, current_delta), gamma));
                current_delta = Fr::mul(current_delta, a.delta);
            }
            value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::sub(left, right), lactive));
        }
    }
    for (uint32_t l = 0; l < c.n_lookups; l++) {
        const DLookup* lk = c.lookups + l;
        Fe ai = fe_zero(), ti = fe_zero();
        for (uint32_t e = 0; e < lk->width; e++) {  // (the first expression enters as it is)
            const Fe in = eval_poly(c, pr.cols, lk->inputs[e], idx), tb = eval_poly(c, pr.cols, lk->tables[e], idx);
            ai = e ? Fr::add(Fr::mul(ai, theta), in) : in;
            ti = e ? Fr::add(Fr::mul(ti, theta), tb) : tb;
        }
        const Fe* zc = pr.lz_cos + (size_t)l * en;
        const Fe* ap = pr.pin_cos + (size_t)l * a.perm_stride;
        const Fe* sp = pr.ptab_cos + (size_t)l * a.perm_stride;
        const Fe z = ldg(zc + idx), apv = ldg(ap + idx), spv = ldg(sp + idx);
        value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::sub(Fr::one(), z), l0));
        value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::sub(Fr::sqr(z), z), llast));
        Fe lft = Fr::mul(Fr::mul(Fr::add(apv, beta), Fr::add(spv, gamma)), ldg(zc + r_next));
        Fe rgt = Fr::mul(Fr::mul(Fr::add(ai, beta), Fr::add(ti, gamma)), z);
        value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::sub(lft, rgt), lactive));
        Fe ams = Fr::sub(apv, spv);
        value = Fr::add(Fr::mul(value, y), Fr::mul(ams, l0));
        value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::mul(ams, Fr::sub(apv, ldg(ap + r_prev))), lactive));
    }
    // divide_by_vanishing_poly
    value = Fr::mul(value, ldg(a.t_eval + (idx & a.t_mask)));
    stg(pr.h + idx, value);
}


// ---- the same evaluation on nine 29-bit limbs (field9.h).  Every operand is in the 2^261 Montgomery form,
// so Fr9::mul is the field product; sums are limb-wise and lazily normalised under one rule: both
// operands of a product have limb magnitudes < 2^29, except that ONE of them may be the sum of two
// normalised values (< 2^30).  A normalised value plus a product (the Horner step) therefore feeds the
// next product directly.
__device__ __forceinline__ F9 ld9(const Fe* p) { return f9_unpack(ldg(p)); }

__device__ __forceinline__ F9 eval_poly9(const DevCircuit& c, const DMono* monos, const Cols& cols, zg_poly p, uint32_t row) {
    const uint32_t mask = (1u << cols.log_size) - 1u;
    auto cell = [&](uint32_t qi) {
        const zg_query q = c.queries[qi];
        const Fe* base = q.kind == ZG_FIXED ? cols.fixed : q.kind == ZG_ADVICE ? cols.advice : cols.instance;
        const uint32_t idx = (row + (uint32_t)(q.rotation * cols.rot_scale)) & mask;
        return ld9(base + ((size_t)q.column << cols.log_size) + idx);
    };
    F9 acc;
#pragma unroll
    for (int i = 0; i < 9; i++) acc.l[i] = 0;
    uint32_t pending = 0;  // terms added since the last carry normalisation
    auto add = [&](const F9& t, bool neg) {  // acc +/- t  (a coefficient -1 is a subtraction, not a product)
        acc = neg ? f9_sub(acc, t) : f9_add(acc, t);
        if (++pending == 2) {  // (wave-uniform: the monomial list is)
            acc = f9_norm(acc);
            pending = 0;
        }
    };
    // A monomial is +/- L * R with R its last factor; the final products of two consecutive monomials share one
    // Montgomery reduction (Fr9::mul2).
    F9 hl, hr;          // a monomial waiting for its partner
    bool held = false, hneg = false;
    for (uint32_t m = p.first; m < p.first + p.count; m++) {
        const DMono* mo = monos + m;
        const uint32_t nf = mo->n_factors;
        const uint32_t kind = mo->coeff_is_one;  // (wave-uniform, like everything read from the monomial)
        const bool small = kind == 3 && nf > 0;  // a small integer coefficient: its first cell times it, no product
        const bool unit = (kind == 1 || kind == 2 || small) && nf > 0;
        const bool neg = kind == 2 && nf > 0;
        const uint32_t terms = nf + (unit ? 0u : 1u);  // operands of the product
        if (terms == 1) {  // a bare cell (times a small integer) or a bare constant
            F9 t = unit ? cell(mo->factors[0]) : f9_unpack(mo->coeff);
            if (small) t = f9_mul_small<Fr9Params>(t, mo->small);
            add(t, neg);
            continue;
        }
        uint32_t f = 0;
        F9 l = unit ? cell(mo->factors[f++]) : f9_unpack(mo->coeff);
        if (small) l = f9_mul_small<Fr9Params>(l, mo->small);
        for (; f + 1 < nf; f++) l = Fr9::mul(l, cell(mo->factors[f]));
        const F9 r = cell(mo->factors[nf - 1]);
        if (held) {
            if (hneg == neg) add(Fr9::mul2<false>(hl, hr, l, r), neg);
            else add(Fr9::mul2<true>(hl, hr, l, r), hneg);  // +(hl hr - l r) or -(hl hr - l r)
            held = false;
        } else {
            hl = l;
            hr = r;
            hneg = neg;
            held = true;
        }
    }
    if (held) add(Fr9::mul(hl, hr), hneg);
    return f9_norm(acc);
}

// U(x) = x * (c_1 + x * (c_2 + ... )) for wave-uniform coefficients c_k = coef[k-1], k = 1..count
__device__ __forceinline__ F9 horner9(const F9& x, const Fe* coef, uint32_t count) {
    F9 u = f9_unpack(coef[count - 1]);
    for (uint32_t k = count - 1; k >= 1; k--) u = f9_add(Fr9::mul(u, x), f9_unpack(coef[k - 1]));
    return Fr9::mul(u, x);
}

__global__ __launch_bounds__(256) void gate_factor9_kernel(const Fe* __restrict__ col, uint32_t rot_off, uint32_t en,
                                                           const Fe* __restrict__ coef, uint32_t count, Fe* __restrict__ out) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= en) return;
    stg(out + idx, f9_reduce_pack<Fr9Params>(horner9(ld9(col + ((idx + rot_off) & (en - 1))), coef, count)));
}

int poly_gate_factor(zg_ctx* ctx, const Fe* col, uint32_t rot_off, uint32_t en, const Fe* coef, uint32_t count, Fe* out) {
    ZG_REQUIRE(count >= 1 && (en & (en - 1)) == 0, ZG_ERR_INVALID_ARG, "poly_gate_factor: %u coefficients, %u points", count, en);
    ZG_LAUNCH(ctx, "gate_factor", 2.0 * en * 32.0, gate_factor9_kernel, dim3((en + 255) / 256), dim3(256), 0, col, rot_off, en, coef,
              count, out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// GROUPED: the terms after the gates are not folded one by one (value * y + term * l, two products each) but
// weighted and summed per l-polynomial,
//     h_num = G y^T + l0 * sum_i y^e_i a_i + llast * sum_i y^e_i b_i + lactive * sum_i y^e_i c_i,
// with the powers of y from pc->eh_ypow: one product per term (two terms per Montgomery reduction) + four at the
// end -- the same field element, since the arithmetic is exact.
//
// Grid: one workgroup per (row tile, proof), the proof index the fast dimension.  Workgroups are dealt to the 8 XCDs
// round-robin, so -- as in ntt_pass_kernel -- workgroup L is renumbered to put consecutive numbers on ONE XCD: the nb
// proofs of a tile then run side by side behind one L2, and the key's lines of that tile (fixed cosets, gate slabs, sigma,
// l-polynomials: two thirds of what a row reads) are fetched once per batch instead of once per proof.
//
// MODE (GROUPED only): the terms by their degree, for the two parts of the split domain.  A term of degree <= m1 + 1 (low)
// contributes a quotient part of degree < m1 n, which the first part's m1 n points fix alone; only the others (high) are
// needed on the second part.  EH_BOTH (part 1) keeps the two classes in separate sums -- each class's gates in a Horner
// carry of its own that skips the other class's places by a power of y (EvalHArgs::gate_cls), the high permutation sets
// and lookup products in a fourth weighted sum -- and stores all terms / Z_H to h, the high ones / Z_H to h_hi; EH_HIGH
// (part 2) evaluates the high terms alone and loads nothing that only a low term reads.  EH_ALL is the kernel as it was.
template <bool GROUPED, int MODE = EH_ALL>
__global__ __launch_bounds__(256) void evaluate_h9_kernel(EvalHArgs a, uint32_t en, uint32_t nb) {
    static_assert(MODE == EH_ALL || GROUPED, "the terms by degree exist in the grouped form only");
    uint32_t bid = blockIdx.x;
    if ((gridDim.x & 7u) == 0) bid = (bid & 7u) * (gridDim.x >> 3) + (bid >> 3);
    const uint32_t tile = bid / nb;
    const uint32_t idx = tile * blockDim.x + threadIdx.x;
    if (idx >= en) return;
    const EvalHProof pr = evalh_proof(a, bid - tile * nb);
    const ProofConst* pc = pr.pc;  // (scalars are re-read where they are used: workgroup-uniform scalar loads)
    const DevCircuit& c = a.c;
    const uint32_t mask = en - 1;
    const uint32_t rs = (uint32_t)a.cols.rot_scale;
    const uint32_t r_next = (idx + rs) & mask;
    const uint32_t r_prev = (idx - rs) & mask;
    const uint32_t r_last = (idx + (uint32_t)(a.last_rot * (int32_t)rs)) & mask;
    // (constants and l-polynomial values are re-materialised at each use: a nine-limb value is 9 VGPRs, and
    // this kernel's occupancy is set by its register count)
    // value <- value * y + term   (term normalised; the sum has limbs < 2^30 and goes into the next product)
    auto fold = [&](const F9& value, const F9& term) { return f9_add(Fr9::mul(value, f9_unpack(pc->eh_y)), term); };
    // value <- value * y + u * v with ONE Montgomery reduction (value normalised, u and v with limbs < 2^29)
    auto fold2 = [&](const F9& value, const F9& u, const F9& v) { return Fr9::mul2<false>(value, f9_unpack(pc->eh_y), u, v); };
    F9 value;
#pragma unroll
    for (int i = 0; i < 9; i++) value.l[i] = 0;
    auto cell = [&](uint32_t qi) {
        const zg_query q = c.queries[qi];
        const Fe* base = q.kind == ZG_FIXED ? pr.cols.fixed : q.kind == ZG_ADVICE ? pr.cols.advice : pr.cols.instance;
        return ld9(base + ((size_t)q.column << a.cols.log_size) + ((idx + (uint32_t)(q.rotation * a.cols.rot_scale)) & mask));
    };
    [[maybe_unused]] F9 vhi;  // MODE: the high gates' carry (`value` is the low gates')
    if constexpr (MODE != EH_ALL) {
#pragma unroll
        for (int i = 0; i < 9; i++) vhi.l[i] = 0;
    }
    for (uint32_t g = 0; g < c.n_gates; g++) {
        if constexpr (MODE != EH_ALL) {
            const uint32_t cls = a.gate_cls[g];  // (wave-uniform)
            if (MODE == EH_HIGH && !(cls & 1u)) continue;
            const F9 inner = eval_poly9(c, a.monos_hat, pr.cols, a.gates_hat[g], idx);
            const uint32_t common = a.gate_common[g];
            const bool factored = common != 0xffffffffu;
            F9 u = inner;
            if (factored) {
                const uint32_t slab = a.gate_slab[g];
                const zg_poly uni = a.gate_uni[g];
                if (slab != 0xffffffffu) u = ld9(a.gate_slabs + (size_t)slab * en + idx);
                else if (uni.count) u = horner9(cell(common), a.uni_coef + uni.first, uni.count);
                else u = cell(common);
            }
            // carry * y^e + gate: as fold2 / fold below, with the power of y that skips the other class's gates
            auto step = [&](F9& carry) {
                const F9 ye = f9_unpack(pc->eh_ypow[cls >> 1]);
                if (factored) carry = Fr9::mul2<false>(f9_norm(carry), ye, u, inner);
                else carry = f9_add(Fr9::mul(carry, ye), inner);
            };
            if (cls & 1u) step(vhi);
            else step(value);
            continue;
        }
        const F9 inner = eval_poly9(c, a.monos_hat, pr.cols, a.gates_hat[g], idx);
        const uint32_t common = a.gate_common[g];  // (wave-uniform)
        if (common != 0xffffffffu) {
            const uint32_t slab = a.gate_slab[g];
            const zg_poly uni = a.gate_uni[g];
            F9 u;
            if (slab != 0xffffffffu) {
                u = ld9(a.gate_slabs + (size_t)slab * en + idx);  // U(fixed cell), tabulated with the proving key
            } else if (uni.count) {
                u = horner9(cell(common), a.uni_coef + uni.first, uni.count);
            } else {
                u = cell(common);
            }
            value = fold2(f9_norm(value), u, inner);  // value * y + U(common) * inner, one reduction
        } else {
            value = fold(value, inner);
        }
    }
    value = f9_norm(value);  // from here on every term is a product: fold2 keeps value normalised

    auto l0 = [&]() { return ld9(a.l0 + idx); };
    auto llast = [&]() { return ld9(a.llast + idx); };
    auto lactive = [&]() { return ld9(a.lactive + idx); };
    auto one = [&]() { return Fr9Params::one(); };
    // theta-compression of a lookup's input and table expressions (the first expression enters as it is)
    auto compress = [&](const DLookup* lk, F9& ai, F9& ti) {
        ai = eval_poly9(c, a.monos_hat, pr.cols, lk->inputs[0], idx);
        ti = eval_poly9(c, a.monos_hat, pr.cols, lk->tables[0], idx);
        for (uint32_t e = 1; e < lk->width; e++) {
            ai = f9_add(Fr9::mul(ai, f9_unpack(pc->eh_theta)), eval_poly9(c, a.monos_hat, pr.cols, lk->inputs[e], idx));
            ti = f9_add(Fr9::mul(ti, f9_unpack(pc->eh_theta)), eval_poly9(c, a.monos_hat, pr.cols, lk->tables[e], idx));
        }
    };
    if constexpr (MODE != EH_ALL) {
        // The grouped form below with the lactive sum in two, sa (low) and sh (high); the weights are the same.
        constexpr bool LOW = MODE == EH_BOTH;  // the low terms are evaluated too
        vhi = f9_norm(vhi);
        uint32_t w = a.n_terms;
        auto yw = [&](uint32_t e) { return f9_unpack(pc->eh_ypow[e]); };
        F9 s0, sl, sa, sh;
#pragma unroll
        for (int i = 0; i < 9; i++) s0.l[i] = sl.l[i] = sa.l[i] = sh.l[i] = 0;
        auto acc1 = [&](F9& s, uint32_t e, const F9& t) { s = f9_norm(f9_add(s, Fr9::mul(yw(e), t))); };
        auto acc2 = [&](F9& s, uint32_t e, const F9& t, uint32_t e2, const F9& t2) {
            s = f9_norm(f9_add(s, Fr9::mul2<false>(yw(e), t, yw(e2), t2)));
        };
        if (c.n_sets > 0) {
            if (LOW) {
                const F9 zf = ld9(pr.pz_cos + idx);
                const F9 zl = ld9(pr.pz_cos + (size_t)(c.n_sets - 1) * en + idx);
                acc1(s0, w - 1, f9_sub(one(), zf));
                acc1(sl, w - 2, f9_sub(Fr9::sqr(zl), zl));
                for (uint32_t s = 1; s < c.n_sets; s++) {
                    const F9 t = f9_sub(ld9(pr.pz_cos + (size_t)s * en + idx), ld9(pr.pz_cos + (size_t)(s - 1) * en + r_last));
                    acc1(s0, w - 2 - s, t);
                }
            }
            w -= 2 + (c.n_sets - 1);
            const bool scaled = a.sigma_sc != nullptr && pc->eh_scaled != 0;
            F9 current_delta = ld9(a.ext_tw + idx);
            if (!scaled) current_delta = Fr9::mul(f9_unpack(pc->eh_delta_start[a.zpow - 1]), current_delta);
            for (uint32_t s = 0; s < c.n_sets; s++) {
                uint32_t c0 = s * c.chunk, c1 = c0 + c.chunk;
                if (c1 > c.n_perm) c1 = c.n_perm;
                --w;
                const bool high = (a.set_hi >> s) & 1u;  // (wave-uniform)
                if (!LOW && !high) {  // (the unscaled term's delta chain walks on over the set's columns)
                    if (!scaled)
                        for (uint32_t col = c0; col < c1; col++) current_delta = Fr9::mul(current_delta, f9_unpack(a.delta));
                    continue;
                }
                F9 left = ld9(pr.pz_cos + (size_t)s * en + r_next);
                F9 right = ld9(pr.pz_cos + (size_t)s * en + idx);
                for (uint32_t col = c0; col < c1; col++) {
                    const zg_query q = c.perm_cols[col];
                    const Fe* base = q.kind == ZG_FIXED ? pr.cols.fixed : q.kind == ZG_ADVICE ? pr.cols.advice : pr.cols.instance;
                    const F9 v = ld9(base + ((size_t)q.column << a.cols.log_size) + idx);
                    F9 fl, fr;
                    if (scaled) {
                        const F9 t = Fr9::mul(f9_add(v, f9_unpack(pc->eh_gamma)), f9_unpack(pc->eh_pcol[a.zpow - 1][col]));
                        fl = f9_add(ld9(a.sigma_sc + (size_t)col * en + idx), t);
                        fr = f9_add(current_delta, t);
                    } else {
                        const F9 sg = ld9(a.sigma_cos + (size_t)col * en + idx);
                        fl = f9_norm(f9_add(f9_add(Fr9::mul(f9_unpack(pc->eh_beta), sg), v), f9_unpack(pc->eh_gamma)));
                        fr = f9_norm(f9_add(f9_add(v, current_delta), f9_unpack(pc->eh_gamma)));
                        current_delta = Fr9::mul(current_delta, f9_unpack(a.delta));
                    }
                    if (col + 1 < c1) {
                        left = Fr9::mul(left, fl);
                        right = Fr9::mul(right, fr);
                    } else {
                        left = Fr9::mul2<true>(left, f9_norm(fl), right, f9_norm(fr));
                    }
                }
                const F9 t = Fr9::mul(scaled ? f9_unpack(pc->eh_pw[a.zpow - 1][s]) : yw(w), left);
                if (high) sh = f9_norm(f9_add(sh, t));
                else sa = f9_norm(f9_add(sa, t));
            }
        }
        for (uint32_t l = 0; l < c.n_lookups; l++, w -= 5) {
            const bool high = (a.lk_hi >> l) & 1u;  // (wave-uniform)
            if (!LOW && !high) continue;
            const DLookup* lk = c.lookups + l;
            F9 ai, ti;
            compress(lk, ai, ti);
            const Fe* zc = pr.lz_cos + (size_t)l * en;
            const Fe* ap = pr.pin_cos + (size_t)l * a.perm_stride;
            const Fe* sp = pr.ptab_cos + (size_t)l * a.perm_stride;
            const F9 z = ld9(zc + idx), apv = ld9(ap + idx), spv = ld9(sp + idx);
            const F9 lft = Fr9::mul(f9_add(apv, f9_unpack(pc->eh_beta)), f9_norm(f9_add(spv, f9_unpack(pc->eh_gamma))));
            const F9 rgt = Fr9::mul(f9_norm(f9_add(ai, f9_unpack(pc->eh_beta))), f9_norm(f9_add(ti, f9_unpack(pc->eh_gamma))));
            const F9 prod = Fr9::mul2<true>(lft, ld9(zc + r_next), rgt, z);
            if (high) acc1(sh, w - 3, prod);
            if (LOW) {
                const F9 ams = f9_sub(apv, spv);
                acc2(s0, w - 1, f9_sub(one(), z), w - 4, ams);
                acc1(sl, w - 2, f9_sub(Fr9::sqr(z), z));
                const F9 last = Fr9::mul(ams, f9_sub(apv, ld9(ap + r_prev)));
                if (high) acc1(sa, w - 5, last);
                else acc2(sa, w - 3, prod, w - 5, last);
            }
        }
        // high = vhi y^tail_hi + lactive sh;  low = value y^tail_lo + l0 s0 + llast sl + lactive sa;  both / Z_H
        const F9 hi = Fr9::mul2<false>(vhi, yw(a.tail_hi), sh, lactive());
        const F9 tz = ld9(a.t_eval + (idx & a.t_mask));
        if (LOW) {
            const F9 lo = f9_norm(f9_add(Fr9::mul2<false>(value, yw(a.tail_lo), s0, l0()), Fr9::mul2<false>(sl, llast(), sa, lactive())));
            stg(pr.h + idx, f9_reduce_pack<Fr9Params>(Fr9::mul2<false>(lo, tz, hi, tz)));
            stg(a.h_hi + (size_t)(bid - tile * nb) * a.h_bs + idx, f9_reduce_pack<Fr9Params>(Fr9::mul(hi, tz)));
        } else {
            stg(pr.h + idx, f9_reduce_pack<Fr9Params>(Fr9::mul(hi, tz)));
        }
        return;
    }
    if (GROUPED) {
        // term i of the sequence (upstream's order) carries y^(T - 1 - i); `w` walks down from T - 1
        uint32_t w = a.n_terms;
        auto yw = [&](uint32_t e) { return f9_unpack(pc->eh_ypow[e]); };
        F9 s0, sl, sa;  // the sums that l0, llast and lactive multiply (normalised after every addition)
#pragma unroll
        for (int i = 0; i < 9; i++) s0.l[i] = sl.l[i] = sa.l[i] = 0;
        auto acc1 = [&](F9& s, uint32_t e, const F9& t) { s = f9_norm(f9_add(s, Fr9::mul(yw(e), t))); };
        auto acc2 = [&](F9& s, uint32_t e, const F9& t, uint32_t e2, const F9& t2) {
            s = f9_norm(f9_add(s, Fr9::mul2<false>(yw(e), t, yw(e2), t2)));
        };
        if (c.n_sets > 0) {
            const F9 zf = ld9(pr.pz_cos + idx);
            const F9 zl = ld9(pr.pz_cos + (size_t)(c.n_sets - 1) * en + idx);
            acc1(s0, w - 1, f9_sub(one(), zf));
            acc1(sl, w - 2, f9_sub(Fr9::sqr(zl), zl));
            w -= 2;
            for (uint32_t s = 1; s < c.n_sets; s++) {
                const F9 t = f9_sub(ld9(pr.pz_cos + (size_t)s * en + idx), ld9(pr.pz_cos + (size_t)(s - 1) * en + r_last));
                acc1(s0, --w, t);
            }
            // Scaled (pc->eh_scaled, workgroup-uniform): both factors of a column divided by K = beta delta^col zeta^a,
            //     (beta sigma + v + gamma) / K = sigma_sc + t,   (v + beta delta^col zeta^a w^idx + gamma) / K = w^idx + t,
            // t = (v + gamma) K^-1 with K^-1 = pc->eh_pcol: three products per column, and the set's weight pc->eh_pw
            // carries prod K -- the same term, exactly.  Operand bounds: v + gamma and sigma_sc + t / w^idx + t are sums
            // of two normalised values (limbs < 2^30, magnitude < 2^258) beside a normalised operand, as Fr9::mul allows;
            // Fr9::mul2 wants all four below 2^29, so the last column's sums are normalised.
            const bool scaled = a.sigma_sc != nullptr && pc->eh_scaled != 0;
            // w^idx (scaled) or beta zeta^a w^idx, which then walks up by delta (unscaled)
            F9 current_delta = ld9(a.ext_tw + idx);
            if (!scaled) current_delta = Fr9::mul(f9_unpack(pc->eh_delta_start[a.zpow - 1]), current_delta);
            for (uint32_t s = 0; s < c.n_sets; s++) {
                uint32_t c0 = s * c.chunk, c1 = c0 + c.chunk;
                if (c1 > c.n_perm) c1 = c.n_perm;
                F9 left = ld9(pr.pz_cos + (size_t)s * en + r_next);
                F9 right = ld9(pr.pz_cos + (size_t)s * en + idx);
                for (uint32_t col = c0; col < c1; col++) {
                    const zg_query q = c.perm_cols[col];
                    const Fe* base = q.kind == ZG_FIXED ? pr.cols.fixed : q.kind == ZG_ADVICE ? pr.cols.advice : pr.cols.instance;
                    const F9 v = ld9(base + ((size_t)q.column << a.cols.log_size) + idx);
                    F9 fl, fr;
                    if (scaled) {
                        const F9 t = Fr9::mul(f9_add(v, f9_unpack(pc->eh_gamma)), f9_unpack(pc->eh_pcol[a.zpow - 1][col]));
                        fl = f9_add(ld9(a.sigma_sc + (size_t)col * en + idx), t);
                        fr = f9_add(current_delta, t);
                    } else {
                        const F9 sg = ld9(a.sigma_cos + (size_t)col * en + idx);
                        fl = f9_norm(f9_add(f9_add(Fr9::mul(f9_unpack(pc->eh_beta), sg), v), f9_unpack(pc->eh_gamma)));
                        fr = f9_norm(f9_add(f9_add(v, current_delta), f9_unpack(pc->eh_gamma)));
                        current_delta = Fr9::mul(current_delta, f9_unpack(a.delta));
                    }
                    if (col + 1 < c1) {
                        left = Fr9::mul(left, fl);
                        right = Fr9::mul(right, fr);
                    } else {
                        left = Fr9::mul2<true>(left, f9_norm(fl), right, f9_norm(fr));
                    }
                }
                --w;
                sa = f9_norm(f9_add(sa, Fr9::mul(scaled ? f9_unpack(pc->eh_pw[a.zpow - 1][s]) : yw(w), left)));
            }
        }
        for (uint32_t l = 0; l < c.n_lookups; l++) {
            const DLookup* lk = c.lookups + l;
            F9 ai, ti;
            compress(lk, ai, ti);
            const Fe* zc = pr.lz_cos + (size_t)l * en;
            const Fe* ap = pr.pin_cos + (size_t)l * a.perm_stride;
            const Fe* sp = pr.ptab_cos + (size_t)l * a.perm_stride;
            const F9 z = ld9(zc + idx), apv = ld9(ap + idx), spv = ld9(sp + idx);
            const F9 lft = Fr9::mul(f9_add(apv, f9_unpack(pc->eh_beta)), f9_norm(f9_add(spv, f9_unpack(pc->eh_gamma))));
            const F9 rgt = Fr9::mul(f9_norm(f9_add(ai, f9_unpack(pc->eh_beta))), f9_norm(f9_add(ti, f9_unpack(pc->eh_gamma))));
            const F9 ams = f9_sub(apv, spv);
            // five terms: (1 - z) l0, (z^2 - z) llast, (lft z(wX) - rgt z) lactive, (a' - s') l0, (a' - s')(a' - a'(w^-1 X)) lactive
            acc2(s0, w - 1, f9_sub(one(), z), w - 4, ams);
            acc1(sl, w - 2, f9_sub(Fr9::sqr(z), z));
            acc2(sa, w - 3, Fr9::mul2<true>(lft, ld9(zc + r_next), rgt, z), w - 5, Fr9::mul(ams, f9_sub(apv, ld9(ap + r_prev))));
            w -= 5;
        }
        // h_num = value y^T + l0 s0 + llast sl + lactive sa
        value = f9_norm(f9_add(Fr9::mul2<false>(value, yw(a.n_terms), s0, l0()), Fr9::mul2<false>(sl, llast(), sa, lactive())));
    } else {
    if (c.n_sets > 0) {
        const F9 zf = ld9(pr.pz_cos + idx);
        const F9 zl = ld9(pr.pz_cos + (size_t)(c.n_sets - 1) * en + idx);
        value = fold2(value, f9_sub(one(), zf), l0());
        value = fold2(value, f9_sub(Fr9::sqr(zl), zl), llast());
        for (uint32_t s = 1; s < c.n_sets; s++) {
            const F9 t = f9_sub(ld9(pr.pz_cos + (size_t)s * en + idx), ld9(pr.pz_cos + (size_t)(s - 1) * en + r_last));
            value = fold2(value, t, l0());
        }
        F9 current_delta = Fr9::mul(f9_unpack(pc->eh_delta_start[a.zpow - 1]), ld9(a.ext_tw + idx));
        const F9 delta = f9_unpack(a.delta);
        for (uint32_t s = 0; s < c.n_sets; s++) {
            uint32_t c0 = s * c.chunk, c1 = c0 + c.chunk;
            if (c1 > c.n_perm) c1 = c.n_perm;
            F9 left = ld9(pr.pz_cos + (size_t)s * en + r_next);
            F9 right = ld9(pr.pz_cos + (size_t)s * en + idx);
            for (uint32_t col = c0; col < c1; col++) {
                const zg_query q = c.perm_cols[col];
                const Fe* base = q.kind == ZG_FIXED ? pr.cols.fixed : q.kind == ZG_ADVICE ? pr.cols.advice : pr.cols.instance;
                const F9 v = ld9(base + ((size_t)q.column << a.cols.log_size) + idx);
                const F9 sg = ld9(a.sigma_cos + (size_t)col * en + idx);
                // three-term sums: normalise before they enter a product
                const F9 fl = f9_norm(f9_add(f9_add(Fr9::mul(f9_unpack(pc->eh_beta), sg), v), f9_unpack(pc->eh_gamma)));
                const F9 fr = f9_norm(f9_add(f9_add(v, current_delta), f9_unpack(pc->eh_gamma)));
                current_delta = Fr9::mul(current_delta, delta);
                if (col + 1 < c1) {
                    left = Fr9::mul(left, fl);
                    right = Fr9::mul(right, fr);
                } else {  // last column of the set: left * fl - right * fr under one reduction
                    left = Fr9::mul2<true>(left, fl, right, fr);
                }
            }
            value = fold2(value, left, lactive());
        }
    }
    for (uint32_t l = 0; l < c.n_lookups; l++) {
        const DLookup* lk = c.lookups + l;
        F9 ai, ti;
        compress(lk, ai, ti);
        const Fe* zc = pr.lz_cos + (size_t)l * en;
        const Fe* ap = pr.pin_cos + (size_t)l * a.perm_stride;
        const Fe* sp = pr.ptab_cos + (size_t)l * a.perm_stride;
        const F9 z = ld9(zc + idx), apv = ld9(ap + idx), spv = ld9(sp + idx);
        value = fold2(value, f9_sub(one(), z), l0());
        value = fold2(value, f9_sub(Fr9::sqr(z), z), llast());
        // (x + beta)(y + gamma): one factor may stay a two-term sum, the other is normalised
        const F9 lft = Fr9::mul(f9_add(apv, f9_unpack(pc->eh_beta)), f9_norm(f9_add(spv, f9_unpack(pc->eh_gamma))));
        const F9 rgt = Fr9::mul(f9_norm(f9_add(ai, f9_unpack(pc->eh_beta))), f9_norm(f9_add(ti, f9_unpack(pc->eh_gamma))));
        value = fold2(value, Fr9::mul2<true>(lft, ld9(zc + r_next), rgt, z), lactive());
        const F9 ams = f9_sub(apv, spv);
        value = fold2(value, ams, l0());
        value = fold2(value, Fr9::mul(ams, f9_sub(apv, ld9(ap + r_prev))), lactive());
    }
    }
    // divide_by_vanishing_poly, then back to the canonical packed form (still x * 2^261)
    value = Fr9::mul(value, ld9(a.t_eval + (idx & a.t_mask)));
    stg(pr.h + idx, f9_reduce_pack<Fr9Params>(value));
}

int poly_evaluate_h(zg_ctx* ctx, const EvalHArgs& a, uint32_t en, uint32_t nb, uint32_t n_columns, double unit_share, EvalHMode mode) {
    if (!nb) return ZG_OK;
    ZG_REQUIRE(a.pc != nullptr && (a.zpow == 1 || a.zpow == 2), ZG_ERR_INVALID_ARG, "evaluate_h: per-proof scalars missing");
    // algorithmic bytes: every input coset read once + h written, as SURVEY.md 8d counts them -- `n_columns` advice,
    // instance and fixed columns, 3 l-polynomials, sigma, the permutation products, 3 polynomials per lookup, h: ONE count
    // (round 3 charged 26 arrays here while bench.py counted 49).  own = over the `en` rows of this launch; unit = over the
    // 2^ext_k rows of EvaluationDomain's extended domain, of which this launch stands for `unit_share`.
    const DevCircuit& c = a.c;
    const double arrays = (double)n_columns + 3.0 + c.n_perm + c.n_sets + 3.0 * c.n_lookups + 1.0;
    const double unit = nb * arrays * unit_share * 32.0;
    ZG_REQUIRE(!a.hat || a.monos_hat != nullptr || (c.n_gates == 0 && c.n_lookups == 0), ZG_ERR_INVALID_ARG,
               "evaluate_h: the 2^261-form monomial table is missing");
    ZG_REQUIRE(!a.hat || c.n_gates == 0 || (a.gates_hat != nullptr && a.gate_common != nullptr && a.gate_uni != nullptr && a.uni_coef != nullptr && a.gate_slab != nullptr && a.gate_slabs != nullptr), ZG_ERR_INVALID_ARG,
               "evaluate_h: the factored gate table is missing");
    ZG_REQUIRE(mode == EH_ALL || (a.hat && a.n_terms && a.gate_cls != nullptr && (mode == EH_HIGH || a.h_hi != nullptr)),
               ZG_ERR_INVALID_ARG, "evaluate_h: the terms by degree need the grouped nine-limb form and their classes");
    const dim3 grid9((en + 255) / 256 * nb);
    if (mode == EH_BOTH)
        ZG_LAUNCH_U(ctx, "evaluate_h", nb * (arrays + 1.0) * en * 32.0, unit, (evaluate_h9_kernel<true, EH_BOTH>), grid9, dim3(256), 0, a, en, nb);
    else if (mode == EH_HIGH)
        ZG_LAUNCH_U(ctx, "evaluate_h", nb * arrays * en * 32.0, unit, (evaluate_h9_kernel<true, EH_HIGH>), grid9, dim3(256), 0, a, en, nb);
    else if (a.hat && a.n_terms)
        ZG_LAUNCH_U(ctx, "evaluate_h", nb * arrays * en * 32.0, unit, evaluate_h9_kernel<true>, dim3((en + 255) / 256 * nb), dim3(256), 0, a, en, nb);
    else if (a.hat)
        ZG_LAUNCH_U(ctx, "evaluate_h", nb * arrays * en * 32.0, unit, evaluate_h9_kernel<false>, dim3((en + 255) / 256 * nb), dim3(256), 0, a, en, nb);
    else
        ZG_LAUNCH_U(ctx, "evaluate_h", nb * arrays * en * 32.0, unit, evaluate_h_kernel, dim3((en + 255) / 256, nb), dim3(256), 0, a, en);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ the shuffle arguments' share of the quotient
// eval_poly on coset slabs that may carry the nine-limb form's factor 2^5 (hat): every cell read is brought back to the
// library form by one product with 2^-5, so the expression comes out in the library form whatever its monomials' degrees
struct LoadUnhat {
    bool hat;
    Fe unhat;
    __device__ __forceinline__ Fe operator()(const Fe* p) const {
        const Fe v = ldg(p);
        return hat ? Fr::mul(v, unhat) : v;
    }
};
// One lane per point of the part, proof b = blockIdx.y.  h (and h_hi, where the terms by degree keep the high terms'
// sum beside it) is read once and written once; y^(3 ns) and y come from the proof's scalars, wave-uniform.  No LDS, no
// atomics.  The sum of the shuffles' terms is formed in the library form and leaves through t_eval, which carries the
// slabs' factor where they have one -- so the sum lands in h's form.
__global__ __launch_bounds__(256) void shuffle_h_kernel(EvalHArgs a, const DLookup* __restrict__ shuffles, uint32_t ns,
                                                        const Fe* __restrict__ sz_cos, uint32_t en, Fe unhat) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= en) return;
    const uint32_t b = blockIdx.y;
    const ProofConst* pc = a.pc + b;
    const Cols cols = cols_of(a.cols, b);
    const Fe y = pc->sh_y, gamma = pc->gamma, theta = pc->theta;
    const uint32_t r_next = (idx + (uint32_t)a.cols.rot_scale) & (en - 1);
    const LoadUnhat ld{a.hat, unhat};
    const Fe l0 = ld(a.l0 + idx), llast = ld(a.llast + idx), lactive = ld(a.lactive + idx);
    const Fe* zc = sz_cos + (size_t)b * a.cos_bs;
    Fe value = fe_zero();
    for (uint32_t j = 0; j < ns; j++, zc += en) {
        const DLookup* sf = shuffles + j;
        Fe ai = fe_zero(), si = fe_zero();
        for (uint32_t e = 0; e < sf->width; e++) {
            const Fe in = eval_poly_with(a.c, cols, sf->inputs[e], idx, ld), sh = eval_poly_with(a.c, cols, sf->tables[e], idx, ld);
            ai = e ? Fr::add(Fr::mul(ai, theta), in) : in;
            si = e ? Fr::add(Fr::mul(si, theta), sh) : sh;
        }
        const Fe z = ld(zc + idx), zn = ld(zc + r_next);
        value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::sub(Fr::one(), z), l0));
        value = Fr::add(Fr::mul(value, y), Fr::mul(Fr::sub(Fr::sqr(z), z), llast));
        const Fe prod = Fr::sub(Fr::mul(zn, Fr::add(si, gamma)), Fr::mul(z, Fr::add(ai, gamma)));
        value = Fr::add(Fr::mul(value, y), Fr::mul(prod, lactive));
    }
    value = Fr::mul(value, ldg(a.t_eval + (idx & a.t_mask)));  // divide_by_vanishing_poly; (hat: back in the slabs' form)
    const Fe ypow = pc->sh_ypow;
    Fe* h = a.h + (size_t)b * a.h_bs + idx;
    stg(h, Fr::add(Fr::mul(ldg(h), ypow), value));
    if (a.h_hi) {
        Fe* hh = a.h_hi + (size_t)b * a.h_bs + idx;
        stg(hh, Fr::add(Fr::mul(ldg(hh), ypow), value));
    }
}

int poly_shuffle_h(zg_ctx* ctx, const EvalHArgs& a, const DLookup* shuffles, uint32_t ns, const Fe* sz_cos, uint32_t en, uint32_t nb) {
    if (!ns || !nb) return ZG_OK;
    ZG_REQUIRE(shuffles && sz_cos && a.pc && a.h && (en & (en - 1)) == 0, ZG_ERR_INVALID_ARG, "shuffle_h: bad argument");
    const Fe unhat = a.hat ? Fr::inv(Fr::from_u64(32)) : Fr::one();
    ZG_LAUNCH(ctx, "shuffle_h", (double)nb * en * 32.0 * (2.0 + 3.0 + 2.0 * ns), shuffle_h_kernel, dim3((en + 255) / 256, nb), dim3(256), 0, a,
              shuffles, ns, sz_cos, en, unhat);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ eval_polynomial
__device__ __forceinline__ const Fe* poly_of(const PolySet& ps, uint32_t ix, uint32_t b) {
    return ix < ps.nsh ? ps.sh + (size_t)ix * ps.n : ps.pp + (size_t)b * ps.pp_bs + (size_t)(ix - ps.nsh) * ps.n;
}

// pow[b][s][i] = x^i for x = pc[b].points[s]: lane computes x^(i0) by square-and-multiply, then a strip of CH products
// (16 in the throughput form; 4 for a lone proof, which waits for the dependent chain: 28 + 4 products instead of 28 + 16)
template <uint32_t CH>
__global__ __launch_bounds__(256) void powers_kernel(const ProofConst* __restrict__ pc, uint32_t n, Fe* __restrict__ pw,
                                                     size_t pw_bs) {
    uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * CH;
    if (i0 >= n) return;
    const uint32_t sl = blockIdx.y, b = blockIdx.z;
    Fe x = pc[b].points[sl];
    Fe cur = Fr::pow_u64(x, i0);
    Fe* out = pw + (size_t)b * pw_bs + (size_t)sl * n;
    for (uint32_t j = 0; j < CH && i0 + j < n; j++) {
        stg(out + i0 + j, cur);
        cur = Fr::mul(cur, x);
    }
}

int poly_powers(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, uint32_t npoints, uint32_t n, Fe* d_pow, size_t pw_bs) {
    if (!npoints || !nb) return ZG_OK;
    ZG_REQUIRE(npoints <= PC_MAX_POINTS, ZG_ERR_UNSUPPORTED, "poly_powers: %u opening points (max %u)", npoints, PC_MAX_POINTS);
    if (ctx->msm_pair)
        ZG_LAUNCH(ctx, "powers", (double)nb * npoints * n * 32, powers_kernel<4>, dim3((n + 256 * 4 - 1) / (256 * 4), npoints, nb),
                  dim3(256), 0, pc, n, d_pow, pw_bs);
    else
        ZG_LAUNCH(ctx, "powers", (double)nb * npoints * n * 32, powers_kernel<16>, dim3((n + 256 * 16 - 1) / (256 * 16), npoints, nb),
                  dim3(256), 0, pc, n, d_pow, pw_bs);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// out[b][j] = <poly_j of proof b, pow_{point_j} of proof b> : one 1024-lane workgroup per (poly, point) pair (a few
// dozen pairs per proof: the wide workgroup is what keeps a lone proof from waiting on 64 products per lane)
constexpr uint32_t DOT_NT = 1024;
__global__ __launch_bounds__(DOT_NT) void dot_kernel(PolySet ps, uint32_t n, const uint32_t* __restrict__ poly_idx,
                                                     const uint32_t* __restrict__ point_idx, const Fe* __restrict__ pw,
                                                     size_t pw_bs, Fe* __restrict__ out, size_t out_bs) {
    __shared__ Fe sh[DOT_NT];
    const uint32_t j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const Fe* p = poly_of(ps, poly_idx[j], b);
    const Fe* w = pw + (size_t)b * pw_bs + (size_t)point_idx[j] * n;
    Fe acc = fe_zero();
    for (uint32_t i = tid; i < n; i += DOT_NT) acc = Fr::add(acc, Fr::mul(ldg(p + i), ldg(w + i)));
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t off = DOT_NT / 2; off > 0; off >>= 1) {
        if (tid < off) sh[tid] = Fr::add(sh[tid], sh[tid + off]);
        __syncthreads();
    }
    if (tid == 0) stg(out + (size_t)b * out_bs + j, sh[0]);
}

// The same dot product with ONE Montgomery reduction per lane (Dot9, field9.h): a term is its 81 multiply-adds, the
// columns are carried every third term, and the loads of three terms are in flight at once (a lone proof has one wave per
// SIMD here and waits on every dependent load).  Both operands are x * 2^256, so a lane's reduced sum is 2^251 * S; the
// factor 2^5 is put back by one product per (polynomial, point) pair at the end.  Same field element as dot_kernel.
// Workgroups of 1024 lanes for a lone proof (the latency form: a few dozen pairs have to fill the chip), of 256 in the
// throughput form, where a 1024-lane workgroup at this register count waits for a whole CU to drain between the other
// provers' kernels.
template <uint32_t DOT_NT>
__global__ __launch_bounds__(DOT_NT) void dot9_kernel(PolySet ps, uint32_t n, const uint32_t* __restrict__ poly_idx,
                                                      const uint32_t* __restrict__ point_idx, const Fe* __restrict__ pw,
                                                      size_t pw_bs, Fe* __restrict__ out, size_t out_bs) {
    __shared__ Fe sh[DOT_NT];
    const uint32_t j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const Fe* p = poly_of(ps, poly_idx[j], b);
    const Fe* w = pw + (size_t)b * pw_bs + (size_t)point_idx[j] * n;
    Dot9<Fr9Params> acc;
    acc.zero();
    uint32_t i = tid;
    for (; i + 2 * DOT_NT < n; i += 3 * DOT_NT) {  // (three terms: what 128 VGPRs hold next to the 17 columns)
        Fe pv[3], wv[3];
#pragma unroll
        for (int t = 0; t < 3; t++) {
            pv[t] = ldg(p + i + t * DOT_NT);
            wv[t] = ldg(w + i + t * DOT_NT);
        }
#pragma unroll
        for (int t = 0; t < 3; t++) acc.mac(f9_unpack(pv[t]), f9_unpack(wv[t]));
        acc.carry();
    }
    for (; i < n; i += DOT_NT) {
        acc.mac(ld9(p + i), ld9(w + i));
        acc.carry();
    }
    sh[tid] = f9_reduce_pack<Fr9Params>(acc.reduce());
    __syncthreads();
    for (uint32_t off = DOT_NT / 2; off > 0; off >>= 1) {
        if (tid < off) sh[tid] = Fr::add(sh[tid], sh[tid + off]);
        __syncthreads();
    }
    if (tid == 0) stg(out + (size_t)b * out_bs + j, Fr::mul(sh[0], Fr9Params::c261_fe()));
}

int poly_dot(zg_ctx* ctx, const PolySet& polys, uint32_t nb, uint32_t n, const uint32_t* d_poly_idx,
             const uint32_t* d_point_idx, const Fe* d_pow, size_t pw_bs, uint32_t count, Fe* d_out, size_t out_bs,
             uint32_t distinct_polys, uint32_t distinct_points) {
    if (!count || !nb) return ZG_OK;
    // algorithmic bytes: a polynomial opened at several points is READ ONCE, and so is each point's power table (round 3
    // charged count * n * 64: more than the kernel moves -- its figure came out above the HBM peak)
    const double dot_bytes = (double)nb * ((double)(distinct_polys ? distinct_polys : count) + (distinct_points ? distinct_points : count)) * n * 32.0;
    // (a lane sums n / 256 terms at most: 2^12 at n = 2^20, inside Dot9's bound of 2^13 terms)
    if (knob(K_LAZY_DOT) != 0 && n <= (1u << 20) && ctx->msm_pair)
        ZG_LAUNCH(ctx, "eval_dot", dot_bytes, dot9_kernel<1024>, dim3(count, nb), dim3(1024), 0, polys, n, d_poly_idx,
                  d_point_idx, d_pow, pw_bs, d_out, out_bs);
    else if (knob(K_LAZY_DOT) != 0 && n <= (1u << 20))
        ZG_LAUNCH(ctx, "eval_dot", dot_bytes, dot9_kernel<256>, dim3(count, nb), dim3(256), 0, polys, n, d_poly_idx,
                  d_point_idx, d_pow, pw_bs, d_out, out_bs);
    else
    ZG_LAUNCH(ctx, "eval_dot", dot_bytes, dot_kernel, dim3(count, nb), dim3(DOT_NT), 0, polys, n, d_poly_idx,
              d_point_idx, d_pow, pw_bs, d_out, out_bs);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ GWC
// out[b][i] = (...((p_0[i]) x + p_1[i]) x + ...) + p_{m-1}[i] with x = pc[b].xn (vanishing::evaluate's h(X))
__global__ __launch_bounds__(256) void horner_combine_kernel(PolySet ps, const ProofConst* __restrict__ pc,
                                                             const uint32_t* __restrict__ list, uint32_t count,
                                                             Fe* __restrict__ out, size_t out_bs, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = blockIdx.y;
    if (i >= n) return;
    const Fe v = pc[b].xn;
    Fe acc = fe_zero();
    for (uint32_t j = 0; j < count; j++) acc = Fr::add(Fr::mul(acc, v), ldg(poly_of(ps, list[j], b) + i));
    stg(out + (size_t)b * out_bs + i, acc);
}

// The same combinations as ONE dot product per coefficient (Dot9, field9.h): sum_j p_j[i] * v^(count - 1 - j) against a
// table of the powers of v in the 2^261 form -- made once per workgroup, lane e takes v^e -- so that a term costs 81
// multiply-adds and the Montgomery reduction is paid once per coefficient instead of once per term; the loads of three
// terms are in flight at once.  Horner's value exactly (the arithmetic is exact), SETS: v = pc[b].v and pc[b].subs[s]
// comes off the constant term (the multiopen argument's lists), else v = pc[b].xn (h(X) from its pieces).
struct HornerSets {
    uint32_t count[HC_MAX_SETS];
};
constexpr uint32_t HC9_MAX = 128;  // longest list the power table holds (longer ones take the Horner kernels)
template <bool SETS>
__global__ __launch_bounds__(256) void combine9_kernel(PolySet ps, const ProofConst* __restrict__ pc,
                                                       const uint32_t* __restrict__ lists, uint32_t list_stride, HornerSets sets,
                                                       Fe* __restrict__ out, size_t out_stride, size_t out_bs, uint32_t n) {
    __shared__ F9 vp[HC9_MAX];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    const uint32_t count = sets.count[s];
    if (threadIdx.x < count) {
        const Fe v = SETS ? pc[b].v : pc[b].xn;
        vp[threadIdx.x] = f9_unpack(Fr::mul(Fr::pow_u64(v, threadIdx.x), Fr9Params::c261_fe()));
    }
    __syncthreads();
    if (i >= n) return;
    const uint32_t* list = lists + (size_t)s * list_stride;
    Dot9<Fr9Params> acc;
    acc.zero();
    uint32_t j = 0;
    for (; j + 3 <= count; j += 3) {
        const Fe p0 = ldg(poly_of(ps, list[j], b) + i), p1 = ldg(poly_of(ps, list[j + 1], b) + i),
                 p2 = ldg(poly_of(ps, list[j + 2], b) + i);
        acc.mac(f9_unpack(p0), vp[count - 1 - j]);
        acc.mac(f9_unpack(p1), vp[count - 2 - j]);
        acc.mac(f9_unpack(p2), vp[count - 3 - j]);
        acc.carry();
    }
    for (; j < count; j++) {
        acc.mac(ld9(poly_of(ps, list[j], b) + i), vp[count - 1 - j]);
        acc.carry();
    }
    Fe r = f9_reduce_pack<Fr9Params>(acc.reduce());
    if (SETS && i == 0) r = Fr::sub(r, pc[b].subs[s]);
    stg(out + (size_t)b * out_bs + (size_t)s * out_stride + i, r);
}

int poly_horner_combine_xn(zg_ctx* ctx, const PolySet& polys, const ProofConst* pc, uint32_t nb, const uint32_t* d_list,
                           uint32_t count, Fe* out, size_t out_bs, uint32_t n) {
    if (!nb) return ZG_OK;
    if (knob(K_LAZY_DOT) != 0 && count <= HC9_MAX) {
        HornerSets sets;
        memset(&sets, 0, sizeof(sets));
        sets.count[0] = count;
        ZG_LAUNCH(ctx, "horner_combine", (double)nb * (count + 1) * n * 32, combine9_kernel<false>, dim3((n + 255) / 256, 1, nb),
                  dim3(256), 0, polys, pc, d_list, 0u, sets, out, (size_t)0, out_bs, n);
        ZG_HIP(hipGetLastError());
        return ZG_OK;
    }
    ZG_LAUNCH(ctx, "horner_combine", (double)nb * (count + 1) * n * 32, horner_combine_kernel, dim3((n + 255) / 256, nb), dim3(256),
              0, polys, pc, d_list, count, out, out_bs, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// the same in pc[b].v for up to HC_MAX_SETS lists at once (GWC: one list per opening point): set s = blockIdx.y of
// proof b = blockIdx.z reads lists + s * list_stride and writes out + b * out_bs + s * out_stride, with
// pc[b].subs[s] taken off the constant term
__global__ __launch_bounds__(256) void horner_combine_sets_kernel(PolySet ps, const ProofConst* __restrict__ pc,
                                                                  const uint32_t* __restrict__ lists, uint32_t list_stride,
                                                                  HornerSets sets, Fe* __restrict__ out, size_t out_stride,
                                                                  size_t out_bs, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    if (i >= n) return;
    const uint32_t* list = lists + (size_t)s * list_stride;
    const uint32_t count = sets.count[s];
    const Fe v = pc[b].v;
    Fe acc = fe_zero();
    for (uint32_t j = 0; j < count; j++) acc = Fr::add(Fr::mul(acc, v), ldg(poly_of(ps, list[j], b) + i));
    if (i == 0) acc = Fr::sub(acc, pc[b].subs[s]);
    stg(out + (size_t)b * out_bs + (size_t)s * out_stride + i, acc);
}

int poly_horner_combine_sets(zg_ctx* ctx, const PolySet& polys, const ProofConst* pc, uint32_t nb, const uint32_t* d_lists,
                             uint32_t list_stride, const uint32_t* counts, uint32_t nsets, Fe* out, size_t out_stride,
                             size_t out_bs, uint32_t n) {
    if (!nsets || !nb) return ZG_OK;
    ZG_REQUIRE(nsets <= HC_MAX_SETS, ZG_ERR_UNSUPPORTED, "poly_horner_combine_sets: %u sets", nsets);
    HornerSets sets;
    memset(&sets, 0, sizeof(sets));
    double total = 0;
    for (uint32_t s = 0; s < nsets; s++) {
        sets.count[s] = counts[s];
        total += counts[s] + 1;
    }
    bool lazy = knob(K_LAZY_DOT) != 0;
    for (uint32_t s = 0; s < nsets; s++) lazy = lazy && counts[s] <= HC9_MAX;
    if (lazy)
        ZG_LAUNCH(ctx, "horner_combine", nb * total * n * 32, combine9_kernel<true>, dim3((n + 255) / 256, nsets, nb), dim3(256), 0,
                  polys, pc, d_lists, list_stride, sets, out, out_stride, out_bs, n);
    else
    ZG_LAUNCH(ctx, "horner_combine", nb * total * n * 32, horner_combine_sets_kernel, dim3((n + 255) / 256, nsets, nb), dim3(256), 0,
              polys, pc, d_lists, list_stride, sets, out, out_stride, out_bs, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ proofs of several circuit instances
// (create_proof's `circuits` slice: the slots of a lock-step batch are the circuits of ONE proof, prove_batch.hip)
//
// The quotient of the whole proof from the slots' own: h[0][i] <- sum_c pc[c].fold_w * h[c][i], one part of the extended
// domain per launch.  A streaming kernel -- nb * 32 B read and 32 B written per row -- in the lazy-sum form: nb products
// of 81 multiply-adds and ONE Montgomery reduction per row (Dot9), the weights unpacked once per workgroup.  The rows may
// be in the nine-limb kernel's 2^5-scaled packed form: the sum is linear, so a plain weight keeps whatever form they have.
__global__ __launch_bounds__(256) void fold_slots_kernel(const ProofConst* __restrict__ pc, uint32_t nb, Fe* __restrict__ h, size_t h_bs,
                                                         uint32_t len) {
    __shared__ F9 w9[FOLD_MAX_SLOTS];
    if (threadIdx.x < nb) w9[threadIdx.x] = f9_unpack(Fr::mul(pc[threadIdx.x].fold_w, Fr9Params::c261_fe()));
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    Dot9<Fr9Params> acc;
    acc.zero();
    uint32_t c = 0;
    for (; c + 3 <= nb; c += 3) {
        const Fe h0 = ldg(h + (size_t)c * h_bs + i), h1 = ldg(h + (size_t)(c + 1) * h_bs + i), h2 = ldg(h + (size_t)(c + 2) * h_bs + i);
        acc.mac(f9_unpack(h0), w9[c]);
        acc.mac(f9_unpack(h1), w9[c + 1]);
        acc.mac(f9_unpack(h2), w9[c + 2]);
        acc.carry();
    }
    for (; c < nb; c++) {
        acc.mac(ld9(h + (size_t)c * h_bs + i), w9[c]);
        acc.carry();
    }
    stg(h + i, f9_reduce_pack<Fr9Params>(acc.reduce()));
}

int poly_fold_slots(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, Fe* h, size_t h_bs, uint32_t len) {
    if (nb <= 1 || !len) return ZG_OK;
    ZG_REQUIRE(nb <= FOLD_MAX_SLOTS, ZG_ERR_UNSUPPORTED, "poly_fold_slots: %u circuits in one proof (max %u)", nb, FOLD_MAX_SLOTS);
    ZG_LAUNCH(ctx, "fold_slots", (double)(nb + 1) * len * 32, fold_slots_kernel, dim3((len + 255) / 256), dim3(256), 0, pc, nb, h, h_bs,
              len);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// GWC over (circuit, polynomial) pairs: set s = blockIdx.y is Horner in pc[0].v over the entries lists[first[s] ..
// first[s] + count[s]) -- entry = slot << 16 | polynomial index -- minus pc[0].subs[s] at X^0, to out + s * out_stride.
// A list has no bound: it is taken in chunks of HC9_MAX terms, each one dot product against the table of v's powers
// (one reduction per chunk, as combine9_kernel), and the chunks are chained by one product with v^HC9_MAX.  The first
// chunk is the short one, so every later chunk is whole.
struct PairSets {
    uint32_t first[HC_MAX_SETS], count[HC_MAX_SETS];
};
__global__ __launch_bounds__(256) void combine_pairs_kernel(PolySet ps, const ProofConst* __restrict__ pc,
                                                            const uint32_t* __restrict__ lists, PairSets sets, Fe* __restrict__ out,
                                                            size_t out_stride, uint32_t n) {
    __shared__ F9 vp[HC9_MAX];
    __shared__ Fe v_chunk;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (threadIdx.x < HC9_MAX) vp[threadIdx.x] = f9_unpack(Fr::mul(Fr::pow_u64(pc[0].v, threadIdx.x), Fr9Params::c261_fe()));
    if (threadIdx.x == HC9_MAX) v_chunk = Fr::pow_u64(pc[0].v, HC9_MAX);
    __syncthreads();
    if (i >= n) return;
    const uint32_t* list = lists + sets.first[s];
    const uint32_t count = sets.count[s];
    auto at = [&](uint32_t j) {
        const uint32_t e = list[j];
        return poly_of(ps, e & 0xffffu, e >> 16) + i;
    };
    Fe r = fe_zero();
    uint32_t chunk = count % HC9_MAX ? count % HC9_MAX : HC9_MAX;
    for (uint32_t j0 = 0; j0 < count; j0 += chunk, chunk = HC9_MAX) {
        Dot9<Fr9Params> acc;
        acc.zero();
        uint32_t t = 0;
        for (; t + 3 <= chunk; t += 3) {
            const Fe p0 = ldg(at(j0 + t)), p1 = ldg(at(j0 + t + 1)), p2 = ldg(at(j0 + t + 2));
            acc.mac(f9_unpack(p0), vp[chunk - 1 - t]);
            acc.mac(f9_unpack(p1), vp[chunk - 2 - t]);
            acc.mac(f9_unpack(p2), vp[chunk - 3 - t]);
            acc.carry();
        }
        for (; t < chunk; t++) {
            acc.mac(f9_unpack(ldg(at(j0 + t))), vp[chunk - 1 - t]);
            acc.carry();
        }
        const Fe part = f9_reduce_pack<Fr9Params>(acc.reduce());
        r = j0 ? Fr::add(Fr::mul(r, v_chunk), part) : part;
    }
    if (i == 0) r = Fr::sub(r, pc[0].subs[s]);
    stg(out + (size_t)s * out_stride + i, r);
}

int poly_combine_pairs(zg_ctx* ctx, const PolySet& polys, const ProofConst* pc, const uint32_t* d_lists, const uint32_t* firsts,
                       const uint32_t* counts, uint32_t nsets, Fe* out, size_t out_stride, uint32_t n) {
    if (!nsets) return ZG_OK;
    ZG_REQUIRE(nsets <= HC_MAX_SETS, ZG_ERR_UNSUPPORTED, "poly_combine_pairs: %u sets", nsets);
    PairSets sets;
    memset(&sets, 0, sizeof(sets));
    double total = 0;
    for (uint32_t s = 0; s < nsets; s++) {
        sets.first[s] = firsts[s];
        sets.count[s] = counts[s];
        total += counts[s] + 1;
    }
    ZG_LAUNCH(ctx, "combine_pairs", total * n * 32, combine_pairs_kernel, dim3((n + 255) / 256, nsets), dim3(256), 0, polys, pc,
              d_lists, sets, out, out_stride, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// SHPLONK's two weighted combinations: output o = blockIdx.y of proof b = blockIdx.z is
//   sum_t coef[b][first[o] + t] * poly(lists[first[o] + t])  [+ coef[b][first[o] + count[o]] * extra[b]]  -  corr[b][o]
// over list entries of combine_pairs_kernel's form (slot << 16 | polynomial index; the slot counts from b, so a batch of
// single proofs lists slot 0 and a proof of several circuits is launched as b = 0 alone).  The coefficients differ per
// proof and per term -- y^j v^i c_(i,r) for the numerators, y^j v^i z_i / z_0 for L -- so they live in device memory beside
// ProofConst[b], already times 2^5 and unpacked by the host; every lane of a workgroup reads the same one.  The lazy sum
// of the siblings: 81 multiply-adds a term, one reduction per chunk of HC9_MAX terms.  corr: the interpolants' share,
// ncorr <= PC_MAX_POINTS low coefficients per output (one, the constant, for L).
struct WeightedOuts {
    uint32_t first[HC_MAX_SETS], count[HC_MAX_SETS];
};
__global__ __launch_bounds__(256) void combine_weighted_kernel(PolySet ps, const uint32_t* __restrict__ lists,
                                                               const F9* __restrict__ coef, size_t coef_bs, WeightedOuts outs,
                                                               const Fe* __restrict__ corr, uint32_t ncorr, size_t corr_bs,
                                                               const Fe* __restrict__ extra, size_t extra_bs, Fe* __restrict__ out,
                                                               size_t out_stride, size_t out_bs, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, o = blockIdx.y, b = blockIdx.z;
    if (i >= n) return;
    const uint32_t* list = lists + outs.first[o];
    const F9* cf = coef + (size_t)b * coef_bs + outs.first[o];
    const uint32_t count = outs.count[o];
    auto at = [&](uint32_t j) {
        const uint32_t e = list[j];
        return poly_of(ps, e & 0xffffu, (e >> 16) + b) + i;
    };
    Fe r = fe_zero();
    for (uint32_t j0 = 0; j0 < count; j0 += HC9_MAX) {
        const uint32_t chunk = count - j0 < HC9_MAX ? count - j0 : HC9_MAX;
        Dot9<Fr9Params> acc;
        acc.zero();
        uint32_t t = 0;
        for (; t + 3 <= chunk; t += 3) {
            const Fe p0 = ldg(at(j0 + t)), p1 = ldg(at(j0 + t + 1)), p2 = ldg(at(j0 + t + 2));
            acc.mac(f9_unpack(p0), cf[j0 + t]);
            acc.mac(f9_unpack(p1), cf[j0 + t + 1]);
            acc.mac(f9_unpack(p2), cf[j0 + t + 2]);
            acc.carry();
        }
        for (; t < chunk; t++) {
            acc.mac(f9_unpack(ldg(at(j0 + t))), cf[j0 + t]);
            acc.carry();
        }
        r = Fr::add(r, f9_reduce_pack<Fr9Params>(acc.reduce()));
    }
    if (extra) {
        Dot9<Fr9Params> acc;
        acc.zero();
        acc.mac(f9_unpack(ldg(extra + (size_t)b * extra_bs + i)), cf[count]);
        acc.carry();
        r = Fr::add(r, f9_reduce_pack<Fr9Params>(acc.reduce()));
    }
    if (i < ncorr) r = Fr::sub(r, ldg(corr + (size_t)b * corr_bs + (size_t)o * ncorr + i));
    stg(out + (size_t)b * out_bs + (size_t)o * out_stride + i, r);
}

int poly_combine_weighted(zg_ctx* ctx, const PolySet& polys, uint32_t nb, const uint32_t* d_lists, const uint32_t* firsts,
                          const uint32_t* counts, uint32_t nouts, const F9* d_coef, size_t coef_bs, const Fe* d_corr, uint32_t ncorr,
                          size_t corr_bs, const Fe* extra, size_t extra_bs, Fe* out, size_t out_stride, size_t out_bs, uint32_t n) {
    if (!nouts || !nb || !n) return ZG_OK;
    ZG_REQUIRE(nouts <= HC_MAX_SETS && ncorr <= PC_MAX_POINTS, ZG_ERR_UNSUPPORTED, "poly_combine_weighted: %u outputs", nouts);
    WeightedOuts outs;
    memset(&outs, 0, sizeof(outs));
    double total = 0;
    for (uint32_t o = 0; o < nouts; o++) {
        outs.first[o] = firsts[o];
        outs.count[o] = counts[o];
        total += counts[o] + (extra ? 2 : 1);
    }
    ZG_LAUNCH(ctx, "combine_weighted", (double)nb * total * n * 32, combine_weighted_kernel, dim3((n + 255) / 256, nouts, nb), dim3(256),
              0, polys, d_lists, d_coef, coef_bs, outs, d_corr, ncorr, corr_bs, extra, extra_bs, out, out_stride, out_bs, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// SHPLONK's h1: out[b][i] = sum_(s < rows) in[b][s][i] -- the per-point quotients, canonical values, into one polynomial
__global__ __launch_bounds__(256) void sum_rows_kernel(const Fe* __restrict__ in, size_t in_stride, size_t in_bs, uint32_t rows,
                                                       Fe* __restrict__ out, size_t out_bs, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    const Fe* p = in + (size_t)b * in_bs + i;
    Fe r = ldg(p);
    for (uint32_t s = 1; s < rows; s++) r = Fr::add(r, ldg(p + (size_t)s * in_stride));
    stg(out + (size_t)b * out_bs + i, r);
}

int poly_sum_rows(zg_ctx* ctx, uint32_t nb, const Fe* in, size_t in_stride, size_t in_bs, uint32_t rows, Fe* out, size_t out_bs,
                  uint32_t n) {
    if (!nb || !rows || !n) return ZG_OK;
    ZG_LAUNCH(ctx, "sum_rows", (double)nb * (rows + 1) * n * 32, sum_rows_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, in, in_stride,
              in_bs, rows, out, out_bs, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// zg_fr_lincomb_dev: out[i] = sum_j coeff_j * poly_j[i] for polynomials that live anywhere in HBM (the caller-run
// create_proof's sum x^(n i) h_i and sum v^i p_i - eval).  The lazy sum of combine_pairs_kernel -- 81 multiply-adds per
// term, one Montgomery reduction per chunk -- with the chunk's addresses and coefficients in the KERNEL ARGUMENTS: every
// lane reads term t of the same chunk, so both come through the scalar unit, nothing is uploaded and the entry queues
// without waiting.  The coefficients arrive times 2^5 and unpacked (the host does it once per launch, not every lane).
// Bound: Dot9::reduce takes a sum below 2^521; a term of canonical operands is below r^2 < 2^507.2, so 2^13 terms fit --
// the chunk, LC_CHUNK = 64 terms (what 4 KB of kernel arguments hold at 44 B a term), is far inside it.  Later chunks add
// what the earlier ones left in `out` (canonical after every launch).
constexpr uint32_t LC_CHUNK = ZG_LINCOMB_CHUNK;
struct LincombArgs {
    const Fe* poly[LC_CHUNK];
    F9 w9[LC_CHUNK];  // coefficient * 2^261 mod r, unpacked
    Fe sub0;
    uint32_t count, first, has_sub;
};
static_assert(sizeof(LincombArgs) + 64 <= 4096, "LincombArgs must fit the kernel-argument segment");
static_assert(LC_CHUNK <= (1u << 13), "one reduction per chunk: Dot9::reduce's bound");
__global__ __launch_bounds__(256) void lincomb_kernel(LincombArgs a, Fe* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Dot9<Fr9Params> acc;
    acc.zero();
    uint32_t t = 0;
    for (; t + 3 <= a.count; t += 3) {
        const Fe p0 = ldg(a.poly[t] + i), p1 = ldg(a.poly[t + 1] + i), p2 = ldg(a.poly[t + 2] + i);
        acc.mac(f9_unpack(p0), a.w9[t]);
        acc.mac(f9_unpack(p1), a.w9[t + 1]);
        acc.mac(f9_unpack(p2), a.w9[t + 2]);
        acc.carry();
    }
    for (; t < a.count; t++) {
        acc.mac(f9_unpack(ldg(a.poly[t] + i)), a.w9[t]);
        acc.carry();
    }
    Fe r = f9_reduce_pack<Fr9Params>(acc.reduce());
    if (!a.first) r = Fr::add(ldg(out + i), r);
    if (a.has_sub && i == 0) r = Fr::sub(r, a.sub0);
    stg(out + i, r);
}

int poly_lincomb(zg_ctx* ctx, const Fe* const* polys, const Fe* coeffs, size_t count, uint32_t n, const Fe* sub0, Fe* out) {
    if (!n) return ZG_OK;
    size_t j0 = 0;
    do {
        LincombArgs a;
        memset(&a, 0, sizeof(a));
        a.count = (uint32_t)std::min<size_t>(LC_CHUNK, count - j0);
        a.first = j0 == 0;
        a.has_sub = j0 == 0 && sub0 != nullptr;
        if (a.has_sub) a.sub0 = *sub0;
        for (uint32_t t = 0; t < a.count; t++) {
            a.poly[t] = polys[j0 + t];
            a.w9[t] = f9_unpack(Fr::mul(coeffs[j0 + t], Fr9Params::c261_fe()));
        }
        ZG_LAUNCH(ctx, "lincomb", ((double)a.count + (a.first ? 1 : 2)) * n * 32, lincomb_kernel, dim3((n + 255) / 256), dim3(256), 0, a,
                  out, n);
        j0 += a.count;
    } while (j0 < count);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int poly_one_const(zg_ctx* ctx, WsScope& ws, const ProofConst& hc, ProofConst** out) {
    ProofConst* d = ws.get<ProofConst>(1);
    if (!d) return ZG_ERR_OOM;
    ZG_HIP(hipMemcpyAsync(d, &hc, sizeof(hc), hipMemcpyHostToDevice, ctx->stream));
    ZG_HIP(hipStreamSynchronize(ctx->stream));  // (hc is the caller's stack memory)
    *out = d;
    return ZG_OK;
}

// kate_division: q_i = a_{i+1} + z q_{i+1} (i = n-2 .. 0, q_{n-1} = 0) -- upstream's one-core recurrence.  Strip form,
// one workgroup per polynomial: lane l owns the strip [l S, (l + 1) S) of coefficients, S = n / lanes.
//   pass A   the strip's own contribution at its first element, H_l = sum_{i in strip} a_{i+1} z^(i - l S) (Horner,
//            S products);
//   scan     the true values at the strip starts obey the same recurrence with ratio z^S over the lanes,
//            Q_l = H_l + z^S Q_{l+1}: a weighted Hillis-Steele suffix scan through LDS (two products per step);
//   pass B   the recurrence again, now started from the true carry Q_{l+1}: every q_i of the strip, S products.
// About 3.3 products per coefficient where the block-scan form (three launches) spent ~30: 16 in its scan steps, up
// to 16 in the z^(256 - tid) of its apply pass.  Batched over (proof, point set): set s of proof b divides by
// X - pc[b].points[slot[s]].
constexpr uint32_t KD_LANES = 1024;
struct KdSlots {
    uint32_t slot[HC_MAX_SETS];
};

__global__ __launch_bounds__(KD_LANES) void kd_strip_kernel(const ProofConst* __restrict__ pc, KdSlots slots,
                                                            const Fe* __restrict__ a, size_t a_stride, size_t a_bs,
                                                            Fe* __restrict__ q, size_t q_stride, size_t q_bs, uint32_t n,
                                                            uint32_t lanes, uint32_t strip) {
    __shared__ Fe sh[KD_LANES];
    const uint32_t tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const Fe* ap = a + (size_t)b * a_bs + (size_t)s * a_stride;
    Fe* qp = q + (size_t)b * q_bs + (size_t)s * q_stride;
    const Fe z = pc[b].points[slots.slot[s]];
    const uint32_t i0 = tid * strip;
    const uint32_t i1 = tid < lanes ? (i0 + strip < n ? i0 + strip : n) : i0;  // (lanes beyond the polynomial: empty strips)
    Fe acc = fe_zero();
    for (uint32_t i = i1; i-- > i0;) {
        acc = Fr::mul(z, acc);
        if (i + 1 < n) acc = Fr::add(acc, ldg(ap + i + 1));
    }
    sh[tid] = acc;
    __syncthreads();
    Fe w = Fr::pow_u64(z, strip);  // z^S, squared at every step
    for (uint32_t off = 1; off < KD_LANES; off <<= 1) {
        Fe t = fe_zero();
        const bool has = tid + off < KD_LANES;
        if (has) t = sh[tid + off];
        __syncthreads();
        if (has) sh[tid] = Fr::add(sh[tid], Fr::mul(w, t));
        w = Fr::sqr(w);
        __syncthreads();
    }
    acc = tid + 1 < KD_LANES ? sh[tid + 1] : fe_zero();  // q at the first coefficient of the strip above
    for (uint32_t i = i1; i-- > i0;) {
        acc = Fr::mul(z, acc);
        if (i + 1 < n) acc = Fr::add(acc, ldg(ap + i + 1));
        stg(qp + i, acc);
    }
}

// ---- latency form (a lone proof): block-local weighted scans, coalesced accesses, three short launches -- ~30 products
// per coefficient, but 70 us against the strip form's 130 us when four polynomials are all there is
constexpr uint32_t KD_BLOCK = 256;

__global__ __launch_bounds__(KD_BLOCK) void kd_local_kernel(const ProofConst* __restrict__ pc, KdSlots slots,
                                                            const Fe* __restrict__ a, size_t a_stride, size_t a_bs,
                                                            Fe* __restrict__ loc, Fe* __restrict__ heads, uint32_t n,
                                                            uint32_t nblk) {
    __shared__ Fe sh[KD_BLOCK];
    const uint32_t tid = threadIdx.x, blk = blockIdx.x, s = blockIdx.y, b = blockIdx.z;
    const uint32_t q = b * gridDim.y + s;
    const uint32_t i = blk * KD_BLOCK + tid;
    const Fe* ap = a + (size_t)b * a_bs + (size_t)s * a_stride;
    Fe v = (i + 1 < n) ? ldg(ap + i + 1) : fe_zero();
    sh[tid] = v;
    __syncthreads();
    Fe w = pc[b].points[slots.slot[s]];  // z^off
    for (uint32_t off = 1; off < KD_BLOCK; off <<= 1) {
        Fe t = fe_zero();
        const bool has = tid + off < KD_BLOCK;
        if (has) t = sh[tid + off];
        __syncthreads();
        if (has) sh[tid] = Fr::add(sh[tid], Fr::mul(w, t));
        w = Fr::sqr(w);
        __syncthreads();
    }
    if (i < n) stg(loc + (size_t)q * n + i, sh[tid]);
    if (tid == 0) stg(heads + (size_t)q * nblk + blk, sh[0]);
}

// heads[blk] <- sum_{blk' > blk} heads[blk'] * (z^256)^(blk' - blk - 1): the carry entering block blk from above
__global__ __launch_bounds__(1024) void kd_heads_kernel(const ProofConst* __restrict__ pc, KdSlots slots, uint32_t nsets,
                                                        Fe* __restrict__ heads, uint32_t nblk) {
    __shared__ Fe sh[1024];
    const uint32_t tid = threadIdx.x, q = blockIdx.x;
    const uint32_t b = q / nsets, s = q % nsets;
    Fe* hp = heads + (size_t)q * nblk;
    sh[tid] = tid < nblk ? ldg(hp + tid) : fe_zero();
    __syncthreads();
    Fe w = Fr::pow_u64(pc[b].points[slots.slot[s]], KD_BLOCK);
    uint32_t span = 64;  // (entries at and beyond nblk are zero: the scan only has to span the block heads)
    while (span < nblk) span <<= 1;
    for (uint32_t off = 1; off < span; off <<= 1) {
        Fe t = fe_zero();
        const bool has = tid + off < span;
        if (has) t = sh[tid + off];
        __syncthreads();
        if (has) sh[tid] = Fr::add(sh[tid], Fr::mul(w, t));
        w = Fr::sqr(w);
        __syncthreads();
    }
    Fe carry = tid + 1 < span ? sh[tid + 1] : fe_zero();
    __syncthreads();
    if (tid < nblk) stg(hp + tid, carry);
}

__global__ __launch_bounds__(KD_BLOCK) void kd_apply_kernel(const ProofConst* __restrict__ pc, KdSlots slots,
                                                            const Fe* __restrict__ loc, const Fe* __restrict__ heads,
                                                            Fe* __restrict__ qo, size_t q_stride, size_t q_bs, uint32_t n,
                                                            uint32_t nblk) {
    const uint32_t tid = threadIdx.x, blk = blockIdx.x, s = blockIdx.y, b = blockIdx.z;
    const uint32_t q = b * gridDim.y + s;
    const uint32_t i = blk * KD_BLOCK + tid;
    if (i >= n) return;
    Fe v = ldg(loc + (size_t)q * n + i);
    Fe carry = ldg(heads + (size_t)q * nblk + blk);
    if (!fe_is_zero(carry)) v = Fr::add(v, Fr::mul(Fr::pow_u64(pc[b].points[slots.slot[s]], KD_BLOCK - tid), carry));
    stg(qo + (size_t)b * q_bs + (size_t)s * q_stride + i, v);
}

size_t poly_kate_tmp_elems(uint32_t n, uint32_t batch) {  // (the latency form's scratch; the strip form needs none)
    size_t nblk = (n + KD_BLOCK - 1) / KD_BLOCK;
    return (size_t)batch * n + (size_t)batch * nblk + batch;
}

int poly_kate_division(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, const uint32_t* slots, uint32_t nsets, const Fe* a,
                       size_t a_stride, size_t a_bs, Fe* q, size_t q_stride, size_t q_bs, Fe* tmp, uint32_t n) {
    if (!nb || !nsets || !n) return ZG_OK;
    ZG_REQUIRE(nsets <= HC_MAX_SETS, ZG_ERR_UNSUPPORTED, "kate division: %u point sets", nsets);
    KdSlots ks;
    memset(&ks, 0, sizeof(ks));
    for (uint32_t s = 0; s < nsets; s++) {
        ZG_REQUIRE(slots[s] <= PC_U_SLOT, ZG_ERR_INVALID_ARG, "kate division: point slot %u", slots[s]);
        ks.slot[s] = slots[s];
    }
    if (ctx->msm_pair && n <= (1u << 18)) {  // latency form (tmp per poly_kate_tmp_elems(n, nb * nsets))
        const uint32_t nblk = (n + KD_BLOCK - 1) / KD_BLOCK;
        const uint32_t m = nb * nsets;
        Fe* loc = tmp;
        Fe* heads = loc + (size_t)m * n;
        const double bytes = (double)m * n * 64;
        ZG_LAUNCH(ctx, "kate_local", bytes, kd_local_kernel, dim3(nblk, nsets, nb), dim3(KD_BLOCK), 0, pc, ks, a, a_stride, a_bs, loc,
                  heads, n, nblk);
        // (as many lanes as block heads, a power of two from 64: at n = 2^14 one wave, whose barriers cost nothing)
        uint32_t hl = 64;
        while (hl < nblk) hl <<= 1;
        ZG_LAUNCH(ctx, "kate_heads", (double)m * nblk * 64, kd_heads_kernel, dim3(m), dim3(hl), 0, pc, ks, nsets, heads, nblk);
        ZG_LAUNCH(ctx, "kate_apply", bytes, kd_apply_kernel, dim3(nblk, nsets, nb), dim3(KD_BLOCK), 0, pc, ks, loc, heads, q, q_stride,
                  q_bs, n, nblk);
        ZG_HIP(hipGetLastError());
        return ZG_OK;
    }
    const uint32_t lanes = n < KD_LANES ? n : KD_LANES;
    const uint32_t strip = (n + lanes - 1) / lanes;
    ZG_LAUNCH(ctx, "kate_division", (double)nb * nsets * n * 64, kd_strip_kernel, dim3(nsets, nb), dim3(KD_LANES), 0, pc, ks, a,
              a_stride, a_bs, q, q_stride, q_bs, n, lanes, strip);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ------------------------------------------------------------------ l_0 / l_last / l_blind
__global__ void l_init_kernel(Fe* l0, Fe* llast, Fe* lblind, uint32_t n, uint32_t bf) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe one = Fr::one(), zero = fe_zero();
    stg(l0 + i, i == 0 ? one : zero);
    stg(llast + i, i == n - bf - 1 ? one : zero);
    stg(lblind + i, i >= n - bf ? one : zero);
}
int poly_l_cosets_init(zg_ctx* ctx, Fe* l0, Fe* llast, Fe* lblind, uint32_t n, uint32_t bf) {
    ZG_LAUNCH(ctx, "l_init", 0, l_init_kernel, dim3((n + 255) / 256), dim3(256), 0, l0, llast, lblind, n, bf);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}
__global__ void lactive_kernel(Fe* lactive, const Fe* llast, const Fe* lblind, uint32_t en, Fe one) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < en) stg(lactive + i, Fr::sub(one, Fr::add(ldg(llast + i), ldg(lblind + i))));
}
int poly_lactive(zg_ctx* ctx, Fe* lactive, const Fe* llast, const Fe* lblind, uint32_t en, bool hat) {
    const Fe one = hat ? Fr::mul(Fr::one(), Fr9Params::c261_fe()) : Fr::one();  // "1" in the slabs' form
    ZG_LAUNCH(ctx, "lactive", 0, lactive_kernel, dim3((en + 255) / 256), dim3(256), 0, lactive, llast, lblind, en, one);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

__global__ void scale_kernel(const Fe* in, Fe* out, size_t count, Fe factor) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) stg(out + i, Fr::mul(ldg(in + i), factor));
}
int poly_scale(zg_ctx* ctx, const Fe* in, Fe* out, size_t count, const Fe& factor) {
    if (!count) return ZG_OK;
    ZG_LAUNCH(ctx, "scale", (double)count * 64, scale_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, in, out,
              count, factor);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ---- interpolation across the two cosets of the split extended domain (prove_batch.hip); proof b = blockIdx.y
__global__ void fold_kernel(const Fe* a, size_t a_bs, uint32_t len, uint32_t parts, Fe e, Fe* out, size_t out_bs) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= len) return;
    a += (size_t)blockIdx.y * a_bs;
    Fe acc = ldg(a + (size_t)(parts - 1) * len + r);
    for (uint32_t q = parts - 1; q-- > 0;) acc = Fr::add(Fr::mul(acc, e), ldg(a + (size_t)q * len + r));
    stg(out + (size_t)blockIdx.y * out_bs + r, acc);
}
int poly_fold(zg_ctx* ctx, uint32_t nb, const Fe* a, size_t a_bs, uint32_t len, uint32_t parts, const Fe& e, Fe* out,
              size_t out_bs) {
    ZG_REQUIRE(parts >= 1 && len >= 1, ZG_ERR_INVALID_ARG, "poly_fold: %u parts of %u", parts, len);
    if (!nb) return ZG_OK;
    ZG_LAUNCH(ctx, "fold", (double)nb * (parts + 1) * len * 32, fold_kernel, dim3((len + 255) / 256, nb), dim3(256), 0, a, a_bs, len,
              parts, e, out, out_bs);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}
__global__ void diff_scale_kernel(const Fe* u, size_t u_bs, Fe cu, const Fe* v, size_t v_bs, Fe scale, Fe* out, size_t out_bs,
                                  uint32_t len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i < len)
        stg(out + (size_t)b * out_bs + i,
            Fr::mul(Fr::sub(Fr::mul(ldg(u + (size_t)b * u_bs + i), cu), ldg(v + (size_t)b * v_bs + i)), scale));
}
int poly_diff_scale(zg_ctx* ctx, uint32_t nb, const Fe* u, size_t u_bs, const Fe& cu, const Fe* v, size_t v_bs, const Fe& scale,
                    Fe* out, size_t out_bs, uint32_t len) {
    if (!nb) return ZG_OK;
    ZG_LAUNCH(ctx, "diff_scale", (double)nb * len * 96, diff_scale_kernel, dim3((len + 255) / 256, nb), dim3(256), 0, u, u_bs, cu, v,
              v_bs, scale, out, out_bs, len);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}
__global__ void split_combine_kernel(Fe* h, size_t h_bs, const Fe* bq, size_t b_bs, uint32_t len, Fe c1, uint32_t hi_at) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= len) return;
    h += (size_t)blockIdx.y * h_bs;
    const Fe bj = ldg(bq + (size_t)blockIdx.y * b_bs + j);
    stg(h + j, Fr::sub(ldg(h + j), Fr::mul(c1, bj)));
    stg(h + hi_at + j, bj);
}
int poly_split_combine(zg_ctx* ctx, uint32_t nb, Fe* h, size_t h_bs, const Fe* b, size_t b_bs, uint32_t len, const Fe& c1,
                       uint32_t hi_at) {
    if (!nb) return ZG_OK;
    ZG_LAUNCH(ctx, "split_combine", (double)nb * len * 128, split_combine_kernel, dim3((len + 255) / 256, nb), dim3(256), 0, h, h_bs,
              b, b_bs, len, c1, hi_at);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// ---- challenges as columns: grid (row blocks, challenges of the phase, proofs).  A challenge's rows are, one behind the
// other, its n values, its n coefficients and its slab on each part in use; a thread stores one element (32 bytes).
__global__ void challenge_fill_kernel(ChalFill f) {
    const uint32_t j = f.chal[blockIdx.y], b = blockIdx.z;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const Fe* v = f.vals + ((size_t)b * f.stride + j) * 2;
    if (i < f.n) {
        stg(f.val + (size_t)b * f.val_bs + (size_t)(f.col0 + j) * f.n + i, ldg(v));
        return;
    }
    i -= f.n;
    if (i < f.n) {
        stg(f.coef + (size_t)b * f.coef_bs + (size_t)j * f.n + i, i == 0 ? ldg(v) : fe_zero());
        return;
    }
    i -= f.n;
    for (uint32_t d = 0; d < f.nparts; d++) {
        if (i < f.en[d]) {
            stg(f.cos[d] + (size_t)b * f.cos_bs[d] + (size_t)j * f.en[d] + i, ldg(v + 1));
            return;
        }
        i -= f.en[d];
    }
}
int poly_challenge_fill(zg_ctx* ctx, const ChalFill& f, uint32_t nb) {
    if (!nb || !f.count) return ZG_OK;
    size_t rows = (size_t)2 * f.n;
    for (uint32_t d = 0; d < f.nparts; d++) rows += f.en[d];
    ZG_REQUIRE(f.count <= ZG_MAX_CHALLENGES && f.nparts <= 2 && nb <= 65535 && rows < (1ull << 31), ZG_ERR_INVALID_ARG, "challenge_fill: %u challenges, %zu rows", f.count, rows);
    ZG_LAUNCH(ctx, "challenge_fill", (double)nb * f.count * rows * 32, challenge_fill_kernel, dim3((unsigned)((rows + 255) / 256), f.count, nb),
              dim3(256), 0, f);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

// ------------------------------------------------------------------ context-level entries (no prover): host-facing forms
// of the launch helpers above
extern "C" {

int zg_grand_product_dev(zg_ctx* ctx, const void* d_num, const void* d_den, const zg_fr* z0, size_t n, void* d_z) {
    ZG_REQUIRE(ctx && d_num && d_den && d_z && z0, ZG_ERR_INVALID_ARG, "zg_grand_product_dev: null argument");
    ZG_REQUIRE(n < (1u << 28), ZG_ERR_UNSUPPORTED, "zg_grand_product_dev: n too large");
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    Fe* tmp = ws.get<Fe>(poly_grand_product_tmp_elems((uint32_t)n, 1) + 1);
    if (ws.failed) return ZG_ERR_OOM;
    Fe* z0d = tmp + poly_grand_product_tmp_elems((uint32_t)n, 1);
    ZG_HIP(hipMemcpyAsync(z0d, z0, 32, hipMemcpyHostToDevice, ctx->stream));
    ZG_TRY(poly_grand_product(ctx, (const Fe*)d_num, (const Fe*)d_den, z0d, (Fe*)d_z, tmp, (uint32_t)n, 1, 0, 0));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    return ZG_OK;
}

// Host-pointer form of the same (lookup::prover::commit_product / permutation::prover::commit's running product):
// z[0] = z0, z[i+1] = z[i] * num[i] / den[i] with BatchInvert's rule for a zero denominator (ratio 0); z has n entries.
int zg_grand_product(zg_ctx* ctx, const zg_fr* num, const zg_fr* den, const zg_fr* z0, size_t n, zg_fr* z) {
    ZG_REQUIRE(ctx && num && den && z0 && z, ZG_ERR_INVALID_ARG, "zg_grand_product: null argument");
    ZG_REQUIRE(n >= 1 && n < (1u << 28), ZG_ERR_UNSUPPORTED, "zg_grand_product: n out of range");
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    Fe* d = ws.get<Fe>(3 * n);
    if (ws.failed) return ZG_ERR_OOM;
    ZG_HIP(hipMemcpyAsync(d, num, n * 32, hipMemcpyHostToDevice, ctx->stream));
    ZG_HIP(hipMemcpyAsync(d + n, den, n * 32, hipMemcpyHostToDevice, ctx->stream));
    ZG_TRY(zg_grand_product_dev(ctx, d, d + n, z0, n, d + 2 * n));
    ZG_HIP(hipMemcpy(z, d + 2 * n, n * 32, hipMemcpyDeviceToHost));
    return ZG_OK;
}

int zg_eval_polys_dev(zg_ctx* ctx, const void* d_polys, size_t stride_elems, size_t n, const uint32_t* poly_index,
                      const zg_fr* points, size_t count, zg_fr* out) {
    ZG_REQUIRE(ctx && d_polys && poly_index && points && out, ZG_ERR_INVALID_ARG, "zg_eval_polys_dev: null argument");
    if (!count) return ZG_OK;
    ZG_REQUIRE(stride_elems == n || count == 0, ZG_ERR_UNSUPPORTED, "zg_eval_polys_dev: stride %zu != n %zu", stride_elems, n);
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    // the pairs are served PC_MAX_POINTS at a time, every pair with a powers row of its own (callers with shared
    // points should use the prover)
    Fe* pw = ws.get<Fe>((size_t)PC_MAX_POINTS * n);
    uint32_t* di = ws.get<uint32_t>(2 * PC_MAX_POINTS);
    Fe* de = ws.get<Fe>(PC_MAX_POINTS);
    ProofConst* dpc = ws.get<ProofConst>(1);
    if (ws.failed) return ZG_ERR_OOM;
    PolySet ps;
    ps.sh = (const Fe*)d_polys; ps.pp = nullptr; ps.nsh = 0xffffffffu; ps.n = n; ps.pp_bs = 0;
    for (size_t c0 = 0; c0 < count; c0 += PC_MAX_POINTS) {
        const uint32_t m = (uint32_t)std::min<size_t>(PC_MAX_POINTS, count - c0);
        ProofConst hc;
        memset(&hc, 0, sizeof(hc));
        uint32_t idx[2 * PC_MAX_POINTS];
        for (uint32_t i = 0; i < m; i++) {
            hc.points[i] = to_fe(&points[c0 + i]);
            idx[i] = poly_index[c0 + i];
            idx[m + i] = i;
        }
        ZG_HIP(hipMemcpyAsync(dpc, &hc, sizeof(hc), hipMemcpyHostToDevice, ctx->stream));
        ZG_HIP(hipMemcpyAsync(di, idx, 2 * m * 4, hipMemcpyHostToDevice, ctx->stream));
        ZG_HIP(hipStreamSynchronize(ctx->stream));  // (hc and idx are stack memory)
        ZG_TRY(poly_powers(ctx, dpc, 1, m, (uint32_t)n, pw, 0));
        ZG_TRY(poly_dot(ctx, ps, 1, (uint32_t)n, di, di + m, pw, 0, m, de, 0));
        ZG_HIP(hipMemcpyAsync(out + c0, de, m * 32, hipMemcpyDeviceToHost, ctx->stream));
        ZG_HIP(hipStreamSynchronize(ctx->stream));
    }
    return ZG_OK;
}

int zg_kate_division_dev(zg_ctx* ctx, const void* d_a, size_t n, const zg_fr* z, void* d_q) {
    ZG_REQUIRE(ctx && d_a && z && d_q && n >= 1, ZG_ERR_INVALID_ARG, "zg_kate_division_dev: bad argument");
    ZG_ENTER(ctx);
    ZG_REQUIRE(n < (1u << 28), ZG_ERR_UNSUPPORTED, "zg_kate_division_dev: n too large");
    WsScope ws(ctx);
    Fe* tmp = ws.get<Fe>(poly_kate_tmp_elems((uint32_t)n, 1));
    ProofConst* dpc = ws.get<ProofConst>(1);
    if (ws.failed) return ZG_ERR_OOM;
    ProofConst hc;
    memset(&hc, 0, sizeof(hc));
    hc.points[0] = to_fe(z);
    ZG_HIP(hipMemcpyAsync(dpc, &hc, sizeof(hc), hipMemcpyHostToDevice, ctx->stream));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    const uint32_t slot0 = 0;
    ZG_TRY(poly_kate_division(ctx, dpc, 1, &slot0, 1, (const Fe*)d_a, n, 0, (Fe*)d_q, n, 0, tmp, (uint32_t)n));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    return ZG_OK;
}

// ---- the arithmetic level on device pointers: thin host code over the prover's own launch helpers

// lookup::prover::permute_expression_pair: the prover's path (prove_batch.hip, permuted_queue) for ONE pair -- canonical
// keys with the sentinel padding, the bitonic sort of both columns, the scan-built s' (sort.hip) -- then back to
// Montgomery form on the usable rows and zeros behind them.
int zg_permute_expression_pair_dev(zg_ctx* ctx, const void* d_input, const void* d_table, uint32_t k, uint32_t usable,
                                   void* d_permuted_input, void* d_permuted_table) {
    ZG_REQUIRE(ctx && d_input && d_table && d_permuted_input && d_permuted_table, ZG_ERR_INVALID_ARG,
               "zg_permute_expression_pair_dev: null argument");
    ZG_REQUIRE(k >= 4 && k <= 20, ZG_ERR_UNSUPPORTED, "zg_permute_expression_pair_dev: k=%u outside 4..20", k);
    const uint32_t n = 1u << k;
    ZG_REQUIRE(usable >= 1 && usable <= n, ZG_ERR_INVALID_ARG, "zg_permute_expression_pair_dev: %u usable rows of %u", usable, n);
    ZG_REQUIRE(d_permuted_input != d_input && d_permuted_input != d_table && d_permuted_table != d_input &&
                   d_permuted_table != d_table && d_permuted_input != d_permuted_table,
               ZG_ERR_INVALID_ARG, "zg_permute_expression_pair_dev: an output aliases another column");
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    Fe* raw = ws.get<Fe>((size_t)4 * n);  // input keys -> a', table keys, s', the left-over list
    uint32_t* u32 = ws.get<uint32_t>((size_t)2 * n + 3);
    if (ws.failed) return ZG_ERR_OOM;
    Fe *raw_in = raw, *raw_tab = raw + n, *sraw = raw + (size_t)2 * n, *left = raw + (size_t)3 * n;
    uint32_t* d_err = u32 + (size_t)2 * n + 2;  // behind permute_pairs' scratch: zeroed by the same fill
    ZG_TRY(poly_to_raw(ctx, (const Fe*)d_input, raw_in, n));
    ZG_TRY(poly_to_raw(ctx, (const Fe*)d_table, raw_tab, n));
    ZG_TRY(poly_sort_pad(ctx, raw, n, usable, 2));
    ZG_TRY(poly_sort_keys(ctx, raw, n, 2));
    ZG_TRY(poly_permute_pairs(ctx, raw_in, raw_tab, sraw, n, usable, 1, u32, left, d_err));
    uint32_t h_err = 0;
    ZG_HIP(hipMemcpyAsync(&h_err, d_err, sizeof(h_err), hipMemcpyDeviceToHost, ctx->stream));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    ZG_REQUIRE(h_err == 0, ZG_ERR_CONSTRAINT,
               "zg_permute_expression_pair_dev: an input value is missing from the table (ConstraintSystemFailure)");
    ZG_TRY(poly_from_raw(ctx, raw_in, (Fe*)d_permuted_input, usable));
    ZG_TRY(poly_from_raw(ctx, sraw, (Fe*)d_permuted_table, usable));
    if (usable < n) {
        ZG_HIP(hipMemsetAsync((Fe*)d_permuted_input + usable, 0, (size_t)(n - usable) * 32, ctx->stream));
        ZG_HIP(hipMemsetAsync((Fe*)d_permuted_table + usable, 0, (size_t)(n - usable) * 32, ctx->stream));
    }
    return ZG_OK;
}

int zg_permute_expression_pair(zg_ctx* ctx, const zg_fr* input, const zg_fr* table, uint32_t k, uint32_t usable,
                               zg_fr* permuted_input, zg_fr* permuted_table) {
    ZG_REQUIRE(ctx && input && table && permuted_input && permuted_table, ZG_ERR_INVALID_ARG,
               "zg_permute_expression_pair: null argument");
    ZG_REQUIRE(k >= 4 && k <= 20, ZG_ERR_UNSUPPORTED, "zg_permute_expression_pair: k=%u outside 4..20", k);
    const size_t n = (size_t)1 << k;
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    Fe* d = ws.get<Fe>(4 * n);
    if (ws.failed) return ZG_ERR_OOM;
    ZG_HIP(hipMemcpyAsync(d, input, n * 32, hipMemcpyHostToDevice, ctx->stream));
    ZG_HIP(hipMemcpyAsync(d + n, table, n * 32, hipMemcpyHostToDevice, ctx->stream));
    ZG_TRY(zg_permute_expression_pair_dev(ctx, d, d + n, k, usable, d + 2 * n, d + 3 * n));
    ZG_HIP(hipMemcpyAsync(permuted_input, d + 2 * n, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZG_HIP(hipMemcpyAsync(permuted_table, d + 3 * n, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    return ZG_OK;
}

int zg_lookup_product_terms_dev(zg_ctx* ctx, const void* d_input, const void* d_table, const void* d_permuted_input,
                                const void* d_permuted_table, const zg_fr* beta, const zg_fr* gamma, size_t n, void* d_num,
                                void* d_den) {
    ZG_REQUIRE(ctx && d_input && d_table && d_permuted_input && d_permuted_table && beta && gamma && d_num && d_den,
               ZG_ERR_INVALID_ARG, "zg_lookup_product_terms_dev: null argument");
    ZG_REQUIRE(n < (1u << 28), ZG_ERR_UNSUPPORTED, "zg_lookup_product_terms_dev: n too large");
    if (!n) return ZG_OK;
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    ProofConst hc;  // (a one-entry batch: lookup 0 of proof 0, product 0)
    memset(&hc, 0, sizeof(hc));
    hc.beta = to_fe(beta);
    hc.gamma = to_fe(gamma);
    ProofConst* dpc = nullptr;
    ZG_TRY(poly_one_const(ctx, ws, hc, &dpc));
    return poly_lookup_terms(ctx, dpc, 1, (const Fe*)d_input, (const Fe*)d_table, (const Fe*)d_permuted_input,
                             (const Fe*)d_permuted_table, 0, 0, (Fe*)d_num, (Fe*)d_den, 1, 0, (uint32_t)n, 1);
}

int zg_fr_lincomb_dev(zg_ctx* ctx, const void* const* d_polys, const zg_fr* coeffs, size_t count, size_t n, const zg_fr* sub0,
                      void* d_out) {
    ZG_REQUIRE(ctx && d_out && (count == 0 || (d_polys && coeffs)), ZG_ERR_INVALID_ARG, "zg_fr_lincomb_dev: null argument");
    ZG_REQUIRE(n < (1u << 28), ZG_ERR_UNSUPPORTED, "zg_fr_lincomb_dev: n too large");
    for (size_t j = 0; j < count; j++) {
        ZG_REQUIRE(d_polys[j], ZG_ERR_INVALID_ARG, "zg_fr_lincomb_dev: polynomial %zu is null", j);
        ZG_REQUIRE(d_polys[j] != d_out, ZG_ERR_INVALID_ARG, "zg_fr_lincomb_dev: d_out is polynomial %zu", j);
    }
    ZG_ENTER(ctx);
    Fe sub;
    if (sub0) sub = to_fe(sub0);
    return poly_lincomb(ctx, reinterpret_cast<const Fe* const*>(d_polys), reinterpret_cast<const Fe*>(coeffs), count, (uint32_t)n,
                        sub0 ? &sub : nullptr, (Fe*)d_out);
}

int zg_fr_random_dev(zg_ctx* ctx, const uint8_t key[32], uint32_t tag, void* d_out, size_t count) {
    ZG_REQUIRE(ctx && key && (d_out || !count), ZG_ERR_INVALID_ARG, "zg_fr_random_dev: null argument");
    ZG_REQUIRE(count <= 0xffffffffull, ZG_ERR_UNSUPPORTED, "zg_fr_random_dev: %zu scalars", count);
    ZG_ENTER(ctx);
    uint32_t kw[8];
    memcpy(kw, key, sizeof(kw));
    return poly_rand_fill(ctx, kw, tag, (Fe*)d_out, (uint32_t)count);
}

}  // extern "C"
