// Device-side circuit image and the launch helpers of poly.hip (shared with prover.hip and prove_batch.hip).
#pragma once

#include "common.h"
#include "msm.h"

namespace zg {

struct alignas(16) DMono {
    Fe coeff;
    uint32_t n_factors;
    // 1: coefficient +1, 2: coefficient -1 (the nine-limb evaluation adds / subtracts instead of multiplying);
    // 3 (monos_hat only): the coefficient is the integer `small`, |small| <= F9_SMALL_MAX (field9.h): f9_mul_small
    uint32_t coeff_is_one;
    uint32_t factors[ZG_MAX_FACTORS];
    int32_t small;
    uint32_t pad;
};
static_assert(sizeof(DMono) == 80, "DMono layout");

struct DLookup {
    uint32_t width;
    zg_poly inputs[ZG_MAX_LOOKUP_WIDTH];
    zg_poly tables[ZG_MAX_LOOKUP_WIDTH];
};

// circuit arrays in HBM (read through the scalar cache: every index is wave-uniform)
struct DevCircuit {
    const zg_query* queries;
    const DMono* monos;
    const zg_poly* gates;
    const DLookup* lookups;
    const zg_query* perm_cols;
    uint32_t n_gates, n_lookups, n_perm, chunk, n_sets;
};

// one family of column arrays [column][size]; in a lock-step batch proof b's advice / instance columns start
// adv_bs / inst_bs elements after proof b-1's (the fixed columns belong to the proving key: one copy)
struct Cols {
    const Fe* fixed;
    const Fe* advice;
    const Fe* instance;
    uint32_t log_size;
    int32_t rot_scale;
    size_t adv_bs, inst_bs;
};

// Per-proof scalars of a lock-step batch: one entry per proof in HBM, rewritten by the host at every transcript step
// (kernels read their proof's entry through the scalar cache: the proof index is workgroup-uniform).
constexpr uint32_t PC_MAX_POINTS = 16;
constexpr uint32_t PC_U_SLOT = PC_MAX_POINTS;  // ProofConst::points: the slot of SHPLONK's u, behind the rotations'
constexpr uint32_t EH_MAX_YPOW = 48;  // evaluate_h's grouped form: powers of y, one per term after the gates (+ 1)
// evaluate_h's scaled permutation term (EvalHArgs::sigma_sc): the most permutation columns / sets it holds constants for
constexpr uint32_t EH_MAX_PCOLS = 16, EH_MAX_PSETS = 8;
struct alignas(16) ProofConst {
    uint32_t key[8];            // blinding key (ChaCha20), rand_fr
    Fe theta, beta, gamma;      // library (2^256 Montgomery) form: lookup compression, product terms
    Fe eh_y, eh_beta, eh_gamma, eh_theta;  // the form evaluate_h computes in (x 2^5 for the nine-limb kernel)
    Fe eh_delta_start[2];       // beta * zeta^zpow for zpow = 1, 2, same form
    Fe eh_ypow[EH_MAX_YPOW];    // y^j, same form (the weights of the permutation / lookup terms, EvalHArgs::n_terms)
    // scaled permutation term, per coset shift zeta^a (index a - 1), same form: both factors of column `col` are divided by
    // K = beta delta^col zeta^a, so eh_pcol[a - 1][col] = K^-1 and eh_pw[a - 1][s] = y^e_s * prod_(col in set s) K
    // (the weight of set s's term); eh_scaled = 0 (beta = 0, or more columns than fit): the unscaled term
    Fe eh_pcol[2][EH_MAX_PCOLS];
    Fe eh_pw[2][EH_MAX_PSETS];
    uint32_t eh_scaled, eh_pad[7];
    Fe xn;                      // x^n (vanishing::evaluate's Horner variable)
    Fe v;                       // GWC's v
    Fe points[PC_MAX_POINTS + 1];  // opening points x * omega^rotation, by slot; the last one: SHPLONK's u (PC_U_SLOT)
    Fe subs[PC_MAX_POINTS];     // eval_batch of GWC point set s
    Fe fold_w;                  // a proof of several circuits: the weight of this slot's quotient in the proof's (poly_fold_slots)
    // the shuffle pass over h (poly_shuffle_h), library form: y, and y^(3 NS), by which the terms before the shuffles' move up
    Fe sh_y, sh_ypow;
};

struct EvalHArgs {
    DevCircuit c;
    Cols cols;  // extended cosets
    const Fe* sigma_cos;
    // sigma_cos' column `col` times (delta^col zeta^zpow)^-1: the grouped nine-limb kernel reads it INSTEAD of sigma_cos
    // for a proof with pc->eh_scaled (null: the unscaled permutation term for every proof)
    const Fe* sigma_sc;
    const Fe* pz_cos;
    const Fe* lz_cos;
    const Fe* pin_cos;   // lookup l's permuted input / table cosets: pin_cos + l * perm_stride, ptab_cos + l * perm_stride
    const Fe* ptab_cos;
    size_t perm_stride;  // (2 * en when the two live interleaved in one batch, as the prover keeps them)
    const Fe* l0;
    const Fe* llast;
    const Fe* lactive;
    const Fe* ext_tw;  // extended_omega^i
    const Fe* t_eval;  // ((zeta*ext_omega^i)^n - 1)^-1, period t_len (power of two)
    uint32_t t_mask;
    int32_t last_rot;  // -(blinding_factors + 1)
    // lock-step batch: workgroup row blockIdx.y = proof b; its challenges are pc[b] (eh_* fields; delta_start is
    // eh_delta_start[zpow - 1]), its cosets start b * cos_bs after sigma_cos' siblings, its h at h + b * h_bs
    const ProofConst* pc;
    uint32_t zpow;
    size_t cos_bs, h_bs;
    Fe delta;
    Fe* h;
    // nine-limb evaluation (hat = true): every coset slab, l-polynomial, ext_tw and t_eval entry and every
    // constant above is in the 2^261 Montgomery form (x * 2^261 mod r, packed), and so are the monomial
    // coefficients in monos_hat; h comes out in that form too (extended_to_coeff_dev(unhat) undoes it)
    bool hat;
    const DMono* monos_hat;
    // gates with a cell common to all their monomials (zero_g's are selector * (...)) are given factored:
    // gates_hat[g] ranges over monos_hat entries with that cell removed, gate_common[g] is its query index
    // (0xffffffff: not factored, gates_hat[g] is the plain polynomial)
    const zg_poly* gates_hat;
    const uint32_t* gate_common;
    // the factor may be a polynomial in that cell (halo2's merged selectors: q * prod (u - q)):
    // gate g = U(cell) * gates_hat[g], U(x) = sum_{k=1..count} uni_coef[first + k - 1] x^k; count 0: U(x) = x
    const zg_poly* gate_uni;
    const Fe* uni_coef;
    // ... and when that cell is a fixed one, U(cell) is tabulated over the extended domain by poly_gate_factor:
    // gate_slab[g] = index of the gate's slab (en entries) in gate_slabs, 0xffffffff: evaluate U in the kernel
    const uint32_t* gate_slab;
    const Fe* gate_slabs;
    // grouped form of the nine-limb evaluation: the n_terms permutation / lookup terms that follow the gates are
    // weighted by pc->eh_ypow and summed per l-polynomial (0: the plain Horner fold in y)
    uint32_t n_terms;
    // The terms by degree (poly_evaluate_h's modes EH_BOTH / EH_HIGH, the split domain's two parts): gate_cls[g] = (gate g
    // is a high term) | e << 1, its class's Horner carry being multiplied by y^e before the gate is added; tail_lo /
    // tail_hi = the power of y each class's gate sum ends on; bit s of set_hi / bit l of lk_hi = the product term of
    // permutation set s / lookup l is high (every other term after the gates is low).  EH_BOTH stores the sum of all
    // terms to h and the high terms' sum to h_hi (proof b's at h_hi + b * h_bs); EH_HIGH stores the high terms' to h.
    const uint32_t* gate_cls;
    uint32_t tail_lo, tail_hi, set_hi;
    uint64_t lk_hi;
    Fe* h_hi;
};
// which terms a launch of evaluate_h evaluates (EvalHArgs::gate_cls)
enum EvalHMode : int { EH_ALL = 0, EH_BOTH = 1, EH_HIGH = 2 };

// blinding scalar = f(seed, tag, index); identical to the oracle's definition
enum {
    TAG_ADVICE_BLIND = 1,
    TAG_PERMUTED_INPUT = 2,
    TAG_PERMUTED_TABLE = 3,
    TAG_PERM_Z = 4,
    TAG_LOOKUP_Z = 5,
    TAG_RANDOM_POLY = 6,
    TAG_VERIFY_BATCH = 7,  // the verifier's batch weights r_b (verify.hip), not a blinding scalar
    TAG_SRS_POWERS = 8,    // zg_params_check: the weights r_i of the powers relation (params.hip)
    TAG_SRS_LAGRANGE = 9,  // zg_params_check: the coefficients c_j of the Lagrange relation
    TAG_SHUFFLE_Z = 10     // the blinding rows of shuffle j's product: index j * rows + row
};
inline Fe to_fe(const zg_fr* s) {
    Fe r;
    memcpy(&r, s, 32);
    return r;
}
// rand_fr on the host (Montgomery form)
Fe rand_fr_host(const uint32_t* key, uint32_t tag, uint64_t index);

// ---- launch helpers (all asynchronous on ctx->stream) ----
// out[i] = rand_fr(key, tag, i), i < count (Montgomery form): a vector of scalars drawn on the device under one key
int poly_rand_fill(zg_ctx* ctx, const uint32_t key[8], uint32_t tag, Fe* out, uint32_t count);
// Lock-step batches: `nb` proofs, proof b's scalars in pc[b], its arrays `*_bs` elements after proof b-1's.
// The two draws a proof starts with: the vanishing argument's random polynomial (n values, to out and out2) and
// the blinding rows [row0, row0 + nrows) of the ncols advice columns.
int poly_random_and_blind(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, Fe* out, size_t out_bs, Fe* out2, size_t out2_bs,
                          uint32_t n, uint32_t tag, Fe* base, size_t base_bs, size_t col_stride, uint32_t ncols,
                          uint32_t row0, uint32_t nrows, uint32_t blind_tag);
// columns [0, ncols0) draw from tag0 (index c * nrows + j), the ncols1 columns after them from tag1 (index restarts)
int poly_blind_rows2(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, Fe* base, size_t base_bs, size_t col_stride,
                     uint32_t ncols0, uint32_t tag0, uint32_t ncols1, uint32_t tag1, uint32_t row0, uint32_t nrows);
// lookup l of proof b: compressed columns (and the sort keys raw_in / raw_tab) at index b * n_lookups + l
int poly_lookup_compress(zg_ctx* ctx, const DevCircuit& c, const Cols& cols, const ProofConst* pc, uint32_t nb, Fe* cin,
                         Fe* ctab, uint32_t n, Fe* raw_in = nullptr, Fe* raw_tab = nullptr, uint32_t usable = 0);
// perm + b * perm_bs + 2l * n = a'_l, + n = s'_l
int poly_permuted_finish(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, const Fe* raw_in, const Fe* raw_tab, Fe* perm,
                         size_t perm_bs, uint32_t n, uint32_t usable, uint32_t nblind, uint32_t n_lookups, uint32_t tag_in,
                         uint32_t tag_tab);
int poly_to_raw(zg_ctx* ctx, const Fe* in, Fe* out, size_t count);
int poly_from_raw(zg_ctx* ctx, const Fe* in, Fe* out, size_t count);
int poly_from_raw_rows(zg_ctx* ctx, const Fe* src, size_t src_stride, Fe* dst, size_t dst_stride, uint32_t rows,
                       uint32_t len);
// product q = b * per + j of the batch (per products per proof: `sets` permutation sets, then the lookups):
// num / den at q * n
int poly_lookup_terms(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, const Fe* cin, const Fe* ctab, const Fe* pin,
                      const Fe* ptab, size_t perm_stride, size_t perm_bs, Fe* num, Fe* den, uint32_t per, uint32_t first,
                      uint32_t n, uint32_t n_lookups);
// (only_set >= 0: that column set alone, written as product 0 of each proof)
int poly_perm_terms(zg_ctx* ctx, const DevCircuit& c, const Cols& cols, const ProofConst* pc, uint32_t nb,
                    const Fe* sigma_val, const Fe* omega_tw, Fe* num, Fe* den, uint32_t per, uint32_t n, int only_set = -1);
// A one-entry ProofConst in workspace memory for the stand-alone entries that borrow a prover kernel: *hc is copied to a
// block of `ws` and the stream is drained (hc is the caller's stack memory), *out = the device copy
int poly_one_const(zg_ctx* ctx, WsScope& ws, const ProofConst& hc, ProofConst** out);
// z[q][0] = z0[q] (device array, or all ones if null), z[q][i+1] = z[q][i]*num[q][i]/den[q][i] for the `batch`
// products q = g * per + j (per = 0: one group); within a group the first `chain` products are chained: product j
// starts from product j-1's value at row `last`.  num / den / tmp are flat ([q][n]); z of product q goes to
// z + g * z_outer + j * n (z_outer = 0: flat).
size_t poly_grand_product_tmp_elems(uint32_t n, uint32_t batch);
// half: 0 = the whole sequence; 1 = only the launches up to the totals, 2 = only what follows them (the latency form's
// host inversion of the totals -- a stream synchronisation -- and the apply launch): the two halves of one call, same arguments.
int poly_grand_product(zg_ctx* ctx, const Fe* num, const Fe* den, const Fe* d_z0, Fe* z, Fe* tmp, uint32_t n,
                       uint32_t batch, uint32_t chain, uint32_t last, uint32_t per = 0, size_t z_outer = 0, int half = 0);
// what zg_prover_create*_shuffles and zg_verifier_create_shuffles ask of the shuffles, before anything is allocated
// (who: the entry's name; cs: the caller's circuit, a challenge still a ZG_CHALLENGE query)
int shuffles_ok(const char* who, const zg_circuit* cs, const zg_shuffle* shuffles, uint32_t n_shuffles);
// The shuffle arguments' grand-product terms: product q = b * ns + j of the batch (shuffle j of proof b) gets
// num[q][row] = a + gamma, den[q][row] = s + gamma, a and s the theta-folds of shuffles[j]'s inputs / tables on the value rows
int poly_shuffle_terms(zg_ctx* ctx, const DevCircuit& c, const DLookup* shuffles, uint32_t ns, const Cols& cols, const ProofConst* pc,
                       uint32_t nb, Fe* num, Fe* den, uint32_t n);
// The shuffle arguments' share of the quotient, a pass over h behind evaluate_h on one part of the extended domain:
// h <- h y^(3 ns) + (sum over the shuffles, folded by y, of l0 (1 - z), l_last (z^2 - z), l_active (z(wX) (s + gamma) - z (a + gamma))) t_eval
// a: evaluate_h's arguments for that part (columns, l-polynomials, t_eval, pc, strides, h; with h_hi the same pass over it);
// sz_cos: shuffle 0's product slab of proof 0 (shuffle j's en further, proof b's a.cos_bs further)
int poly_shuffle_h(zg_ctx* ctx, const EvalHArgs& a, const DLookup* shuffles, uint32_t ns, const Fe* sz_cos, uint32_t en, uint32_t nb);
// n_columns = advice + instance + fixed columns of the circuit, unit_share = the rows of EvaluationDomain's extended domain
// this launch stands for (both only shape the profile's byte charges); mode: every term into h, or the terms by degree
// (EvalHArgs::gate_cls -- the grouped nine-limb kernel only)
int poly_evaluate_h(zg_ctx* ctx, const EvalHArgs& a, uint32_t en, uint32_t nb, uint32_t n_columns, double unit_share,
                    EvalHMode mode = EH_ALL);
// out[i] = U(col[(i + rot_off) mod en]),  U(x) = sum_{k=1..count} coef[k-1] x^k; everything in the 2^261 form
int poly_gate_factor(zg_ctx* ctx, const Fe* col, uint32_t rot_off, uint32_t en, const Fe* coef, uint32_t count, Fe* out);
// Coefficient-form polynomials a kernel may be asked for by index: indices below nsh name the proving key's
// (one copy: sh + ix * n), the others proof b's (pp + b * pp_bs + (ix - nsh) * n).
struct PolySet {
    const Fe* sh;
    const Fe* pp;
    uint32_t nsh;
    size_t n;      // elements per polynomial
    size_t pp_bs;
};
// pw + b * pw_bs + s * n <- powers 0 .. n-1 of pc[b].points[s], s < npoints
int poly_powers(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, uint32_t npoints, uint32_t n, Fe* d_pow, size_t pw_bs);
// out[b * out_bs + j] = <poly poly_idx[j] of proof b, powers row point_idx[j] of proof b>
int poly_dot(zg_ctx* ctx, const PolySet& polys, uint32_t nb, uint32_t n, const uint32_t* d_poly_idx,
             const uint32_t* d_point_idx, const Fe* d_pow, size_t pw_bs, uint32_t count, Fe* d_out, size_t out_bs,
             uint32_t distinct_polys = 0, uint32_t distinct_points = 0);  // (distinct counts: the profile's byte charge only)
// out[b][i] = Horner in pc[b].xn over the polys listed (first listed = highest power)
int poly_horner_combine_xn(zg_ctx* ctx, const PolySet& polys, const ProofConst* pc, uint32_t nb, const uint32_t* d_list,
                           uint32_t count, Fe* out, size_t out_bs, uint32_t n);
constexpr uint32_t HC_MAX_SETS = PC_MAX_POINTS;
constexpr uint32_t FESET_MAX = 8;
struct FeSet {  // a few field elements passed by value in kernel arguments
    Fe v[FESET_MAX];
};
// GWC: set s of proof b = Horner in pc[b].v over the polys of list s, minus pc[b].subs[s] at X^0;
// out + b * out_bs + s * out_stride
int poly_horner_combine_sets(zg_ctx* ctx, const PolySet& polys, const ProofConst* pc, uint32_t nb, const uint32_t* d_lists,
                             uint32_t list_stride, const uint32_t* counts, uint32_t nsets, Fe* out, size_t out_stride,
                             size_t out_bs, uint32_t n);
// A proof of several circuit instances (create_proof's `circuits` slice; the slots are the circuits, pc[0] the proof's scalars):
// h[i] <- sum_c pc[c].fold_w * h[c * h_bs + i], i < len, c < nb <= FOLD_MAX_SLOTS
constexpr uint32_t FOLD_MAX_SLOTS = 64;
int poly_fold_slots(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, Fe* h, size_t h_bs, uint32_t len);
// GWC: set s = Horner in pc[0].v over d_lists[firsts[s] .. + counts[s]) (entry = slot << 16 | polynomial index, any
// length), minus pc[0].subs[s] at X^0; out + s * out_stride
int poly_combine_pairs(zg_ctx* ctx, const PolySet& polys, const ProofConst* pc, const uint32_t* d_lists, const uint32_t* firsts,
                       const uint32_t* counts, uint32_t nsets, Fe* out, size_t out_stride, uint32_t n);
// SHPLONK: output o of proof b = sum_t d_coef[b * coef_bs + firsts[o] + t] * poly(d_lists[firsts[o] + t])
// (entry = slot << 16 | polynomial index, the slot counted from b), plus, with `extra`, d_coef[.. + counts[o]] * extra[b * extra_bs ..],
// minus d_corr[b * corr_bs + o * ncorr + i] at i < ncorr; to out + b * out_bs + o * out_stride.  d_coef: device memory, the
// coefficients times 2^5 and unpacked (f9_unpack(Fr::mul(c, Fr9Params::c261_fe()))).
struct F9;
int poly_combine_weighted(zg_ctx* ctx, const PolySet& polys, uint32_t nb, const uint32_t* d_lists, const uint32_t* firsts,
                          const uint32_t* counts, uint32_t nouts, const F9* d_coef, size_t coef_bs, const Fe* d_corr, uint32_t ncorr,
                          size_t corr_bs, const Fe* extra, size_t extra_bs, Fe* out, size_t out_stride, size_t out_bs, uint32_t n);
// out[b * out_bs + i] = sum_(s < rows) in[b * in_bs + s * in_stride + i]
int poly_sum_rows(zg_ctx* ctx, uint32_t nb, const Fe* in, size_t in_stride, size_t in_bs, uint32_t rows, Fe* out, size_t out_bs,
                  uint32_t n);
// out[i] = sum_j coeffs[j] * polys[j][i], i < n, minus *sub0 (may be null) at i = 0; polys and coeffs are HOST arrays of
// `count` entries (device pointers / library-form scalars) that travel in the kernel arguments, 64 terms per launch
int poly_lincomb(zg_ctx* ctx, const Fe* const* polys, const Fe* coeffs, size_t count, uint32_t n, const Fe* sub0, Fe* out);
// kate_division of `nsets` polynomials per proof: a + b * a_bs + s * a_stride divided by (X - pc[b].points[slot[s]])
// (slot: a rotation's point slot, or PC_U_SLOT for SHPLONK's u)
size_t poly_kate_tmp_elems(uint32_t n, uint32_t batch);
int poly_kate_division(zg_ctx* ctx, const ProofConst* pc, uint32_t nb, const uint32_t* slots, uint32_t nsets, const Fe* a,
                       size_t a_stride, size_t a_bs, Fe* q, size_t q_stride, size_t q_bs, Fe* tmp, uint32_t n);
int poly_l_cosets_init(zg_ctx* ctx, Fe* l0, Fe* llast, Fe* lblind, uint32_t n, uint32_t bf);
int poly_lactive(zg_ctx* ctx, Fe* lactive, const Fe* llast, const Fe* lblind, uint32_t en, bool hat);
int poly_scale(zg_ctx* ctx, const Fe* in, Fe* out, size_t count, const Fe& factor);  // out[i] = in[i] * factor

// Challenges as columns (zg_prover_set_phases): what challenge_fill_kernel writes for one phase of a batch -- the constant
// into all n rows of each challenge's value row (the blinding rows included: the polynomial IS the constant), (c, 0, ..)
// into its coefficient row and the constant into its slab on every part of the extended domain in use, there in the form
// that part's readers expect (vals[..][1]: x 2^5 for the nine-limb evaluate_h).  No transform is spent on a constant.
struct ChalFill {
    uint32_t count = 0;                    // challenges of the phase that have a pseudo-column
    uint32_t chal[ZG_MAX_CHALLENGES] = {};  // their indices
    uint32_t col0 = 0;                     // pseudo-column of challenge 0 among the value rows (IU) ...
    Fe* val = nullptr; size_t val_bs = 0;  // value rows [nb][I][n]
    Fe* coef = nullptr; size_t coef_bs = 0;  // coefficient row of challenge 0, proof 0; proof b's coef_bs further
    uint32_t n = 0, nparts = 0;
    Fe* cos[2] = {nullptr, nullptr};       // slab of challenge 0, proof 0, per part in use
    size_t cos_bs[2] = {0, 0};
    uint32_t en[2] = {0, 0};
    const Fe* vals = nullptr;              // [nb][stride][2]
    uint32_t stride = 0;
};
int poly_challenge_fill(zg_ctx* ctx, const ChalFill& f, uint32_t nb);

// from sort.hip: lookup::prover::permute_expression_pair on the device
int poly_sort_pad(zg_ctx* ctx, Fe* keys, uint32_t n, uint32_t usable, uint32_t batch);
int poly_sort_keys(zg_ctx* ctx, Fe* keys, uint32_t n, uint32_t batch);
int poly_permute_pairs(zg_ctx* ctx, const Fe* a, const Fe* t, Fe* sprime, uint32_t n, uint32_t usable, uint32_t batch,
                       uint32_t* scratch_u32, Fe* scratch_fe, uint32_t* d_err);

// from ntt.hip
// Batches laid out in groups (the same columns of several proofs): array v of a batch sits at
// base + (v / per) * outer + (v % per) * stride, on the input and on the output side; per = 0: flat (v * stride).
struct Grouping {
    uint32_t per = 0;
    size_t in_outer = 0, out_outer = 0;
};
int ntt_batch_dev(zg_ctx* ctx, Fe* d_a, size_t stride, size_t batch, uint32_t log_n, const Fe& omega,
                  const Fe* divisor);
int ntt_batch_to_dev(zg_ctx* ctx, const Fe* d_in, Fe* d_out, size_t stride, size_t batch, uint32_t log_n, const Fe& omega,
                     const Fe* divisor, const Grouping* grp = nullptr);
int coeff_to_extended_dev(zg_ctx* ctx, const Fe* d_in, size_t in_stride, Fe* d_out, size_t out_stride,
                          size_t batch, uint32_t k, uint32_t ext_k, bool hat);
int extended_to_coeff_dev(zg_ctx* ctx, Fe* d_evals, uint32_t k, uint32_t ext_k, size_t out_len, Fe* d_out, bool unhat);
int coeff_to_coset_dev(zg_ctx* ctx, const Fe* d_in, size_t in_stride, uint32_t in_len, Fe* d_out, size_t out_stride,
                       size_t batch, uint32_t ext_k, bool hat, const Fe& shift, const Grouping* grp = nullptr);
int coset_to_coeff_dev(zg_ctx* ctx, Fe* d_evals, uint32_t ext_k, size_t out_len, Fe* d_out, bool unhat, const Fe& shift,
                       size_t batch = 1, size_t in_stride = 0, size_t out_stride = 0);
// split extended domain (prove_batch.hip): the pieces of the interpolation between its two cosets
// (each for nb proofs: proof b's arrays `*_bs` elements after proof b-1's)
int poly_fold(zg_ctx* ctx, uint32_t nb, const Fe* a, size_t a_bs, uint32_t len, uint32_t parts, const Fe& e, Fe* out,
              size_t out_bs);  // out[r] = sum_q a[r + q*len] e^q
int poly_diff_scale(zg_ctx* ctx, uint32_t nb, const Fe* u, size_t u_bs, const Fe& cu, const Fe* v, size_t v_bs, const Fe& scale,
                    Fe* out, size_t out_bs, uint32_t len);  // (u*cu - v)*scale
int poly_split_combine(zg_ctx* ctx, uint32_t nb, Fe* h, size_t h_bs, const Fe* b, size_t b_bs, uint32_t len, const Fe& c1,
                       uint32_t hi_at);  // h[j] -= c1 b[j]; h[hi_at + j] = b[j]

}  // namespace zg
