/*
 * zg_halo2.h -- C ABI of the MI355X proving backend for zero_g's Halo2 WNN circuit.
 *
 * This is the drop-in boundary.  The reference has no FFI seam of its own:
 * `Wnn::proof` (/root/reference/src/wnn.rs:232-262) calls `halo2_proofs::plonk::create_proof`
 * (wnn.rs:242-259) with `KZGCommitmentScheme<Bn256>` / `ProverGWC` (wnn.rs:243-244), and the hot
 * arithmetic sits behind halo2's `arithmetic::{best_multiexp, best_fft}`, `poly::EvaluationDomain`,
 * `poly::commitment::{Params, ParamsProver}` and `plonk::{evaluation, lookup, permutation,
 * vanishing}` (git dependency halo2_proofs v2023_04_20, reference Cargo.toml:21-25).  Each entry
 * point below names the upstream function it replaces; INTEGRATION.md shows the Rust `extern "C"`
 * binding a maintainer would add in a `[patch]`-ed halo2_proofs (the mechanism the reference
 * already uses for halo2curves, Cargo.toml:14-18).
 *
 * Conventions
 *   - zg_fr / zg_fq : 4 x u64 little-endian limbs, Montgomery form, R = 2^256 (halo2curves 0.3.3).
 *   - zg_g1_affine  : {x, y}, 64 B, (0,0) = identity (bn256::G1Affine).
 *   - zg_g1         : Jacobian {x, y, z}, 96 B, z = 0 = identity (bn256::G1).  MSM results are
 *                     returned NORMALISED (z = 1, or (0,1,0) for the identity) so that the bytes are
 *                     canonical: a Jacobian triple is otherwise only defined up to scaling.
 *   - every function returns 0 on success or a negative zg_status; zg_last_error() describes the
 *     most recent failure on the calling thread.  Nothing throws or aborts across the ABI.
 *     Upstream MSM/FFT are infallible apart from length asserts; the Rust shim maps nonzero to panic!.
 *   - pointers are borrowed for the duration of the call unless a handle is returned.
 *   - one zg_ctx drives one GPU (one process per GPU; multi-GPU composition is in INTEGRATION.md).
 *   - thread safety: every entry point that takes a zg_ctx (or a zg_prover / zg_bases created on one) holds that
 *     context's lock for the whole call, so calls on ONE context serialise and calls on DIFFERENT contexts run
 *     concurrently (e.g. from rayon workers, each with its own context).  Objects that are only read -- zg_bases
 *     tables, the proving key of forked provers -- may be shared by all contexts of their device.
 *   - *_dev entry points take DEVICE pointers (HBM-resident data, e.g. torch tensors' data_ptr())
 *     and are asynchronous on the context stream; call zg_ctx_sync() before reading results.
 */
#ifndef ZG_HALO2_H
#define ZG_HALO2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } zg_fr;
typedef struct { uint64_t l[4]; } zg_fq;
typedef struct { zg_fq x, y; } zg_g1_affine;
typedef struct { zg_fq x, y, z; } zg_g1;
typedef struct { zg_fq c0, c1; } zg_fq2;        /* c0 + c1 u, u^2 = -1 (bn256::Fq2)                          */
typedef struct { zg_fq2 x, y; } zg_g2_affine;   /* bn256::G2Affine on y^2 = x^3 + 3/(9+u); (0,0) = identity */

typedef struct zg_ctx zg_ctx;       /* one GPU: stream, workspace, twiddle cache        */
typedef struct zg_bases zg_bases;   /* HBM-resident base set (ParamsKZG::g / g_lagrange) */

typedef enum {
    ZG_OK = 0,
    ZG_ERR_INVALID_ARG = -1,   /* null pointer, length mismatch (upstream: assert_eq! panic) */
    ZG_ERR_NO_DEVICE = -2,     /* no usable HIP device: the library never falls back to a CPU path */
    ZG_ERR_HIP = -3,           /* a HIP runtime call failed                                  */
    ZG_ERR_UNSUPPORTED = -4,   /* size outside what the kernels are built for                */
    ZG_ERR_CONSTRAINT = -5,    /* plonk::Error::ConstraintSystemFailure (lookup input not in table) */
    ZG_ERR_OOM = -6
} zg_status;

const char *zg_last_error(void);
/* Library version string and the gfx target it was compiled for ("gfx950"). */
const char *zg_version(void);

/* ------------------------------------------------------------------ tuning
 * Every switch of the library, by name.  A knob starts from the environment variable of the same name (read once, when
 * the first knob is asked for) and may be set at run time; value < 0 restores the library's default.  None changes a
 * result: every form computes the same group elements and field elements, bit for bit (tests/test_gpu_knobs.py walks
 * them all against the oracle).  Knobs that shape resident data are read when that object is built (ZG_MSM_C: a base
 * set registered with window_bits = 0; ZG_MSM_NAF, ZG_MSM_NAF_GL, ZG_MSM_RUNS, ZG_EVALH9, ZG_EVALH_GROUPED,
 * ZG_SPLIT_DOMAIN: zg_prover_create*; ZG_LAT_SPLIT_K: zg_prover_create* and zg_prover_set_overlap; ZG_LAT_FULL_C: zg_prover_enable_digit_tables), launch shapes at every launch (ZG_MSM_K, ZG_MSM_K_LAT, ZG_MSM_RB, ZG_MSM_LANES,
 * ZG_MSM_STRIP, ZG_LAT_FULL_K, ZG_LAZY_DOT, ZG_MSM_AFFINE, ZG_MSM_HEAVY, ZG_LAT_PULL, ZG_LAT_GATE).
 *   ZG_MSM_C          window bits of the MSM tables, 2..16 (default from n: k - 2)
 *   ZG_MSM_K          points per bucket-accumulation task in the throughput form, 4..120 (48)
 *   ZG_MSM_K_LAT      ... in the latency form (16; 32 / 48 from n = 2^16 / 2^17)
 *   ZG_MSM_RB         buckets per block of the latency form's bucket reduction: 64 / 128 / 256
 *   ZG_MSM_LANES      lanes per EC addition there: 2 / 4
 *   ZG_MSM_STRIP      buckets per lane in the throughput form's reduction: 2 / 4 / 8 / 16 (8)
 *   ZG_MSM_NAF        digit width of the free-position form for all-random commitments, 3..16; 0 = window tables only
 *   ZG_MSM_NAF_GL     ... for the run-form commitments against g_lagrange (c + 1); 0 = windows
 *   ZG_MSM_RUNS       0 = no run form (summation by parts over running base sums)
 *   ZG_EVALH_GROUPED  0 = evaluate_h folds in y term by term (the fallback of circuits with > 40 such terms)
 *   ZG_EVALH9         0 = evaluate_h on 8 x 32-bit limbs; implies the single extended coset
 *   ZG_SPLIT_DOMAIN   0 = EvaluationDomain's single extended coset in the throughput form too
 *   ZG_LAT_SPLIT_K    smallest k at which a lone proof (the latency form) takes the quotient from the split domain too (15)
 *   ZG_LAT_FULL_C     window bits of the latency form's digit tables (zg_bases_enable_digit_table); 0 = none
 *   ZG_LAT_FULL_K     summands per lane pair in the digit-table accumulation, 4..120 (16)
 *   ZG_LAZY_DOT       0 = eval_polynomial's dot products and the multiopen combinations reduce after every term
 *   ZG_MSM_AFFINE     rounds (0..4) of batched-affine pairwise additions -- one shared inversion per launch and round --
 *                     before the buckets' XYZZ chains in the throughput form; 0 = none
 *   ZG_MSM_HEAVY      task partials of a bucket above which it is merged ahead of the bucket reduction (msm_heavy), 1..64
 *                     (4 in the throughput form, 16 in the latency form)
 *   ZG_LAT_PULL       1 = a lone proof's per-phase scalars (challenges, opening points) reach the device through a one-wave
 *                     kernel that reads the pinned staging arena, 0 = through a copy command
 *   ZG_LAT_GATE       1 = a lone proof (latency form, one proof per call, unsharded; from the second proof in that form on)
 *                     puts each phase's launches on the stream BEFORE the host has the challenge they depend on, behind a
 *                     one-workgroup kernel that polls a word of mapped host memory; the host opens it with one store once
 *                     the challenge is staged (-1 to -2 % latency).  0 (default) = every phase is launched after its
 *                     challenge.  OPT-IN because a kernel that waits for the host needs every stream of the process on a
 *                     hardware queue of its own (GPU_MAX_HW_QUEUES >= the process's streams; two per latency-form prover):
 *                     where streams share a queue another stream's work can stand between this prover's streams and the
 *                     gate then only opens at its time limit (4 s), after which the proof is made again in the plain
 *                     order -- a stall, never a wrong proof.  Ignored under AMD_SERIALIZE_KERNEL / HIP_LAUNCH_BLOCKING; must be
 *                     OFF under counter collection (rocprofv3 --pmc serialises kernels across queues, which the library
 *                     cannot see).  A proof is gated only when it repeats the last completed proof's signature (scheduling
 *                     form, batch, instance length, digit tables, and no zg_tuning_set / zg_prover_set_batch in between):
 *                     anything else may allocate or synchronise and is made in the plain order; should a queued-ahead
 *                     phase still reach a blocking call, the gate is let go at once and the proof re-made (zg_prover_gate_stats).
 *                     (2: as 1, with the first gate of every proof left closed for 0.2 s -- exercises that path in tests.)
 *   ZG_WITNESS_LDS    0 = a witness plan (zg_witness_plan_create) keeps every operand of its program in HBM; 1 (default) =
 *                     the plan is register-allocated into LDS cells when it is made (live values in LDS, a level costs an LDS
 *                     round trip instead of three HBM round trips); n >= 2 = at most n KB of cells (what does not fit stays
 *                     in HBM: the medium and large models' case at the full 150 KB); read when the plan is created
 *   ZG_MSM_TOPSPLIT   0 = the free-position recoding (ZG_MSM_NAF) leaves its last digit whatever bits remain above the previous one
 *                     (tiny with probability 1/5: the hot small buckets); 1 (default) = the last two digits are cut evenly
 *   ZG_NTT9           the transforms' butterflies: 0 = on 8 x 32-bit limbs (a canonical value after every operation), 1 = on nine
 *                     29-bit limbs (limb-wise sums, no carry word in the products: a quarter fewer instructions per pass, 27 %
 *                     more multiply-adds; 36-byte elements in LDS).  Default: nine in the latency form (a lone proof: -0.3 / -1.7 /
 *                     -1.2 % at k = 14 / 15 / 17), eight in the throughput form (the nine-limb pass measured +0.4 ... +0.6 % ms/proof
 *                     under twelve provers: DESIGN.md section 5).  Same bytes either way: what leaves a pass is canonical. */
int zg_tuning_set(const char *name, int value);
int zg_tuning_get(const char *name, int *value);
/* out[i] = name of knob i for i < min(cap, count); returns the count. */
size_t zg_tuning_names(const char **out, size_t cap);

/* ------------------------------------------------------------------ context */
/* Creates a context on HIP device `device_id`.  Fails with ZG_ERR_NO_DEVICE when no GPU is
 * visible: there is deliberately no CPU fallback.  (SURVEY.md's sketch had zg_ctx_create(n_devices, device_ids):
 * here a context is ONE device -- one process per GPU -- and several GPUs are several contexts, composed by the
 * caller through zg_prover_set_shard / whole proofs per GPU.) */
int zg_ctx_create(int device_id, zg_ctx **out);
void zg_ctx_destroy(zg_ctx *ctx);
int zg_ctx_sync(zg_ctx *ctx);
/* Returns the free blocks of the context's workspace pool (and of its side stream's) to the device allocator, after
 * draining both streams; the pool grows again on demand.  For a long-lived process between workloads of different sizes
 * (upstream has no counterpart: halo2's buffers are Vec<F> owned by create_proof).  *freed_bytes (may be NULL) = what went. */
int zg_ctx_trim(zg_ctx *ctx, uint64_t *freed_bytes);
/* The hipStream_t every call of this context is ordered on (as void* to keep HIP out of the ABI). */
void *zg_ctx_stream(zg_ctx *ctx);

/* Per-kernel timing with HIP events recorded on the context stream around every launch (used by
 * bench.py for the roofline line; off by default).  Two ALGORITHMIC byte counts, neither measured HBM traffic:
 * algo_bytes = what the kernel's own algorithm streams (every distinct input once, every output once);
 * unit_bytes = SURVEY.md 8d's figure for the unit of work (one MSM: n * 96 + 96; one transform: (in + out) * 32; one
 * grand product: 3 n * 32; evaluate_h: (inputs + 1) * 8n * 32), charged ONCE per unit -- on the one kernel of a
 * multi-kernel launch sequence that carries the unit (msm_accumulate for an MSM), 0 on its stage kernels and on
 * kernels SURVEY names no unit for.  Summed over a proof's launches unit_bytes is SURVEY's per-proof figure. */
typedef struct {
    char name[48];
    uint64_t launches;
    double total_ms;
    double algo_bytes;
    double unit_bytes;
} zg_kernel_stat;
int zg_ctx_profile_enable(zg_ctx *ctx, int on);
/* Time only launches of the named kernel (NULL or "" = every kernel).  A timed launch carries its own start and
 * stop event (hipExtLaunchKernelGGL): the kernel's begin and end as rocprofv3 reports them; two events per launch
 * are cheap for one kernel, not for the ~150 launches of a whole proof. */
int zg_ctx_profile_filter(zg_ctx *ctx, const char *kernel_name);
int zg_ctx_profile_collect(zg_ctx *ctx, zg_kernel_stat *out, size_t cap, size_t *count);

/* ------------------------------------------------------------------ MSM
 * Replaces halo2_proofs::arithmetic::best_multiexp as reached through
 * ParamsKZG::commit / commit_lagrange (halo2_proofs/src/poly/kzg/commitment.rs upstream),
 * i.e. every commitment create_proof makes (30 per WNN proof).        */

/* Uploads a fixed base set once (ParamsKZG::g or ::g_lagrange) and precomputes the
 * window-shifted copies 2^(c*w) * P_i that let all Pippenger windows share one bucket set.
 * window_bits = 0 picks c from n; otherwise 2..16 (anything else: ZG_ERR_INVALID_ARG).  Host pointer. */
int zg_bases_register(zg_ctx *ctx, const zg_g1_affine *bases, size_t n, uint32_t window_bits,
                      zg_bases **out);
/* Same, from a device pointer (n * 64 B, HBM resident). */
int zg_bases_register_dev(zg_ctx *ctx, const void *d_bases, size_t n, uint32_t window_bits,
                          zg_bases **out);
void zg_bases_free(zg_bases *b);
/* Optional second table of a base set for batches of FULL-SIZE (random) scalars: one row per bit position, 2^j * P_i for
 * j < 255 (255 * n * 64 B -- 0.27 GB at n = 2^14), against which a scalar is recoded into odd signed digits of
 * `digit_width` bits at free positions (width-w NAF): 254 / (w + 1) additions per scalar where c-bit windows spend
 * 255 / c, on 2^(w-2) buckets.  Used by the zg_msm* entries of a context in its THROUGHPUT form
 * (zg_ctx_set_msm_latency(ctx, 0)); a latency-form context keeps the window table (a lone MSM waits on the gathers from
 * a table no cache holds).  digit_width in [3, 16]; idempotent for the same width.  Same results, bit for bit. */
int zg_bases_enable_bit_table(zg_ctx *ctx, zg_bases *bases, uint32_t digit_width);
/* Optional digit tables of a base set for LONE MSMs (a context in its latency form, zg_ctx_set_msm_latency(ctx, 1)): every
 * multiple d * 2^(c w) * P_i, d <= 2^(c-1), of every c-bit window -- ceil(255 / c) * 2^(c-1) * n * 64 B (26 GB at n = 2^14,
 * c = 11).  A signed digit then names its summand and the MSM is a flat sum of gathered points folded by a tree: no digit
 * sort, no buckets, no bucket reduction -- the latency of a lone commitment phase drops by about half.  window_bits 0 = chosen
 * from n and the free memory (none from n = 2^16 on, or when the card has no room: not an error); 4..12 otherwise.
 * Never built implicitly: this call for a lone base set, zg_prover_enable_digit_tables for a prover's three.
 * Same results, bit for bit. */
int zg_bases_enable_digit_table(zg_ctx *ctx, zg_bases *bases, uint32_t window_bits);
size_t zg_bases_len(const zg_bases *b);
uint32_t zg_bases_window_bits(const zg_bases *b);

/* Form of the MSM bucket reduction on this context: latency = 1 (default) spends two lanes per EC addition
 * (four in the suffix scan) -- shortest dependent chain, for a lone MSM or proof; latency = 0 spends one lane per addition, the
 * form for many MSMs in flight.  Results are identical.
 * zg_prover_set_overlap sets it together with the prover's own scheduling. */
int zg_ctx_set_msm_latency(zg_ctx *ctx, int latency);

/* A base set may be used from any context of the device it was registered on (the tables are read-only); it must
 * outlive every prover created on it, and zg_bases_free waits for the device to go idle. */
/* out = sum_i scalars[i] * bases[i], i < n <= zg_bases_len; == best_multiexp(scalars, &bases[..n]) */
int zg_msm(zg_ctx *ctx, const zg_bases *bases, const zg_fr *scalars, size_t n, zg_g1 *out);
/* `batch` scalar vectors against the same bases in one launch sequence; out[batch]. */
int zg_msm_batch(zg_ctx *ctx, const zg_bases *bases, const zg_fr *const *scalars, size_t batch,
                 size_t n, zg_g1 *out);
/* Device-resident scalars: vector b starts at d_scalars + b*stride_elems*32 B.  The un-normalised
 * results (extended Jacobian X,Y,ZZ,ZZZ; 128 B each) are left in d_out_xyzz[batch]; use
 * zg_msm_finish to bring them to the host as normalised zg_g1. */
int zg_msm_batch_dev(zg_ctx *ctx, const zg_bases *bases, const void *d_scalars, size_t stride_elems,
                     size_t batch, size_t n, void *d_out_xyzz);
int zg_msm_finish(zg_ctx *ctx, const void *d_xyzz, size_t batch, zg_g1 *out);
/* Host helper for point-range sharding across GPUs: out = normalised sum of `count` Jacobian
 * partials (the EC add that follows the RCCL all-gather; EC add is not an ncclRedOp). */
int zg_g1_sum(const zg_g1 *parts, size_t count, zg_g1 *out);

/* Multiexp over points that are NOT registered: the bases are an argument, as in upstream's best_multiexp(coeffs, bases)
 * (MSMKZG::eval in the verifier, a downsized or imported ParamsKZG, a gadget's own points).  No table is built and nothing
 * stays resident: every window has a bucket set of its own and the windows meet in a ladder of 254 dependent doublings per
 * vector (1.3 - 1.65 ms measured, whatever n is: DESIGN.md 13) -- the trade for points used once; points used many times belong
 * in a zg_bases.
 *   result        the host forms return NORMALISED zg_g1 as zg_msm does, the identity as (0, 1, 0); for the same points and
 *                 scalars the bytes are those of zg_msm on a registered set.
 *   window_bits   the Pippenger window width c: 0 = chosen by the library, 2..16 taken as given, anything else
 *                 ZG_ERR_INVALID_ARG.  No width changes a byte.  At 0 the width is the c in 2..16 with the least
 *                 ceil(255 / c) * (n + 4 * 2^(c-1)) -- a window adds n points into buckets and reduces 2^(c-1) buckets at
 *                 about four accumulated points each -- which is 2 or 3 below n = 32, 10 at n = 2^14 and 13 at 2^17; it is
 *                 lowered while batch * ceil(255 / c) * 2^(c-1) exceeds 2^24 bucket sums.
 *   sizes         n = 0 or batch = 0 is ZG_OK, launches nothing, and every out is the identity.  A null pointer where a
 *                 size is non-zero is ZG_ERR_INVALID_ARG.  n >= 2^23 is ZG_ERR_UNSUPPORTED (an entry names its point in 23
 *                 bits, as in a base set), and so is batch > ZG_MSM_VAR_MAX_BATCH: at c = 2 a batch of 256 is 256 * 128
 *                 bucket sets, half of what one launch grid's second dimension holds, and at c = 16 its bucket sums
 *                 (256 * 16 * 2^15 * 144 B) are 19 GB.  These are checked before anything is read or allocated.
 *   points        any points of the curve in any arrangement: (0,0) is the identity and contributes nothing, the same
 *                 point may occur any number of times, a point and its negative may both occur.  Points are NOT validated;
 *                 points off the curve give garbage, as upstream (zg_params_check is the validation).
 *   lifetime      nothing survives the call: every buffer comes from the context's workspace pool and goes back to it; no
 *                 zg_bases is created.  The context lock is held for the call. */
#define ZG_MSM_VAR_MAX_BATCH 256
/* best_multiexp(scalars, bases) with the bases as an ARGUMENT: out = sum_i scalars[i] * bases[i], i < n. */
int zg_msm_var(zg_ctx *ctx, const zg_g1_affine *bases, const zg_fr *scalars, size_t n,
               uint32_t window_bits, zg_g1 *out);
/* `batch` scalar vectors against the same n points, one launch sequence; out[batch]. */
int zg_msm_var_batch(zg_ctx *ctx, const zg_g1_affine *bases, const zg_fr *const *scalars, size_t batch,
                     size_t n, uint32_t window_bits, zg_g1 *out);
/* Device pointers, asynchronous on the context stream: d_bases n * 64 B; vector b at d_scalars + b*stride_elems*32 B
 * (stride_elems >= n); d_out_xyzz[batch] in the 128-byte form zg_msm_batch_dev leaves, finished by zg_msm_finish. */
int zg_msm_var_dev(zg_ctx *ctx, const void *d_bases, const void *d_scalars, size_t stride_elems,
                   size_t batch, size_t n, uint32_t window_bits, void *d_out_xyzz);

/* ------------------------------------------------------------------ SRS
 * Replaces ParamsKZG::<Bn256>::new(k) (reference call sites benches/bench.rs:19, src/main.rs:232):
 * g[i] = s^i * G and g_lagrange[i] = L_i(s) * G, 2^k affine points each.  Upstream draws s from
 * OsRng; here the caller supplies it so that runs are reproducible. */
int zg_params_new(zg_ctx *ctx, uint32_t k, const zg_fr *s, zg_g1_affine *g, zg_g1_affine *g_lagrange);
int zg_params_new_dev(zg_ctx *ctx, uint32_t k, const zg_fr *s, void *d_g, void *d_g_lagrange);

/* halo2_proofs::poly::kzg::commitment: g_to_lagrange(g[..2^k], k), as ParamsKZG::downsize and
 * ParamsKZG::from_parts-style imports use it: best_fft over G1 with omega_inv, then * 2^-k.
 * Reads the FIRST 2^k points of g (so a larger SRS is downsized by passing its prefix);
 * writes 2^k affine points, identity = (0,0).  No scalar is needed.
 * k <= 24 (else ZG_ERR_UNSUPPORTED).  The result is bit-exact: canonical affine Montgomery coordinates, whatever the
 * order of the additions.  The input may hold identities and repeated points: this is a transform, not a validation
 * (points off the curve give points off the curve; zg_params_check is the validation).  The _dev form takes device
 * pointers (2^k * 64 B each; d_g == d_g_lagrange is ZG_ERR_INVALID_ARG), is asynchronous on the context stream like
 * every _dev entry, and its output can go straight into zg_bases_register_dev. */
int zg_params_lagrange(zg_ctx *ctx, uint32_t k, const zg_g1_affine *g, zg_g1_affine *g_lagrange);
int zg_params_lagrange_dev(zg_ctx *ctx, uint32_t k, const void *d_g, void *d_g_lagrange);

/* Is this an SRS?  *verdict = 1 accepted / 0 rejected; *failed = why (ZG_SRS_* bits below, 0 when accepted).
 * g: 2^k points, g_lagrange: 2^k points or NULL (then ZG_SRS_LAGRANGE is not evaluated), g2 / s_g2: ParamsVerifierKZG's.
 *   ZG_SRS_G1_MALFORMED  a G1 coordinate's limbs are not below q, or a point is off y^2 = x^3 + 3 (g or g_lagrange;
 *                        an identity in g_lagrange is a point of the curve)
 *   ZG_SRS_G1_IDENTITY   some g[i] is the identity
 *   ZG_SRS_G2            g2 or s_g2 is non-canonical, off the twist, the identity, or outside the r-torsion (r Q != inf)
 *   ZG_SRS_POWERS        g is no geometric sequence under s_g2: with r_i = rand_fr(key, TAG_SRS_POWERS, i), i < 2^k - 1,
 *                        A = sum r_i g[i] and B = sum r_i g[i+1] (one MSM batch over one base set),
 *                        e(B, g2) e(-A, s_g2) != 1.  k = 0 has no such relation and passes it.
 *   ZG_SRS_LAGRANGE      g_lagrange is not the Lagrange basis of g: with c_j = rand_fr(key, TAG_SRS_LAGRANGE, j) and
 *                        e = the evaluations of sum c_j X^j on the domain (device NTT), sum e_i g_lagrange[i] != sum c_j g[j]
 * The first three are decided point by point, and zg_last_error() names the first offending index; the two relations are
 * evaluated, each on its own, only when those three are clear.  The scalars are drawn on the device, as the prover's
 * blinding rows are; the base sets the check registers are freed before it returns; the pairing runs on the host after
 * the context lock is released.  k <= 22 (what a base set holds), else ZG_ERR_UNSUPPORTED.
 * `key` MUST come from the caller's CSPRNG: whoever made the file and knows the key can choose errors that cancel in the
 * weighted sums.  What the check does NOT do: it does not require g[0] to be the curve generator (a ceremony may start
 * from another point, and the verifier takes g0 as an argument anyway), and it does not replace the verification of a
 * ceremony's own transcript -- it says that the file is A structured reference string, not whose.
 * Returns the zg_status of the call itself: a rejected SRS is not an error of the call. */
enum { ZG_SRS_G1_MALFORMED = 1, ZG_SRS_G1_IDENTITY = 2, ZG_SRS_G2 = 4, ZG_SRS_POWERS = 8, ZG_SRS_LAGRANGE = 16 };
int zg_params_check(zg_ctx *ctx, uint32_t k, const zg_g1_affine *g,
                    const zg_g1_affine *g_lagrange /* may be NULL */,
                    const zg_g2_affine *g2, const zg_g2_affine *s_g2,
                    const uint8_t key[32], int *verdict, uint32_t *failed);

/* out[i] = scalars[i] * points[i], i < n: n independent variable-base multiplications (what an SRS contribution is made
 * of; upstream would write `points.iter().zip(scalars).map(|(p, s)| p * s)` and normalise).  Scalars are Montgomery
 * residues, as zg_msm takes them.  Points may be any points of the curve, (0,0), repeats and P beside -P included; they
 * are not validated (a point off the curve gives garbage in ITS slot).  A zero scalar or an identity point gives (0,0)
 * and disturbs no neighbour.  The output is affine, canonical Montgomery coordinates, hence bit-exact whatever the
 * order of the operations.  n = 0 is ZG_OK and launches nothing; a null pointer with n > 0 is ZG_ERR_INVALID_ARG;
 * n >= 2^28 is ZG_ERR_UNSUPPORTED.  The _dev form takes device pointers (points and out n * 64 B, scalars n * 32 B;
 * d_out == d_points is allowed) and is asynchronous on the context stream.  One lane per point, signed 2-bit windows,
 * one shared inversion per wave. */
int zg_g1_mul_each(zg_ctx *ctx, const zg_g1_affine *points, const zg_fr *scalars, size_t n, zg_g1_affine *out);
int zg_g1_mul_each_dev(zg_ctx *ctx, const void *d_points, const void *d_scalars, size_t n, void *d_out);

/* The 32-byte GroupEncoding of G1 points (halo2curves 0.3.3 G1Affine::to_bytes / from_bytes; what halo2's own transcript
 * writes into a proof, ZG_TRANSCRIPT_BLAKE2B below).  As known from the published sources -- the crates were not at hand;
 * DESIGN.md section 17 lists what remains to be verified against them:
 *   to_bytes    the identity is 32 zero bytes; otherwise x.to_repr() (32 little-endian bytes of the canonical integer)
 *               with (y.to_repr()[0] & 1) << 7 OR-ed into byte 31; bit 6 of byte 31 is always 0.
 *   from_bytes  bit 7 of byte 31 is the sign and is cleared; the remaining 32 bytes must be a canonical x < q (a set bit 6
 *               therefore fails here); x = 0 with sign 0 is the identity; otherwise y = sqrt(x^3 + 3) -- the encoding is
 *               invalid when there is none -- negated when its low bit differs from the sign.  q = 3 (mod 4): the root is
 *               t^((q+1)/4), checked by squaring; 3 is a non-residue, so x = 0 with the sign set is invalid.
 * zg_g1_compress is to_bytes for n points on the host (no device); it does not validate: a point off the curve gives bytes
 * that do not decompress to it.  zg_g1_decompress is from_bytes for n encodings on the GPU, one lane per point: out[i] is
 * the affine point in Montgomery form and valid[i] = 1 (the identity encoding: (0,0), valid 1); an invalid encoding gives
 * (0,0) with valid[i] = 0, disturbs no neighbour and is not an error of the call.  n = 0 is ZG_OK and launches nothing; a
 * null pointer with n > 0 is ZG_ERR_INVALID_ARG; n >= 2^28 is ZG_ERR_UNSUPPORTED.  The _dev form takes device pointers
 * (d_in n * 32 B, d_out n * 64 B, d_valid n bytes; d_out may not alias d_in) and is asynchronous on the context stream. */
typedef struct { uint8_t b[32]; } zg_g1_compressed;
int zg_g1_compress(const zg_g1_affine *points, size_t n, zg_g1_compressed *out);
int zg_g1_decompress(zg_ctx *ctx, const zg_g1_compressed *in, size_t n, zg_g1_affine *out, uint8_t *valid);
int zg_g1_decompress_dev(zg_ctx *ctx, const void *d_in, size_t n, void *d_out, void *d_valid);

/* The G2 half of ParamsKZG::new (ParamsKZG::setup: g2 = G2Affine::generator(), s_g2 = g2 * s), on the host: with
 * zg_params_new it makes a complete ParamsKZG, which zg_verifier_create and an SRS file need.  s: Montgomery, limbs
 * below r (else ZG_ERR_INVALID_ARG); s = 0 gives s_g2 = (0,0). */
int zg_params_g2(const zg_fr *s, zg_g2_affine *g2, zg_g2_affine *s_g2);
/* out = t * q on the twist, on the host; the identity is (0,0), as input and as output (t = 0, or t = the order of q).
 * A q with a coordinate not below q or off y^2 = x^3 + 3/(9+u), and a t whose limbs are not below r, are
 * ZG_ERR_INVALID_ARG and leave out as it was.  The subgroup is not asked for (zg_params_check does that). */
int zg_g2_mul(const zg_g2_affine *q, const zg_fr *t, zg_g2_affine *out);

/* One contribution to an updatable SRS: the string of s becomes the string of s*t,
 *     g_out[i] = t^i * g[i] (i < 2^k),   s_g2_out = t * s_g2,   g_lagrange_out = g_to_lagrange(g_out),   g2 unchanged,
 * and *record = (t * g[0], t * g2) is the public half of the step, which zg_params_check_update reads.  Parties that
 * each apply a t of their own, one after the other, end with an SRS whose scalar nobody knows if ONE of them forgot
 * theirs.  The powers t^i are made on the device and multiplied through the kernel of zg_g1_mul_each; g_lagrange_out
 * (may be NULL: not computed) comes from the path of zg_params_lagrange_dev and never visits the host; the two G2
 * products run on the host.  t = 0 or limbs not below r is ZG_ERR_INVALID_ARG, k > 24 ZG_ERR_UNSUPPORTED, a g2 or s_g2
 * that zg_g2_mul refuses ZG_ERR_INVALID_ARG: all are decided before anything is written.  g_out may be g.  The _dev
 * form takes device pointers (d_g_out may equal d_g; d_g_lagrange_out may be NULL, and may be neither of the other
 * two), does the G1 part only and is asynchronous on the context stream.
 * The workspace that held the powers of t is zeroed before it returns to the context's pool.  That is best effort:
 * t itself travels in kernel arguments, and registers and LDS are not cleared; a caller who must forget t forgets its
 * own copy and destroys the context. */
typedef struct { zg_g1_affine t_g1; zg_g2_affine t_g2; } zg_srs_contribution;
int zg_params_update(zg_ctx *ctx, uint32_t k, const zg_fr *t,
                     const zg_g1_affine *g, const zg_g2_affine *g2, const zg_g2_affine *s_g2,
                     zg_g1_affine *g_out, zg_g1_affine *g_lagrange_out /* may be NULL */,
                     zg_g2_affine *s_g2_out, zg_srs_contribution *record);
int zg_params_update_dev(zg_ctx *ctx, uint32_t k, const zg_fr *t, const void *d_g, void *d_g_out /* may equal d_g */,
                         void *d_g_lagrange_out /* may be NULL */);

/* Is `next` the update of `prev` that `record` describes?  *verdict / *failed as zg_params_check, with two more bits:
 *   (a) zg_params_check(k, g_next, g_lagrange_next, g2, s_g2_next, key) accepts -- the same code, the same bits;
 *   (b) ZG_SRS_UPDATE_BASE  g_next[0] is not prev g[0] (a step multiplies g[0] by t^0);
 *   (c) ZG_SRS_UPDATE_LINK  record->t_g2 is non-canonical, off the twist, the identity or outside the r-torsion;
 *                           record->t_g1 is non-canonical, off the curve or the identity; or one of
 *                           e(t_g1, g2) = e(prev g[0], t_g2) (the record's halves carry ONE t) and
 *                           e(g_next[1], g2) = e(prev g[1], t_g2) (g_next[1] = t * prev g[1]) fails.
 * With (a), (c) fixes every g_next[i] and s_g2_next.  prev_g01: the previous string's g[0] and g[1] -- all of it that
 * the check needs.  k = 0 has no g[1]: ZG_ERR_INVALID_ARG; k > 22 ZG_ERR_UNSUPPORTED, as for zg_params_check.  A
 * rejected step is not an error of the call.  Both pairings run on the host.
 * What this is NOT: there is no hash-chained transcript and no random beacon, and the pair (t_g1, t_g2) is a
 * knowledge-of-exponent style record of one step, not a ceremony protocol -- who contributed, in what order, and that
 * nobody adapted a t to a later party's are a ceremony's to establish. */
enum { ZG_SRS_UPDATE_BASE = 32, ZG_SRS_UPDATE_LINK = 64 };
int zg_params_check_update(zg_ctx *ctx, uint32_t k, const zg_g1_affine prev_g01[2] /* prev g[0], g[1] */,
                           const zg_g1_affine *g_next, const zg_g1_affine *g_lagrange_next /* may be NULL */,
                           const zg_g2_affine *g2, const zg_g2_affine *s_g2_next,
                           const zg_srs_contribution *record, const uint8_t key[32], int *verdict, uint32_t *failed);

/* ------------------------------------------------------------------ NTT
 * Replaces halo2_proofs::arithmetic::best_fft and the EvaluationDomain wrappers
 * (halo2_proofs/src/poly/domain.rs upstream: lagrange_to_coeff, coeff_to_extended,
 * extended_to_coeff, divide_by_vanishing_poly).                                             */

/* In place, natural order in and out: a[k] <- sum_j a[j] * omega^(j*k); a has 2^log_n entries. */
int zg_ntt(zg_ctx *ctx, zg_fr *a, uint32_t log_n, const zg_fr *omega);
/* EvaluationDomain::ifft: best_fft with omega_inv followed by the multiplication by `divisor`. */
int zg_intt(zg_ctx *ctx, zg_fr *a, uint32_t log_n, const zg_fr *omega_inv, const zg_fr *divisor);
int zg_ntt_batch(zg_ctx *ctx, zg_fr *const *a, size_t batch, uint32_t log_n, const zg_fr *omega);
int zg_intt_batch(zg_ctx *ctx, zg_fr *const *a, size_t batch, uint32_t log_n,
                  const zg_fr *omega_inv, const zg_fr *divisor);
/* Device-resident, in place; array b at d_a + b*stride_elems*32 B.  divisor may be NULL. */
int zg_ntt_batch_dev(zg_ctx *ctx, void *d_a, size_t stride_elems, size_t batch, uint32_t log_n,
                     const zg_fr *omega, const zg_fr *divisor);

/* EvaluationDomain::coeff_to_extended: coefficient i is multiplied by g_coset^(i mod 3) (g_coset: the context's
 * generator, zg_ctx_set_coset_generator), zero-padded from 2^k to 2^ext_k and transformed with extended_omega. */
int zg_coeff_to_extended(zg_ctx *ctx, const zg_fr *coeffs, uint32_t k, uint32_t ext_k, zg_fr *out);
int zg_coeff_to_extended_batch_dev(zg_ctx *ctx, const void *d_coeffs, size_t in_stride_elems,
                                   void *d_out, size_t out_stride_elems, size_t batch, uint32_t k,
                                   uint32_t ext_k);
/* EvaluationDomain::extended_to_coeff: inverse transform on the extended domain, multiplication by
 * 2^-ext_k and by g_coset^-(i mod 3), truncated to out_len (= n * quotient_poly_degree). evals is
 * clobbered. */
int zg_extended_to_coeff(zg_ctx *ctx, zg_fr *evals, uint32_t k, uint32_t ext_k, size_t out_len,
                         zg_fr *out);
int zg_extended_to_coeff_dev(zg_ctx *ctx, void *d_evals, uint32_t k, uint32_t ext_k, size_t out_len,
                             void *d_out);

/* The standard domain roots: omega = ROOT_OF_UNITY^(2^(28-log_n)) and its inverse. */
int zg_domain_omega(uint32_t log_n, zg_fr *omega, zg_fr *omega_inv);

/* ------------------------------------------------------------------ evaluation domain
 * EvaluationDomain's extended coset is g_coset * <extended_omega>, with g_coset = <Fr as WithSmallOrderMulGroup<3>>::ZETA
 * upstream: one of the TWO primitive cube roots of unity of Fr, each the other's square.  The library takes it as a
 * parameter.  The DEFAULT is zg_fr_cube_root(0) = 7^((r-1)/3) = 0x...b99c90dd, because that is the value the golden vectors
 * and the oracle were made with; whether upstream's literal is this one or its square (0x30644e72...36636f23) has not
 * been verified against halo2curves here, so no constant in the source decides it: a shim passes
 * <Fr as WithSmallOrderMulGroup<3>>::ZETA at run time.  Proof bytes do NOT depend on the
 * choice (the quotient h is unique); what does are the arrays of the arithmetic-level entries -- zg_coeff_to_extended*,
 * zg_extended_to_coeff*, zg_prover_evaluate_h, zg_prover_fetch(what = 0) and the extended families of
 * zg_prover_export_key -- which a caller mixes with its own pk.fixed_cosets / l0 only under the same generator. */
/* Host helper: which = 0: 7^((r-1)/3), the default; which = 1: its square.  Montgomery form. */
int zg_fr_cube_root(uint32_t which, zg_fr *out);
/* g_coset of this context: governs zg_coeff_to_extended* and zg_extended_to_coeff* on it (and on its side stream), and is
 * captured by zg_prover_create*.  Accepts exactly the two primitive cube roots of unity; anything else (0, 1, 7, a value
 * not below r) is ZG_ERR_INVALID_ARG and leaves the setting as it was.  Provers that already exist are not touched. */
int zg_ctx_set_coset_generator(zg_ctx *ctx, const zg_fr *g_coset);
int zg_ctx_coset_generator(zg_ctx *ctx, zg_fr *out);

/* ------------------------------------------------------------------ circuit description
 * What halo2 keeps in `ConstraintSystem` + `ProvingKey` (halo2_proofs v2023_04_20
 * src/plonk/circuit.rs, src/plonk/keygen.rs), flattened to plain arrays so that it can cross a C ABI.
 * For zero_g it is produced from `WnnCircuit::configure` (/root/reference/src/gadgets/wnn.rs:334-371,
 * chips configured at wnn.rs:125-172); SURVEY.md appendix A lists its 12 gate polynomials,
 * 4 lookups and 8 permutation columns.  Every polynomial (gate, lookup input, lookup table) is given
 * in expanded form sum_m coeff_m * prod_f cell(query_f): exact over the field, so the value is the
 * one halo2's Expression tree / GraphEvaluator computes. */
enum { ZG_FIXED = 0, ZG_ADVICE = 1, ZG_INSTANCE = 2, ZG_CHALLENGE = 3 };
enum { ZG_MAX_FACTORS = 8, ZG_MAX_LOOKUP_WIDTH = 4 };
/* create_proof's phases (FirstPhase / SecondPhase / ThirdPhase) and Expression::Challenge: see zg_prover_set_phases */
enum { ZG_MAX_CHALLENGES = 16, ZG_MAX_PHASES = 3 };

typedef struct {
    uint32_t kind;      /* ZG_FIXED / ZG_ADVICE / ZG_INSTANCE, or ZG_CHALLENGE: Expression::Challenge(column), rotation 0 */
    uint32_t column;    /* (ZG_CHALLENGE: the challenge's index, < ZG_MAX_CHALLENGES; a circuit has 1 + the largest index used) */
    int32_t rotation;   /* Rotation(i32): row offset in the 2^k domain */
} zg_query;

typedef struct {
    zg_fr coeff;                          /* Montgomery form */
    uint32_t n_factors;                   /* 0 = constant term */
    uint32_t factors[ZG_MAX_FACTORS];     /* indices into zg_circuit.queries */
} zg_monomial;

typedef struct { uint32_t first, count; } zg_poly;   /* range in zg_circuit.monomials */

typedef struct {
    uint32_t width;                              /* tuple length m (same for inputs and table) */
    zg_poly inputs[ZG_MAX_LOOKUP_WIDTH];         /* lookup::Argument::input_expressions */
    zg_poly tables[ZG_MAX_LOOKUP_WIDTH];         /* lookup::Argument::table_expressions */
} zg_lookup;

/* halo2's shuffle argument (ConstraintSystem::shuffle; privacy-scaling-explorations/halo2 v0.3.0 on): over the usable rows
 * the tuples (inputs[0..width)) are a permutation of the tuples (shuffles[0..width)).  The layout is zg_lookup's; the
 * expressions' monomials stand in zg_circuit.monomials with everything else's.  A circuit's shuffles are no part of
 * zg_circuit: they are handed to zg_prover_create_shuffles / zg_verifier_create_shuffles beside it. */
typedef struct {
    uint32_t width;                              /* tuple length m, 1 .. ZG_MAX_LOOKUP_WIDTH */
    zg_poly inputs[ZG_MAX_LOOKUP_WIDTH];         /* shuffle::Argument::input_expressions */
    zg_poly shuffles[ZG_MAX_LOOKUP_WIDTH];       /* shuffle::Argument::shuffle_expressions */
} zg_shuffle;
enum { ZG_MAX_SHUFFLES = 16 };

typedef struct {
    uint32_t k;                  /* rows = 2^k */
    uint32_t cs_degree;          /* ConstraintSystem::degree(); extended domain = smallest 2^e >= 2^k*(degree-1) */
    uint32_t blinding_factors;   /* ConstraintSystem::blinding_factors(); last rotation = -(bf+1) */
    uint32_t n_fixed, n_advice, n_instance;
    uint32_t n_queries;        const zg_query *queries;
    uint32_t n_monomials;      const zg_monomial *monomials;
    uint32_t n_gates;          const zg_poly *gates;         /* gate polynomials in creation order */
    uint32_t n_lookups;        const zg_lookup *lookups;
    uint32_t n_perm_columns;   const zg_query *perm_columns; /* permutation::Argument::columns (rotation unused) */
    uint32_t n_advice_queries; const zg_query *advice_queries;  /* cs.advice_queries: order of the advice evals */
    uint32_t n_fixed_queries;  const zg_query *fixed_queries;   /* cs.fixed_queries  */
} zg_circuit;

/* ------------------------------------------------------------------ prover
 * Replaces halo2_proofs::plonk::create_proof::<KZGCommitmentScheme<Bn256>, ProverGWC, _, _,
 * EvmTranscript, _> for ONE circuit instance, as Wnn::proof calls it
 * (/root/reference/src/wnn.rs:242-259), from "advice columns assigned" to "proof bytes":
 * commitments (MSM), lagrange_to_coeff / coeff_to_extended (NTT), lookup::prover::{commit_permuted,
 * commit_product}, permutation::prover::commit, vanishing::prover::{commit, construct, evaluate},
 * Evaluator::evaluate_h, eval_polynomial and ProverGWC::create_proof, with the Keccak-256
 * EvmTranscript of snark-verifier (wnn.rs:21,249).  Witness synthesis (the Rust WnnChip) stays on the
 * caller's side: advice arrives as column values.
 *
 * Randomness: upstream draws every blinding scalar from OsRng (wnn.rs:256).  Here each one is
 * rand_fr(key, purpose tag, index): the ChaCha20 (RFC 7539) keystream under a 32-byte key supplied by the caller,
 * nonce = (tag, index), rejection-sampled below r.  A caller who passes 32 fresh bytes from its own
 * CSPRNG (the Rust shim: OsRng.fill_bytes) gets blinding that is as hidden as that key; a fixed key makes the proof
 * reproducible, which is what lets the oracle produce the same bytes -- tests use small integers as keys
 * (little-endian, zero-padded), production callers must not. */
typedef struct zg_prover zg_prover;

/* Uploads the proving key material and derives what keygen_pk derives (fixed/sigma polys and their
 * extended cosets, l_0 / l_last / l_active_row cosets).  fixed_values: [n_fixed][2^k] Lagrange values;
 * sigma_values: [n_perm_columns][2^k] Lagrange values of the permutation polynomials
 * (pk.permutation.permutations); g / g_lagrange: ParamsKZG; vk_repr: vk.transcript_repr, the scalar
 * create_proof hashes into the transcript first.  All host pointers, copied. */
int zg_prover_create(zg_ctx *ctx, const zg_circuit *circuit, const zg_fr *fixed_values,
                     const zg_fr *sigma_values, const zg_g1_affine *g, const zg_g1_affine *g_lagrange,
                     const zg_fr *vk_repr, zg_prover **out);
/* Same, with base tables registered once per device (zg_bases_register on any context of that device)
 * and shared read-only by several provers / proof streams: the window tables are the largest resident
 * object (2 * W * 2^k * 64 B) and sharing them keeps them in the Infinity Cache.  The bases must outlive
 * the prover and use the same window size.  Base sets with FEWER than 2^k points are a point-range shard of the
 * SRS: see zg_prover_set_shard. */
int zg_prover_create_shared(zg_ctx *ctx, const zg_circuit *circuit, const zg_fr *fixed_values,
                            const zg_fr *sigma_values, const zg_bases *g, const zg_bases *g_lagrange,
                            const zg_fr *vk_repr, zg_prover **out);
/* zg_prover_create / zg_prover_create_shared for a circuit with shuffle arguments (n_shuffles = 0: the same call).  Per
 * shuffle j the prover commits one product z_j where the lookup products are committed -- z_j[0] = 1,
 * z_j[r + 1] = z_j[r] (a[r] + gamma) / (s[r] + gamma) over the usable rows, a and s the theta-folds of the two tuples as the
 * lookups fold theirs, the blinding_factors rows behind them rand_fr(key, 10, j * blinding_factors + i) for the i-th -- adds l_0 (1 - z), l_last (z^2 - z) and
 * (1 - (l_last + l_blind)) (z(wX) (s + gamma) - z(X) (a + gamma)) to the quotient behind all lookup terms, and evaluates
 * and opens z_j at x and omega x behind the lookups' (DESIGN.md section 19).  circuit->cs_degree must cover
 * max(2 + deg a, 2 + deg s), an expression's degree counting as at least 1.  A witness that is no shuffle still yields
 * ZG_OK and a proof of full length, which no verifier accepts (upstream checks the product only under its sanity-check
 * feature).  ZG_ERR_INVALID_ARG: a null array with a count, a width of 0 or above ZG_MAX_LOOKUP_WIDTH, a polynomial outside
 * the monomials, a cs_degree below the shuffles'; ZG_ERR_UNSUPPORTED: more than ZG_MAX_SHUFFLES.
 * A prover with shuffles makes single proofs and lock-step batches (zg_prover_prove, _dev, _batch, _batch_dev, _phased);
 * zg_prover_prove_multi* of several circuits, zg_prover_prove_images*, zg_prover_check_batch, _batch_dev and _images (a
 * witness of such a circuit is checked by zg_prover_check_circuit*), a point-range shard and the arithmetic-level entries
 * that take the whole circuit (zg_prover_evaluate_h*) answer ZG_ERR_UNSUPPORTED.  One proof of several such circuits is
 * made by zg_prover_prove_circuits* and verified by zg_verifier_verify_circuits; input -> proof and input -> check go
 * through zg_prover_prove_inputs* and zg_prover_check_inputs. */
int zg_prover_create_shuffles(zg_ctx *ctx, const zg_circuit *circuit, const zg_shuffle *shuffles, uint32_t n_shuffles,
                              const zg_fr *fixed_values, const zg_fr *sigma_values, const zg_g1_affine *g,
                              const zg_g1_affine *g_lagrange, const zg_fr *vk_repr, zg_prover **out);
int zg_prover_create_shared_shuffles(zg_ctx *ctx, const zg_circuit *circuit, const zg_shuffle *shuffles, uint32_t n_shuffles,
                                     const zg_fr *fixed_values, const zg_fr *sigma_values, const zg_bases *g,
                                     const zg_bases *g_lagrange, const zg_fr *vk_repr, zg_prover **out);
/* the number of shuffle arguments of the prover's circuit */
uint32_t zg_prover_shuffles(const zg_prover *p);
/* A second prover on the SAME proving key (no copy: the key's HBM is shared and freed with its last prover) and
 * the same base tables (tables the parent registered itself are owned jointly and freed with the last prover; tables
 * the caller registered stay the caller's), on another context of the device -- another stream of proofs or proof
 * batches. */
int zg_prover_fork(const zg_prover *parent, zg_ctx *ctx, zg_prover **out);
void zg_prover_destroy(zg_prover *p);
/* g_coset of the prover's proving key: the generator of the context it was created on, at that time
 * (zg_ctx_set_coset_generator).  A fork shares the key and so its generator, whatever its own context says; changing a
 * context later changes no existing prover. */
int zg_prover_coset_generator(const zg_prover *p, zg_fr *out);
/* What keygen_pk derives (halo2_proofs src/plonk/keygen.rs: pk.fixed_polys / fixed_cosets, pk.permutation.polys / cosets,
 * pk.l0 / l_last / l_active_row), copied from the prover's resident key to the host.  ZG_KEY_FIXED_POLY / ZG_KEY_SIGMA_POLY:
 * [2^k] coefficients of fixed column / permutation column `index`; ZG_KEY_FIXED_COSET / ZG_KEY_SIGMA_COSET and ZG_KEY_L0 /
 * ZG_KEY_L_LAST / ZG_KEY_L_ACTIVE_ROW (index 0): [2^ext_k] values.  Every array is in plain Montgomery form and halo2's
 * order; the extended ones sit on the single coset g_coset * <extended_omega> of the prover's generator, whichever layout
 * evaluate_h reads (split parts, 2^5-scaled nine-limb slabs, scaled sigma).  An index outside its family (any index of
 * the sigma families of a circuit without permutation columns) is ZG_ERR_INVALID_ARG.  Works on forks; reads the key
 * only, so a later proof is not disturbed.  The commitments are zg_prover_vk_commitments. */
enum { ZG_KEY_FIXED_POLY = 0, ZG_KEY_SIGMA_POLY = 1, ZG_KEY_FIXED_COSET = 2, ZG_KEY_SIGMA_COSET = 3, ZG_KEY_L0 = 4,
       ZG_KEY_L_LAST = 5, ZG_KEY_L_ACTIVE_ROW = 6 };
int zg_prover_export_key(zg_prover *p, uint32_t family, uint32_t index, zg_fr *out, size_t cap_elems);

/* Lock-step batches.  A prover has `max_batch` proof slots (1 after creation); zg_prover_prove_batch makes up to
 * that many proofs of the same circuit AT ONCE: every kernel launch of create_proof serves all of them (the
 * commitments of a phase are one MSM over batch x columns vectors, the transforms one NTT batch, evaluate_h one
 * grid with a row of workgroups per proof ...), while each proof keeps its own transcript, challenges and
 * blinding key.  Proof bytes are those of the one-at-a-time calls. */
int zg_prover_set_batch(zg_prover *p, size_t max_batch);
size_t zg_prover_batch(const zg_prover *p);
/* Device address of slot `slot`'s advice columns, [n_advice][2^k] (a witness generator may write there directly);
 * valid until the next zg_prover_set_batch. */
void *zg_prover_advice_slot(zg_prover *p, size_t slot);
/* count <= max_batch proofs.  advice[b]: [n_advice][2^k] column values of proof b (host), or NULL when the slot
 * already holds them; the last blinding_factors+1 rows are overwritten with blinding scalars as create_proof does.
 * instance[b]: [n_instance][instance_len].  rng_keys: count x 32 bytes.  proofs[b] (proof_cap bytes each) receives
 * proof b's transcript bytes, proof_lens[b] their length (0 on failure), statuses[b] (optional) its zg_status: a
 * witness that fails a lookup fails ITS proof (ZG_ERR_CONSTRAINT), the others complete.  Returns the first
 * non-zero status. */
int zg_prover_prove_batch(zg_prover *p, size_t count, const zg_fr *const *advice, const zg_fr *const *instance,
                          size_t instance_len, const uint8_t *rng_keys, uint8_t *const *proofs, size_t proof_cap,
                          size_t *proof_lens, int *statuses);
/* Same with the advice columns in HBM: d_advice[b] is a device pointer (copied into the slot unless it IS the slot,
 * zg_prover_advice_slot) or NULL = the slot as it stands; d_advice itself may be NULL. */
int zg_prover_prove_batch_dev(zg_prover *p, size_t count, void *const *d_advice, const zg_fr *const *instance,
                              size_t instance_len, const uint8_t *rng_keys, uint8_t *const *proofs,
                              size_t proof_cap, size_t *proof_lens, int *statuses);
/* ONE proof of several instances of the circuit: halo2_proofs::plonk::create_proof's `circuits: &[C]` /
 * `instances: &[&[&[F]]]` slice (v2023_04_20 src/plonk/prover.rs) -- every instance behind one transcript, one set of
 * challenges, one quotient h, one random polynomial, one GWC opening.  The `circuits` slots of the prover are the
 * circuits (1 <= circuits <= zg_prover_batch(p), else ZG_ERR_INVALID_ARG; more than 64, or a point-range shard:
 * ZG_ERR_UNSUPPORTED).  advice[c], instance[c]: as zg_prover_prove_batch takes them.  rng_keys: circuits x 32 bytes --
 * circuit c draws its blinding rows from key c (tags and indices of the one-circuit proof), the random polynomial comes
 * from key 0.  Transcript order, the fold of the quotients and the limits: DESIGN.md section 11.  A lookup failure in ANY
 * circuit fails the call (ZG_ERR_CONSTRAINT, *proof_len = 0; the message names the circuit).  circuits = 1 gives
 * zg_prover_prove's bytes.  After such a proof zg_prover_fetch_slot(p, 0, 0, ...) returns the FOLDED h (the proof's
 * quotient), other slots' item 0 their own circuit's. */
size_t zg_prover_proof_size_multi(const zg_prover *p, size_t circuits); /* upper bound, bytes */
int zg_prover_prove_multi(zg_prover *p, size_t circuits, const zg_fr *const *advice, const zg_fr *const *instance,
                          size_t instance_len, const uint8_t *rng_keys, uint8_t *proof, size_t proof_cap,
                          size_t *proof_len);
/* Same with the advice columns in HBM, as zg_prover_prove_batch_dev takes them. */
int zg_prover_prove_multi_dev(zg_prover *p, size_t circuits, void *const *d_advice, const zg_fr *const *instance,
                              size_t instance_len, const uint8_t *rng_keys, uint8_t *proof, size_t proof_cap,
                              size_t *proof_len);
/* The general form of zg_prover_prove_multi / _dev: ONE proof of `circuits` instances of ANY circuit the library proves,
 * those with shuffle arguments, challenges and advice phases included.  Arguments, keys, limits
 * and statuses are zg_prover_prove_multi's: 1 <= circuits <= zg_prover_batch(p) else ZG_ERR_INVALID_ARG; more than 64
 * circuits or a point-range shard ZG_ERR_UNSUPPORTED; a lookup failure in any circuit ZG_ERR_CONSTRAINT with
 * *proof_len = 0.  zg_prover_proof_size_multi is the bound for these entries too: it is computed from the circuit's shape,
 * which counts the shuffle arguments, and the phases change no length.  On a circuit without shuffles, challenges and
 * later phases the entries ARE zg_prover_prove_multi / _dev (the same bytes, the same kernel launches); circuits = 1 is
 * zg_prover_prove / zg_prover_prove_phased, byte for byte.
 *
 * The proof, with N = circuits: the vk scalar and every circuit's instance scalars; per phase in ascending order every
 * circuit's advice commitments of that phase (circuit after circuit, ascending column) and then ONE squeeze per challenge
 * of that phase, theta behind the last phase; every circuit's permuted columns, beta, gamma; every circuit's permutation
 * products, then every circuit's lookup products, then every circuit's shuffle products, the random polynomial once, y;
 * the pieces of h once, x; the evaluations in zg_prover_prove_multi's order with every circuit's z_j(x), z_j(omega x) behind
 * every circuit's lookup evaluations; the opening queries circuit after circuit (advice, permutation, lookups, shuffles),
 * then fixed, sigmas, h, random; either multi-open tail.  h = sum_c y^(m (N - 1 - c)) h_c with m = gates + permutation
 * terms + 5 per lookup + 3 per shuffle.  Circuit c draws every blinding row -- advice, permuted columns, every product,
 * the shuffle products under their own tag -- from key c with the tags and indices of the single proof; the random
 * polynomial comes from key 0.  A witness that is no shuffle still gives ZG_OK and a proof of full length that no
 * verifier accepts.
 *
 * The plain forms take a circuit with challenges while every advice column is in phase 0 and return ZG_ERR_INVALID_ARG
 * otherwise (use zg_prover_prove_circuits_phased), as the single-proof entries do.  _phased: fn is called once per phase
 * with count = circuits, d_advice[c] the slot of circuit c and challenges [circuits][n_challenges], every row the same
 * values (one transcript); the rest is zg_prover_prove_phased's contract -- a non-zero return gives ZG_ERR_INVALID_ARG,
 * *proof_len = 0, the queue drained and the prover usable. */
int zg_prover_prove_circuits(zg_prover *p, size_t circuits, const zg_fr *const *advice, const zg_fr *const *instance,
                             size_t instance_len, const uint8_t *rng_keys, uint8_t *proof, size_t proof_cap,
                             size_t *proof_len);
int zg_prover_prove_circuits_dev(zg_prover *p, size_t circuits, void *const *d_advice, const zg_fr *const *instance,
                                 size_t instance_len, const uint8_t *rng_keys, uint8_t *proof, size_t proof_cap,
                                 size_t *proof_len);
/* One proof (the batch of one).  advice: [n_advice][2^k] column values (host).  instance: [n_instance][instance_len]
 * public inputs.  proof: receives the transcript bytes (EvmTranscript layout). */
int zg_prover_prove(zg_prover *p, const zg_fr *advice, const zg_fr *instance, size_t instance_len,
                    const uint8_t rng_key[32], uint8_t *proof, size_t proof_cap, size_t *proof_len);
/* Same with the advice columns already in HBM ([n_advice][2^k]; copied into slot 0 unless they are slot 0). */
int zg_prover_prove_dev(zg_prover *p, void *d_advice, const zg_fr *instance, size_t instance_len,
                        const uint8_t rng_key[32], uint8_t *proof, size_t proof_cap, size_t *proof_len);

/* Advice phases and challenges: create_proof's multi-phase schedule (halo2_proofs v2023_04_20 src/plonk/prover.rs;
 * ConstraintSystem::advice_column_in, challenge_usable_after, Expression::Challenge).  After the vk
 * scalar and the instances the prover runs, for each phase in ascending order: the commitments of the advice columns of
 * that phase (ascending column) into the transcript, then one squeeze per challenge of that phase (ascending index).
 * theta follows the last phase.  Only the ORDER OF THE ADVICE COMMITMENTS at the head of a proof depends on the phases:
 * evaluations, opening queries and the proof's length do not.  A ZG_CHALLENGE query evaluates to its challenge and has
 * degree 0; it may stand in gates, lookup inputs and lookup tables.
 *
 * advice_phase: [n_advice] phases (may be NULL without advice columns); challenge_phase: [n_challenges] the phase after
 * which each challenge is squeezed.  Before the call every advice column is in phase 0 and every challenge the circuit
 * uses is squeezed after phase 0.  ZG_ERR_INVALID_ARG, and nothing changes, when a phase is >= ZG_MAX_PHASES, when a phase
 * up to the last one used has no advice column (phases are contiguous from 0), when n_challenges is smaller than the
 * circuit's count (1 + the largest index a ZG_CHALLENGE query names) or larger than ZG_MAX_CHALLENGES, or when a
 * challenge's phase is greater than the last advice phase.  A fork starts with its parent's setting; the cached opening
 * plans / query tables are made anew after a call.  The getter returns the number of phases (0 for a null object) and
 * copies the setting: advice_phase [n_advice], *n_challenges, challenge_phase [ZG_MAX_CHALLENGES]; each may be NULL.
 *
 * Inside the library challenge j is an instance-like column behind the caller's n_instance ones -- the constant
 * polynomial, filled by one kernel per phase (value row, coefficient row, coset slabs), never hashed, committed or opened
 * -- so every kernel reads it as it reads any column.  The arithmetic-level entries that take instance families over the
 * prover's circuit (zg_prover_evaluate_h*, zg_prover_lookup_compress_dev) therefore expect n_instance + challenges columns
 * from the caller, the challenges' constant columns last.  Each challenge costs a slot one value row, one coefficient row
 * and one slab per part of the extended domain.
 *
 * On a circuit with a challenge or a phase > 0: zg_prover_prove, _dev, _batch, _batch_dev work while every advice column
 * is in phase 0 (the witness cannot depend on a challenge then) and return ZG_ERR_INVALID_ARG otherwise (use
 * zg_prover_prove_phased); zg_prover_prove_multi*, zg_prover_prove_images*, zg_prover_check_batch, _batch_dev and _images
 * (a witness of such a circuit is checked by zg_prover_check_circuit*, with the caller's challenge values),
 * zg_verifier_verify_multi with more than one circuit and a point-range shard are ZG_ERR_UNSUPPORTED; the ZG_LAT_GATE
 * gate stays off.  One proof of several such circuits is made by zg_prover_prove_circuits* and verified by
 * zg_verifier_verify_circuits; a witness program with field operations and phases (zg_witness_plan_create_field) goes from
 * input bytes to such proofs through zg_prover_prove_inputs*, and to the check through zg_prover_check_inputs. */
int zg_prover_set_phases(zg_prover *p, const uint8_t *advice_phase, uint32_t n_challenges, const uint8_t *challenge_phase);
int zg_prover_phases(const zg_prover *p, uint8_t *advice_phase, uint32_t *n_challenges, uint8_t *challenge_phase);
/* create_proof's phase loop for a batch of `count` proofs whose witness is synthesised phase by phase.  The library
 * calls fn(user, phase, count, challenges, d_advice) once per phase, phase 0 included, before it commits that phase's
 * columns: challenges is [count][n_challenges] (Montgomery form, zero where not yet squeezed), d_advice[b] the device
 * address of proof b's slot, [n_advice][2^k] (zg_prover_advice_slot).  The callback writes the USABLE rows (the first
 * 2^k - blinding_factors - 1) of the columns of `phase` and nothing else: the blinding rows hold the proof's blinding
 * scalars already (the same rand_fr tag and index per column and row as every other entry draws), and the columns of
 * earlier phases are committed.  It orders its writes on zg_ctx_stream(ctx) or completes them before it returns.  A
 * non-zero return aborts the batch with ZG_ERR_INVALID_ARG, the queue drained.  The context's lock is held across the
 * callback: it must not call zg_prover_prove* on the same prover (or its context) from another thread and wait for it.
 * proofs[b] must hold zg_prover_proof_size(p) bytes.  A circuit without challenges, in one phase, gives zg_prover_prove's
 * bytes and launches. */
typedef int (*zg_phase_fn)(void *user, uint32_t phase, size_t count, const zg_fr *challenges, void *const *d_advice);
int zg_prover_prove_phased(zg_prover *p, size_t count, zg_phase_fn fn, void *user, const zg_fr *const *instance,
                           size_t instance_len, const uint8_t *rng_keys, uint8_t *const *proofs, size_t *proof_lens);
/* ... for ONE proof of `circuits` instances: zg_prover_prove_circuits with the witness synthesised phase by phase (the
 * contract stands at zg_prover_prove_circuits).  proof must hold zg_prover_proof_size_multi(p, circuits) bytes. */
int zg_prover_prove_circuits_phased(zg_prover *p, size_t circuits, zg_phase_fn fn, void *user, const zg_fr *const *instance,
                                    size_t instance_len, const uint8_t *rng_keys, uint8_t *proof, size_t proof_cap,
                                    size_t *proof_len);

/* Point-range shard of the commitments across `world` GPUs (one process and one prover per GPU):
 * this prover's base sets hold points [first_point, first_point + zg_bases_len) of ParamsKZG::g / ::g_lagrange, it
 * multiplies only that range of every scalar vector, and per commitment phase the ranks exchange their partial sums
 * -- `exchange` is an ALL-GATHER: `bytes` bytes of `send` from every rank, rank order, into recv[world * bytes]
 * (torch.distributed / RCCL on the caller's side; EC addition is not a reduction operator, so it is a gather plus
 * local additions, never an all-reduce).  Every rank runs the rest of create_proof (transforms, evaluate_h) itself and
 * ends with the same proof bytes. */
typedef int (*zg_exchange_fn)(void *user, const void *send, size_t bytes, void *recv);
/* Host helper, the additions behind that all-gather: parts = world x count partial sums in the MSM's extended
 * Jacobian form (X, Y, ZZ, ZZZ; 128 B each, as zg_msm_batch_dev leaves them), out[i] = normalised sum over the ranks. */
int zg_xyzz_sum_ranks(const void *parts, size_t world, size_t count, zg_g1 *out);
int zg_prover_set_shard(zg_prover *p, uint32_t rank, uint32_t world, size_t first_point, zg_exchange_fn exchange,
                        void *user);
/* The same shard with the exchange INSIDE the library: nccl_comm is an initialised RCCL communicator (ncclComm_t) of
 * `world` ranks whose rank order is the point-range order, one per prover (a communicator serialises its collectives
 * on one stream; forks do not inherit it).  Per commitment phase: ONE ncclAllGather of the phase's partial sums
 * (128 B each) over xGMI on the prover's stream, the world - 1 additions per commitment in a kernel behind it, and
 * only whole sums reach the host -- north_star's "single RCCL reduce of partial sums", spelt as gather + additions
 * because EC addition is no ncclRedOp.  librccl.so is bound with dlopen when this entry is first used. */
int zg_prover_set_shard_rccl(zg_prover *p, uint32_t rank, uint32_t world, size_t first_point, void *nccl_comm);
/* The additions of that path as an entry of their own (device pointers, on the context's stream, not normalised:
 * d_out[i] = sum over r of d_parts[r * count + i], both in the 128-byte extended Jacobian form). */
int zg_xyzz_sum_ranks_dev(zg_ctx *ctx, const void *d_parts, size_t world, size_t count, void *d_out);
/* Upper bound of the proof size in bytes for this circuit. */
size_t zg_prover_proof_size(const zg_prover *p);
/* Test hook: copies an intermediate of the LAST proof to the host.  what: 0 = h(X) on the extended
 * coset after the division by (X^n - 1) [2^ext_k], 1 = permutation z (index = set) [2^k Lagrange],
 * 2 = lookup z (index = lookup) [2^k Lagrange], 3 = permuted input a' (index = lookup),
 * 4 = permuted table s' (index = lookup), 5 = h pieces in coefficient form [5 * 2^k].  The pseudo-column of
 * challenge `index` (zg_prover_set_phases): 6 = its value row [2^k], 7 = its coefficient row [2^k], 8 = its slab on the
 * single extended coset [2^ext_k], 9 / 10 = its slabs on the first / second part of the split domain; the slabs in
 * plain Montgomery form, and only for the extended domain the last proof used (else ZG_ERR_INVALID_ARG).
 * 11 = shuffle z (index = shuffle) [2^k Lagrange].  12 / 13 = h on the first / second part of the split domain, as the
 * last proof left it there (plain Montgomery form; ZG_ERR_INVALID_ARG when that proof used the single coset, or took the
 * quotient's terms by degree, which reuses those buffers: zg_prover_set_quotient_terms(0) keeps them). */
int zg_prover_fetch(zg_prover *p, uint32_t what, uint32_t index, zg_fr *out, size_t cap_elems);
/* ... of proof `slot` of the last batch. */
int zg_prover_fetch_slot(zg_prover *p, size_t slot, uint32_t what, uint32_t index, zg_fr *out, size_t cap_elems);

/* Host wall-clock milliseconds the LAST proof spent per phase (diagnostics): 0 instance+advice
 * commitments, 1 lookup compression + permutation (of which out[7] is the host sort) + commitments,
 * 2 permutation/lookup products + random poly, 3 evaluate_h + h commitments, 4 evaluations,
 * 5 GWC openings, 6 total. */
int zg_prover_phase_ms(const zg_prover *p, double *out, size_t cap);
/* What the gate (ZG_LAT_GATE) did on this prover so far (diagnostics; upstream has no counterpart -- create_proof there
 * launches nothing ahead): out[0] proofs made in the gated order, out[1] gates armed, out[2] proofs re-made in the plain
 * order because a gate ran into its time limit or was let go, out[3] gates let go early by a blocking call. */
int zg_prover_gate_stats(const zg_prover *p, uint64_t *out, size_t cap);
/* The quotient's terms by degree.  On the split extended domain (zg_prover_set_overlap) only the terms of the highest
 * degrees need the second part's points: a term of degree d <= m1 + 1 contributes a quotient part of degree < m1 n, which
 * the first part (m1 n points) fixes alone.  The prover therefore evaluates only the high terms on the second part and
 * transforms only the witness polynomials they read onto it.  Proof bytes of a statement that holds do not depend on it
 * (for one that does not, see zg_prover_set_overlap: deterministic bytes that verify nowhere, in either setting).
 * enable = 0: every term on both parts (tests and A/B measurements); 1 (default): by degree, where the key has low terms. */
int zg_prover_set_quotient_terms(zg_prover *p, int enable);
/* ... and what the key's classification is: out = { active, G, S, L, C, G words: gate g is high, S words: permutation
 * set s's product term is high, L words: lookup l's product term is high, C words: coset slab c of a proof (advice,
 * instance, permutation z, lookup z, then a'_l and s'_l interleaved) is read by a high term and kept on the second part }.
 * active = 0: no split domain or no low term -- every term is evaluated everywhere.  *count = the words needed; out may be
 * NULL to ask for it. */
int zg_prover_quotient_terms(const zg_prover *p, uint32_t *out, size_t cap, size_t *count);

/* Scheduling of one proof on its GPU.  enable = 1 (default): the coefficient / coset transforms run on a
 * second HIP stream beside the commitment MSMs -- lowest latency for a lone proof.  enable = 0: one
 * stream per proof -- the throughput configuration when many provers share the GPU (other proofs fill
 * the gaps, and every extra stream costs a hardware queue); in this form the quotient is also computed on a
 * split extended domain (4n + n points instead of EvaluationDomain's 8n for a degree-6 circuit: the same
 * polynomial h from fewer evaluations) and the MSM reductions spend one lane per EC addition.  Proof bytes do
 * not depend on it. */
int zg_prover_set_overlap(zg_prover *p, int enable);
/* The multi-open argument a prover ends its proofs with.  ZG_MULTIOPEN_GWC (default): halo2's ProverGWC, one witness
 * commitment per distinct opening point.  ZG_MULTIOPEN_SHPLONK: ProverSHPLONK (halo2_proofs v2023_04_20
 * src/poly/kzg/multiopen/shplonk/; snark-verifier's Bdfg21): TWO commitments whatever the number of points, so a proof is
 * 64 * (point sets - 2) bytes shorter; everything up to and including the evaluations is the GWC proof's, byte for byte.
 * Order and equations: DESIGN.md section 16.  A property of the prover object, like zg_prover_set_overlap: it governs
 * zg_prover_prove, _dev, _batch, _batch_dev, _images, zg_prover_prove_multi, _multi_dev, _images_multi and the two
 * proof-size bounds; a fork starts with its parent's value.  The buffers SHPLONK needs, and its share of the pinned
 * staging range, are allocated HERE and resized by zg_prover_set_batch, never inside a proof: the first switch to SHPLONK
 * allocates the prover's slots anew, as zg_prover_set_batch does -- addresses from zg_prover_advice_slot and the slots'
 * contents do not survive it (ZG_ERR_OOM leaves the prover without slots and the setting unchanged).  Both scheduling forms make the same bytes; a SHPLONK prover makes its
 * proofs in the plain order -- the ZG_LAT_GATE gate does not arm, because the second commitment starts from the first
 * one's challenge.  On a point-range shard (zg_prover_set_shard*) a SHPLONK proof is refused with ZG_ERR_UNSUPPORTED.
 * More than 16 rotation sets or distinct opening points: ZG_ERR_UNSUPPORTED at the proof; an identity h1 or h2 is
 * refused as every identity commitment is.  Any other scheme value: ZG_ERR_INVALID_ARG, nothing changes. */
enum { ZG_MULTIOPEN_GWC = 0, ZG_MULTIOPEN_SHPLONK = 1 };
int zg_prover_set_multiopen(zg_prover *p, int scheme);
int zg_prover_multiopen(const zg_prover *p);
/* The transcript a prover writes its proofs into.  ZG_TRANSCRIPT_EVM (default): snark-verifier's EvmTranscript, Keccak-256,
 * a commitment as 64 uncompressed big-endian bytes.  ZG_TRANSCRIPT_BLAKE2B: halo2's own Blake2bWrite with Challenge255
 * (halo2_proofs v2023_04_20 src/transcript/blake2b.rs), a commitment as its 32-byte GroupEncoding (zg_g1_compress): a
 * proof is 32 bytes per commitment shorter.  As known from the published sources -- the crates were not at hand, and no
 * interoperability is claimed beyond this description; DESIGN.md section 17 lists what remains to be verified:
 *   hash state         BLAKE2b, 64-byte digest, no key, personalisation the 16 bytes "Halo2-Transcript"; never reset:
 *                      everything since init is one running hash
 *   common_scalar(s)   absorb the byte 0x02, then s.to_repr(): 32 bytes, little-endian, the canonical integer;
 *                      write_scalar also appends those 32 bytes to the proof
 *   common_point(P)    absorb 0x01, then x.to_repr() and y.to_repr(), 32 little-endian bytes each (the uncompressed
 *                      pair); the identity is refused
 *   write_point        appends the 32-byte compressed form P.to_bytes() to the proof
 *   squeeze_challenge  absorb 0x00, finalise a clone of the state, take the 64-byte digest as a little-endian integer and
 *                      reduce it modulo r (Challenge255::new, from_uniform_bytes); the live state keeps the 0x00 byte
 * The order of writes and squeezes does not depend on the transcript: it is the one documented for GWC and SHPLONK, for
 * one or several circuits.  A property of the prover object, like zg_prover_set_multiopen: it governs every prove entry
 * (zg_prover_prove, _dev, _batch, _batch_dev, _images, _multi, _multi_dev, _images_multi) and the two proof-size bounds,
 * which take 32 bytes per point under Blake2b; it combines with both multi-open schemes, both scheduling forms and
 * point-range shards (host state on every rank); a fork starts with its parent's value.  It allocates nothing on the
 * device.  With the default every byte and bound is what it was.  Any other value: ZG_ERR_INVALID_ARG, nothing changes. */
enum { ZG_TRANSCRIPT_EVM = 0, ZG_TRANSCRIPT_BLAKE2B = 1 };
int zg_prover_set_transcript(zg_prover *p, int transcript);
int zg_prover_transcript(const zg_prover *p);
/* Builds the digit tables (zg_bases_enable_digit_table) of the prover's three base sets -- ParamsKZG::g, ::g_lagrange and
 * the running sums of g_lagrange -- which a LONE proof (zg_prover_set_overlap(p, 1)) then uses instead of Pippenger buckets:
 * 2.9 -> 2.2 ms per create_proof at k = 14.  Footprint: 3 x ceil(255 / c) * 2^(c-1) * n * 64 B -- 78 GB at n = 2^14 (c = 11),
 * 84 GB at n = 2^15 (c = 10) -- and ~0.3 s of build time per table (0.8 s for the three at n = 2^14), which is why it is an
 * explicit call (round 3 built them inside the first latency-form proof, in 3.7 s).  max_bytes = what the three tables may take together; 0 = the library's cap (a third
 * of the card's memory, at most 90 GB) -- window bits shrink until they fit; nothing is built (not an error) when no width
 * fits, when n >= 2^16, when ZG_LAT_FULL_C = 0 or when the card has not that much free memory plus a reserve.
 * *bytes_built (may be NULL) = what is resident afterwards.  The tables belong to the base sets (shared by every prover on
 * them, freed with zg_bases_free); the throughput form never reads them.  Idempotent.  Proof bytes do not depend on it.
 * halo2 has no counterpart (ParamsKZG holds the bases only); the call site served is one synchronous proof,
 * /root/reference/src/wnn.rs:242-259. */
int zg_prover_enable_digit_tables(zg_prover *p, uint64_t max_bytes, uint64_t *bytes_built);

/* Stand-alone building blocks of the above. */
/* Evaluator::evaluate_h (halo2_proofs src/plonk/evaluation.rs) followed by the division by X^n - 1 of
 * vanishing::Argument::construct, for ONE circuit instance over this prover's resident proving key.  Inputs are the
 * coefficient forms upstream hands its evaluator -- advice_polys [n_advice][2^k], instance_polys [n_instance][2^k],
 * perm_z_polys [sets][2^k] (permutation::Committed product polys), lookup_z_polys [lookups][2^k] and permuted_polys
 * [2 * lookups][2^k] (a'_0, s'_0, a'_1, ...) -- and the challenges theta, beta, gamma, y; h_out receives h on
 * EvaluationDomain's extended coset (of the prover's generator, zg_prover_coset_generator), 2^ext_k values.  Host pointers (the arithmetic-level entry: ~60 MiB cross PCIe
 * at k = 14); slot 0 of the prover is used as scratch. */
int zg_prover_evaluate_h(zg_prover *p, const zg_fr *advice_polys, const zg_fr *instance_polys, const zg_fr *perm_z_polys,
                         const zg_fr *lookup_z_polys, const zg_fr *permuted_polys, const zg_fr *theta, const zg_fr *beta,
                         const zg_fr *gamma, const zg_fr *y, zg_fr *h_out);
/* The same (Evaluator::evaluate_h + the division by X^n - 1) with every polynomial family and d_h_out ([2^ext_k], library
 * form) as DEVICE pointers: the families are copied device-to-device into slot 0, nothing crosses PCIe but the four
 * challenges.  A family the circuit does not have may be NULL.  The call waits until those copies and the challenges have
 * arrived (work queued on the stream before it completes); the transforms, the evaluation and the write of d_h_out are
 * then asynchronous on the context stream. */
int zg_prover_evaluate_h_dev(zg_prover *p, const void *d_advice_polys, const void *d_instance_polys,
                             const void *d_perm_z_polys, const void *d_lookup_z_polys, const void *d_permuted_polys,
                             const zg_fr *theta, const zg_fr *beta, const zg_fr *gamma, const zg_fr *y, void *d_h_out);

/* ---- the arithmetic level on device pointers: the steps of create_proof between its MSMs
 * and transforms, for a caller that keeps halo2's own create_proof and holds its columns in HBM.  Columns are [count][2^k],
 * contiguous, zg_fr in Montgomery form.  Every entry holds the context lock and takes its scratch from the workspace pool.
 * The entries that take challenges (theta / beta / gamma) or report an error upload those scalars first, which waits for the
 * work queued on the stream before it; their kernels are then asynchronous on the context stream like every _dev entry. */

/* lookup::prover::Argument::commit_permuted's `compress_expressions` (halo2_proofs src/plonk/lookup/prover.rs) for lookup
 * `lookup` of the prover's circuit: row i of d_input / d_table ([2^k] each) is the theta-fold of the lookup's input / table
 * expressions at row i -- sum_e theta^(width-1-e) expr_e, the first expression entering as it is -- over the caller's
 * Lagrange columns d_advice [n_advice][2^k], d_instance [n_instance][2^k] (either may be NULL when the circuit has none) and
 * the prover's resident fixed columns.  A query with rotation t reads row (i + t) mod 2^k.  All 2^k rows are written.
 * lookup >= n_lookups is ZG_ERR_INVALID_ARG. */
int zg_prover_lookup_compress_dev(zg_prover *p, uint32_t lookup, const void *d_advice, const void *d_instance,
                                  const zg_fr *theta, void *d_input, void *d_table);
/* lookup::prover::permute_expression_pair on rows < usable of two [2^k] columns: d_permuted_input = a', the input sorted
 * by canonical value (Fr: Ord); d_permuted_table = s', which holds at the first row of every distinct a' value that same
 * value (one instance is taken out of the table multiset) and at the repeated rows the left-over table values, ascending
 * left-overs going to the repeated rows taken from the END (upstream pops a Vec of repeated rows).  Rows >= usable of both
 * outputs are written as ZERO: the caller puts its blinding there, as upstream does after the call.  The inputs are not
 * modified; an output may not alias an input.  4 <= k <= 20, else ZG_ERR_UNSUPPORTED (the range of the prover's own
 * path: its sort works on whole power-of-two columns and its scans on at most 2^20 rows); usable = 0 or usable > 2^k is
 * ZG_ERR_INVALID_ARG.  An input value that the table does not hold is ZG_ERR_CONSTRAINT (Error::ConstraintSystemFailure),
 * the outputs are then undefined: to report it this entry BLOCKS until the device has finished -- the one entry of this
 * group that does. */
int zg_permute_expression_pair_dev(zg_ctx *ctx, const void *d_input, const void *d_table, uint32_t k, uint32_t usable,
                                   void *d_permuted_input, void *d_permuted_table);
/* Host-pointer form of the same ([2^k] each); blocking. */
int zg_permute_expression_pair(zg_ctx *ctx, const zg_fr *input, const zg_fr *table, uint32_t k, uint32_t usable,
                               zg_fr *permuted_input, zg_fr *permuted_table);
/* lookup::prover::Permuted::commit_product's factors on all n rows: num[i] = (input[i] + beta)(table[i] + gamma),
 * den[i] = (a'[i] + beta)(s'[i] + gamma).  The running product itself is zg_grand_product_dev(num, den). */
int zg_lookup_product_terms_dev(zg_ctx *ctx, const void *d_input, const void *d_table, const void *d_permuted_input,
                                const void *d_permuted_table, const zg_fr *beta, const zg_fr *gamma, size_t n,
                                void *d_num, void *d_den);
/* permutation::Argument::commit (halo2_proofs src/plonk/permutation/prover.rs) works on the permutation columns in
 * chunks of cs_degree - 2: the number of those column sets, 0 for a circuit without permutation columns. */
uint32_t zg_prover_permutation_sets(const zg_prover *p);
/* permutation::prover::commit's factors of column set `set` on all 2^k rows:
 *   num[i] = prod_col (v_col[i] + beta * delta^col * omega^i + gamma),  den[i] = prod_col (v_col[i] + beta * sigma_col[i] + gamma)
 * over the columns col of the set (indices into zg_circuit.perm_columns; a last set that is not full holds fewer
 * factors), v_col the Lagrange column the entry names -- from d_advice [n_advice][2^k], d_instance [n_instance][2^k] or
 * the resident fixed columns -- and sigma_col from the resident key.  Chaining the sets is the caller's job, as it is
 * upstream's: z of set s starts from z0 = z of set s - 1 at row `usable` = 2^k - (blinding_factors + 1), passed to
 * zg_grand_product_dev.  set >= zg_prover_permutation_sets is ZG_ERR_INVALID_ARG. */
int zg_prover_permutation_terms_dev(zg_prover *p, uint32_t set, const void *d_advice, const void *d_instance,
                                    const zg_fr *beta, const zg_fr *gamma, void *d_num, void *d_den);
/* The linear combinations of polynomials create_proof makes outside its evaluator: vanishing::Argument::construct's
 * sum_i x^(n i) h_i (halo2_proofs src/plonk/vanishing/prover.rs) and ProverGWC::create_proof's sum_i v^i p_i - eval
 * (src/poly/kzg/multiopen/gwc/prover.rs):  d_out[i] = sum_j coeffs[j] * d_polys[j][i], i < n, and *sub0 (may be NULL) is
 * subtracted at i = 0.  d_polys and coeffs are HOST arrays of `count` entries; d_polys[j] is a device pointer to n
 * elements (the same one may occur several times).  count = 0 gives zero (minus *sub0).  d_out equal to an input pointer is
 * ZG_ERR_INVALID_ARG; n >= 2^28 is ZG_ERR_UNSUPPORTED.  Pointers and coefficients travel in the kernel arguments,
 * ZG_LINCOMB_CHUNK terms per launch (nothing is uploaded, nothing waits).  What is written is canonical. */
#define ZG_LINCOMB_CHUNK 64
int zg_fr_lincomb_dev(zg_ctx *ctx, const void *const *d_polys, const zg_fr *coeffs, size_t count, size_t n,
                      const zg_fr *sub0, void *d_out);
/* d_out[i] = rand_fr(key, tag, i), i < count < 2^32: the scalars create_proof draws from its RNG, as the prover level
 * draws them (above, "Randomness") -- vanishing::Argument::commit's random polynomial is tag 6, and a caller that wants
 * the prover level's bytes blinds with the other tags of DESIGN.md. */
int zg_fr_random_dev(zg_ctx *ctx, const uint8_t key[32], uint32_t tag, void *d_out, size_t count);

/* z[0] = z0, z[i+1] = z[i] * num[i] / den[i], i + 1 < n  (the running product of lookup::prover::commit_product and
 * permutation::prover::commit; a zero denominator gives ratio 0, as halo2's BatchInvert leaves zeros alone).
 * Host pointers / device pointers. */
int zg_grand_product(zg_ctx *ctx, const zg_fr *num, const zg_fr *den, const zg_fr *z0, size_t n, zg_fr *z);
int zg_grand_product_dev(zg_ctx *ctx, const void *d_num, const void *d_den, const zg_fr *z0, size_t n,
                         void *d_z);
/* eval_polynomial: out[j] = polys[j](points[j]) for `count` (poly, point) pairs; polys at
 * d_polys + poly_index[j]*stride_elems; points are host scalars; out is a host array. */
int zg_eval_polys_dev(zg_ctx *ctx, const void *d_polys, size_t stride_elems, size_t n,
                      const uint32_t *poly_index, const zg_fr *points, size_t count, zg_fr *out);
/* kate_division: d_q[0..n-1) = a(X) / (X - z). */
int zg_kate_division_dev(zg_ctx *ctx, const void *d_a, size_t n, const zg_fr *z, void *d_q);
/* Keccak-256 (EvmTranscript's hash), host. */
void zg_keccak256(const uint8_t *data, size_t len, uint8_t out[32]);

/* ---- witness of a batch of inputs on the device ------------------------------------------
 * Replaces, for a circuit whose layout does not depend on its input: the host pass upstream's create_proof makes
 * through Circuit::synthesize under its WitnessCollection (halo2_proofs v2023_04_20 src/plonk/prover.rs) -- for zero_g
 * WnnChip::predict, /root/reference/src/gadgets/wnn.rs:180-237, reached once per image from Wnn::proof,
 * /root/reference/src/wnn.rs:232-262.  The caller records that pass ONCE as a straight-line program over unsigned
 * 256-bit integers (one slot per operation; operands are earlier slots) and the library replays it per input:
 *
 *   op  0 CONST  consts[imm]        1 PIXEL  input byte imm     2 ADD a+b    3 SUB a-b     4 MUL a*b (low 256 bits)
 *       5 ADDI a+imm   6 RSUBI imm-a   7 MULI a*imm   8 SHRI a>>imm   9 SHLI a<<imm   10 ANDI a&imm   11 SHRV a>>b
 *       12 GTI a>imm   13 GEI a>=imm   14 EQI a==imm  (0 / 1)    15 DIVI a/imm    16 TABLE table[imm+a] (0 outside)
 *
 * Operations are given sorted by dependency level (level_start[l] .. level_start[l+1]); an operand must lie in an
 * earlier level (checked here, with every immediate: the program runs on the GPU unchecked).  cell_slot[c * 2^k + row]
 * names the slot advice column c shows in that row, or 0xFFFFFFFF for a cell left unassigned (zero); values are
 * reduced modulo r and written in the Montgomery form create_proof takes.  instance_slots: the public inputs. */
typedef struct zg_witness_plan zg_witness_plan;
typedef struct { uint64_t op, a, b, imm; } zg_witness_op;
int zg_witness_plan_create(zg_ctx* ctx, const zg_witness_op* ops, size_t n_ops, const uint32_t* level_start, size_t n_levels,
                           const uint64_t* consts /* [n_consts][4] little-endian words */, size_t n_consts,
                           const uint64_t* table, size_t n_table, const uint32_t* cell_slot /* [n_advice][2^k] */,
                           uint32_t n_advice, uint32_t k, const uint32_t* instance_slots, size_t n_instance,
                           size_t image_bytes, zg_witness_plan** out);
void zg_witness_plan_destroy(zg_witness_plan* plan);
size_t zg_witness_plan_image_bytes(const zg_witness_plan* plan);
size_t zg_witness_plan_instance_len(const zg_witness_plan* plan);
/* How the plan was laid out on the device (diagnostics; upstream has no counterpart -- its synthesis runs on the host):
 * out[0] bytes of LDS per workgroup (0: every operand in HBM, ZG_WITNESS_LDS = 0), out[1] / out[2] 8-byte / 32-byte LDS cells,
 * out[3] values that live in an LDS cell, out[4] consumed values left in HBM, out[5] levels whose barrier waits for HBM,
 * out[6] values whose interval bound exceeds 64 bits, out[7] levels, out[8] operations that run on 64-bit integers (operands
 * and result below 2^64 by their bounds), out[9] lanes of the workgroup. */
int zg_witness_plan_info(const zg_witness_plan* plan, uint64_t* out, size_t cap);
/* images: host, count * image_bytes; d_advice[i]: device, [n_advice][2^k] zg_fr (e.g. zg_prover_advice_slot);
 * instance_out: host, [count][n_instance].  At most 64 inputs per call.  Returns when the columns are written. */
int zg_witness_run_dev(zg_witness_plan* plan, const uint8_t* images, size_t count, void* const* d_advice, zg_fr* instance_out);
/* Wnn::proof for a batch (/root/reference/src/wnn.rs:232-262: image -> witness -> create_proof -> (proof bytes,
 * outputs)): the witness program into the prover's slots 0..count-1, then one lock-step batch of create_proofs with the
 * program's instance values as the single instance column.  outputs: host, [count][n_instance] (the class scores, as
 * field elements); everything else as zg_prover_prove_batch.  plan and prover must live on the same device. */
int zg_prover_prove_images(zg_prover* p, zg_witness_plan* plan, const uint8_t* images, size_t count, const uint8_t* rng_keys,
                           uint8_t* const* proofs, size_t proof_cap, size_t* proof_lens, zg_fr* outputs, int* statuses);
/* ... into ONE proof of `circuits` images (zg_prover_prove_multi: create_proof's `circuits` slice); outputs as above. */
int zg_prover_prove_images_multi(zg_prover* p, zg_witness_plan* plan, const uint8_t* images, size_t circuits,
                                 const uint8_t* rng_keys, uint8_t* proof, size_t proof_cap, size_t* proof_len, zg_fr* outputs);

/* ---- the witness program with field arithmetic, challenges and advice phases ---------------
 * What a circuit with challenges or advice phases otherwise synthesises through a zg_phase_fn on the host: a product
 * modulo r, an inverse, a running random linear combination, a shuffle's grand product.  Five more operations; with r
 * the BN254 scalar modulus, operands are slots holding ANY 256-bit integer and the result is the canonical
 * representative in [0, r) -- exactly (a mod r) * (b mod r) mod r and so on, as integers:
 *
 *   op  17 CHAL  challenge imm of this input, as its canonical integer      18 ADDM (a+b) mod r     19 SUBM (a-b) mod r
 *       20 MULM (a*b) mod r     21 INVM a^-1 mod r, and 0 when a = 0 (mod r): what Assigned::invert / evaluate yields
 *
 * Slots stay integers, so integer and field operations mix freely.  phase_level_start [n_phases + 1]: the levels of
 * phase ph are [phase_level_start[ph], phase_level_start[ph + 1]), contiguous from level 0, 1 <= n_phases <=
 * ZG_MAX_PHASES; a slot's phase is its level's.  advice_phase [n_advice], n_challenges <= ZG_MAX_CHALLENGES and
 * challenge_phase [n_challenges]: as zg_prover_set_phases takes them.  Checked here, before anything is uploaded, and
 * ZG_ERR_INVALID_ARG with a message beside zg_witness_plan_create's own refusals: an unknown opcode; CHAL with imm >=
 * n_challenges or in a phase <= challenge_phase[imm] (the value does not exist yet); a cell of column c showing a slot of
 * a phase > advice_phase[c]; an instance slot outside phase 0 (the instances are hashed before any challenge exists);
 * phase bounds that do not ascend or do not cover the levels; a phase >= n_phases in either phase array.
 *
 * A plan without a field operation, in one phase, is zg_witness_plan_create's: the same layout, the same kernels.  Any
 * other plan takes the field form: one launch per phase over that phase's levels, the slots of a batch in a buffer the
 * plan owns so that a later phase reads what an earlier one made.  The LDS allocation, its spill path and ZG_WITNESS_LDS
 * apply as they do to any plan, phase by phase: a field result counts as "may exceed 64 bits" (range [0, r - 1]), a value
 * holds its cell up to its last consumer of its own phase, and a slot of an earlier phase is an operand in HBM
 * (zg_witness_plan_info counts the levels that read one among those whose barrier waits for HBM).  One call at a time
 * per plan.
 * zg_witness_plan_create itself is unchanged and keeps refusing opcodes above 16. */
int zg_witness_plan_create_field(zg_ctx* ctx, const zg_witness_op* ops, size_t n_ops, const uint32_t* level_start, size_t n_levels,
                                 const uint64_t* consts, size_t n_consts, const uint64_t* table, size_t n_table,
                                 const uint32_t* cell_slot, uint32_t n_advice, uint32_t k, const uint32_t* instance_slots,
                                 size_t n_instance, size_t image_bytes, const uint32_t* phase_level_start, uint32_t n_phases,
                                 const uint8_t* advice_phase, uint32_t n_challenges, const uint8_t* challenge_phase,
                                 zg_witness_plan** out);
/* The whole witness, every phase, for GIVEN challenge values: zg_witness_run_dev's arguments and limits plus challenges,
 * host, [count][n_challenges], Montgomery form, the caller's values -- NULL if and only if the plan has none.  Whole
 * columns are written (unassigned cells zero).  zg_witness_run_dev takes a field-form plan too while it has no challenge. */
int zg_witness_run_field_dev(zg_witness_plan* plan, const uint8_t* inputs, size_t count, const zg_fr* challenges,
                             void* const* d_advice, zg_fr* instance_out);
/* input -> proof for EVERY circuit the library proves: the general form of zg_prover_prove_images.  Phase 0 of the
 * program goes into slots 0..count-1 and its instance values come out (outputs, [count][n_instance]); the proofs ride
 * on zg_prover_prove_batch_dev for a one-phase circuit and on zg_prover_prove_phased otherwise, with a phase callback of
 * the library's own that replays the plan's slice of each phase with the challenges it is handed and writes the usable
 * rows of that phase's columns.  Shuffles, both multi-open schemes, both transcripts, both scheduling forms and forks
 * work because the rides do.  Limits are zg_prover_prove_images': 64 inputs per call, count <= zg_prover_batch(p), plan and
 * prover on one device, the same k and column count, at most one instance column.  Besides, the plan's phases,
 * advice_phase, n_challenges and challenge_phase must EQUAL what zg_prover_phases(p) reports: ZG_ERR_INVALID_ARG
 * otherwise, nothing written, the prover usable.  With advice phases proof_cap must be at least zg_prover_proof_size(p)
 * (ZG_ERR_INVALID_ARG) and statuses[b] is ZG_OK for a proof that has bytes, the call's status (ZG_ERR_CONSTRAINT for a
 * failed lookup) for one that has none.  A point-range shard of a circuit with shuffles, challenges or phases:
 * ZG_ERR_UNSUPPORTED.  On a plan and circuit zg_prover_prove_images accepts: its bytes from its launches. */
int zg_prover_prove_inputs(zg_prover* p, zg_witness_plan* plan, const uint8_t* inputs, size_t count, const uint8_t* rng_keys,
                           uint8_t* const* proofs, size_t proof_cap, size_t* proof_lens, zg_fr* outputs, int* statuses);
/* ... into ONE proof of `circuits` inputs, on zg_prover_prove_circuits_dev / _phased: one squeeze per challenge, the same
 * value into every input's program.  proof must hold zg_prover_proof_size_multi(p, circuits) bytes. */
int zg_prover_prove_inputs_circuits(zg_prover* p, zg_witness_plan* plan, const uint8_t* inputs, size_t circuits,
                                    const uint8_t* rng_keys, uint8_t* proof, size_t proof_cap, size_t* proof_len, zg_fr* outputs);

/* ------------------------------------------------------------------ witness check
 * Replaces halo2_proofs::dev::MockProver::run followed by MockProver::verify / assert_satisfied (halo2_proofs
 * v2023_04_20 src/dev.rs), as Wnn::mock_proof calls them (/root/reference/src/wnn.rs:203-210), for a batch of
 * witnesses of the prover's circuit: is the witness satisfied, and if not, where does it fail.  With n = 2^k and
 * usable = n - (blinding_factors + 1):
 *   gates    gate polynomial g (index in zg_circuit.gates) fails on row r < usable iff its value there is not 0; a
 *            query with rotation t reads row (r + t) mod n of the column as it stands;
 *   lookups  lookup l fails on row r < usable iff the tuple of its input polynomials at r equals, component by
 *            component, the tuple of its table polynomials at NO row r' < usable (exact tuples, no compression);
 *   copies   with next(c, r) = (c', r') the cell for which sigma_c(omega^r) = delta^c' * omega^r' (c, c' index
 *            zg_circuit.perm_columns; halo2's permutation::keygen::Assembly::mapping), cell (c, r), r < n, fails iff
 *            its value differs from that of next(c, r).
 * MockProver's CellNotAssigned / ConstraintPoisoned diagnostics have no counterpart: the ABI carries values, not regions.
 * Per witness the check reports the exact number of failures of each kind and the first min(total, cap) failures in
 * ascending (kind, index, row) order. */
enum { ZG_FAIL_GATE = 0, ZG_FAIL_LOOKUP = 1, ZG_FAIL_COPY = 2, ZG_FAIL_SHUFFLE = 3 /* zg_prover_check_circuit* only */ };
typedef struct {
    uint32_t kind;        /* ZG_FAIL_*                                                         */
    uint32_t index;       /* gate / lookup / permutation-column / shuffle index                */
    uint32_t row;
    uint32_t other_index; /* ZG_FAIL_COPY: permutation column of next(c, r); else 0            */
    uint32_t other_row;   /* ZG_FAIL_COPY: its row; ZG_FAIL_SHUFFLE: the shuffle row met; else 0 */
} zg_failure;

/* count <= max_batch witnesses.  advice[b]: host [n_advice][2^k] (copied into slot b), or NULL = slot b as it stands;
 * instance[b]: [n_instance][instance_len], zero beyond.  failures: [count][cap] (may be NULL when cap == 0; entries past
 * a witness's total are left alone); totals: [count][3] by kind.  The check only READS the slot: it draws no blinding
 * rows and leaves every buffer a following proof reads as it found it (check, then zg_prover_prove_batch_dev on the
 * slot as it stands, gives the bytes proving alone gives).  A point-range shard can be checked: no bases are involved.
 * Returns the status of the CALL -- an unsatisfied witness is not an error of the call; ZG_ERR_INVALID_ARG also when a
 * sigma value of the proving key is no delta^c * omega^r (the mapping is recovered at the first check). */
int zg_prover_check_batch(zg_prover *p, size_t count, const zg_fr *const *advice, const zg_fr *const *instance,
                          size_t instance_len, zg_failure *failures, size_t cap, uint32_t *totals);
/* Same with the advice columns in HBM (as zg_prover_prove_batch_dev: copied into the slot unless they are the slot;
 * NULL entries, or d_advice NULL = the slots as they stand).  Blocking, like the host form. */
int zg_prover_check_batch_dev(zg_prover *p, size_t count, void *const *d_advice, const zg_fr *const *instance,
                              size_t instance_len, zg_failure *failures, size_t cap, uint32_t *totals);
/* Wnn::mock_proof for a batch of images (/root/reference/src/wnn.rs:203-210: image -> witness -> MockProver): the
 * witness program into the prover's slots 0..count-1, then the check with the program's instance values; outputs and
 * the plan's conditions as zg_prover_prove_images. */
int zg_prover_check_images(zg_prover *p, zg_witness_plan *plan, const uint8_t *images, size_t count, zg_fr *outputs,
                           zg_failure *failures, size_t cap, uint32_t *totals);
/* The witness check for a circuit with shuffles (zg_prover_create_shuffles) and challenges (ZG_CHALLENGE queries): what
 * zg_prover_check_batch* refuse.  Gates, lookups and copies as above, except that a ZG_CHALLENGE query evaluates to the
 * challenge value the caller passed for that witness.  A fourth kind, ZG_FAIL_SHUFFLE, modelled on MockProver::verify's
 * shuffle check (privacy-scaling-explorations/halo2 from v0.3.0 on, dev.rs): written from the published source, NOT
 * checked against it here (no upstream build is at hand).  For shuffle j of width m, in[r] the tuple of its m input
 * expressions at row r, sh[r] that of its m shuffle expressions, both for r < usable and as canonical integers (not
 * Montgomery limbs): the input rows are sorted ascending by (in[r], r), the shuffle rows by (sh[r], r) -- tuples compare
 * lexicographically, component 0 first; the row index is the last key, so both orders are total.  For each position
 * i < usable, with a the input row at i and b the shuffle row at i, input row a FAILS iff in[a] != sh[b]; the record is
 * {ZG_FAIL_SHUFFLE, j, a, 0, b}.  Rows >= usable take no part, whatever they hold; a query with rotation t reads row
 * (r + t) mod n of the column as it stands.  The comparison is exact (no theta, no gamma, no probability): a witness has
 * no shuffle failure iff the two multisets are equal, iff the argument's product closes for every gamma.  ONE spoiled cell
 * may report many rows, because the sorted sequences shift (MockProver's behaviour, kept); the totals are exact counts.
 * Reports stay in ascending (kind, index, row) order, shuffles last; a capped report is the head of the full one.
 *
 * totals: [count][4] by kind.  challenges: [count][n_challenges], Montgomery form, n_challenges as zg_prover_phases
 * reports it (the circuit's own count, 1 + the largest index a ZG_CHALLENGE query names, while zg_prover_set_phases was
 * never called).  The values are the CALLER's and any values are accepted: the library does not derive MockProver's own
 * challenge values (that derivation cannot be checked against upstream here).  NULL only when the circuit has no
 * challenge, ZG_ERR_INVALID_ARG otherwise.  The witness is WHOLE: the columns of every phase are in the slot or in
 * advice[b], synthesised by the caller for those challenge values; the check runs no callback.  Everything else --
 * advice, instance, failures, cap, the slots only read, blocking, the status of the call, a point-range shard -- as
 * zg_prover_check_batch / _dev.  On a circuit without shuffles and challenges the report is zg_prover_check_batch's with
 * a fourth total of 0, from the same launches. */
int zg_prover_check_circuit(zg_prover *p, size_t count, const zg_fr *const *advice, const zg_fr *const *instance,
                            size_t instance_len, const zg_fr *challenges, zg_failure *failures, size_t cap, uint32_t *totals);
int zg_prover_check_circuit_dev(zg_prover *p, size_t count, void *const *d_advice, const zg_fr *const *instance,
                                size_t instance_len, const zg_fr *challenges, zg_failure *failures, size_t cap, uint32_t *totals);
/* input -> check for every circuit the library proves: zg_witness_run_field_dev for the caller's challenge values into
 * slots 0..count-1, then zg_prover_check_circuit_dev on the slots with the program's instance values.  totals:
 * [count][4]; challenges: [count][n_challenges], Montgomery form, NULL if and only if the circuit has none; outputs and
 * the plan's conditions as zg_prover_prove_inputs. */
int zg_prover_check_inputs(zg_prover *p, zg_witness_plan *plan, const uint8_t *inputs, size_t count, const zg_fr *challenges,
                           zg_fr *outputs, zg_failure *failures, size_t cap, uint32_t *totals);
/* Host helper (no device): next_col / next_row [n_perm][2^k] such that sigma_values[c][r] = delta^next_col *
 * omega^next_row -- Assembly::mapping back from what halo2's ProvingKey holds (pk.permutation.permutations).
 * ZG_ERR_INVALID_ARG when a value is no such product. */
int zg_permutation_mapping(uint32_t k, uint32_t n_perm, const zg_fr *sigma_values, uint32_t *next_col,
                           uint32_t *next_row);
/* The other direction, on the device: permutation::keygen::Assembly::build_pk's values (halo2_proofs
 * src/plonk/permutation/keygen.rs), sigma_out[c][r] = delta^next_col[c][r] * omega^next_row[c][r] -- the exact inverse of
 * zg_permutation_mapping, same [n_perm][2^k] layout, host pointers.  ZG_ERR_INVALID_ARG when a column index is >= n_perm
 * or a row index >= 2^k.  The order-dependent merging of cycles (Assembly::copy) stays with the caller. */
int zg_permutation_sigma(zg_ctx *ctx, uint32_t k, uint32_t n_perm, const uint32_t *next_col, const uint32_t *next_row,
                         zg_fr *sigma_out);

/* ------------------------------------------------------------------ verifier
 * Replaces halo2_proofs::plonk::verify_proof::<KZGCommitmentScheme<Bn256>, VerifierGWC, _, EvmTranscript,
 * AccumulatorStrategy> followed by `DualMSM::check` (halo2_proofs v2023_04_20 src/plonk/verifier.rs,
 * src/poly/kzg/multiopen/gwc/verifier.rs, src/poly/kzg/strategy.rs), as Wnn::verify_proof calls it
 * (/root/reference/src/wnn.rs:265-280), for a batch of proofs of one circuit.  The proofs' transcripts are replayed
 * and their opening terms multiplied out on the device; a random linear combination reduces the batch to one
 * two-pairing check on the host (DESIGN.md section "Verification"). */
typedef struct zg_verifier zg_verifier;

/* keygen_vk's commitments (halo2_proofs src/plonk/keygen.rs: params.commit_lagrange of each fixed column and each
 * permutation polynomial), with the prover's g_lagrange bases: fixed_out[n_fixed], sigma_out[n_perm_columns], affine,
 * an all-zero column giving (0,0).  A point-range shard (world > 1) holds only part of the bases: ZG_ERR_UNSUPPORTED. */
int zg_prover_vk_commitments(const zg_prover *p, zg_g1_affine *fixed_out, zg_g1_affine *sigma_out);
/* The verifying key on the device: the circuit (its polynomials, queries and opening point sets), the fixed and
 * sigma commitments, and ParamsVerifierKZG's g0 = g[0], g2 and s_g2.  The secret scalar is never needed.  vk_repr:
 * vk.transcript_repr, hashed into every transcript first.  All host pointers, copied. */
int zg_verifier_create(zg_ctx *ctx, const zg_circuit *circuit, const zg_g1_affine *fixed_commitments,
                       const zg_g1_affine *sigma_commitments, const zg_g1_affine *g0, const zg_g2_affine *g2,
                       const zg_g2_affine *s_g2, const zg_fr *vk_repr, zg_verifier **out);
/* ... for a circuit with shuffle arguments (zg_prover_create_shuffles; n_shuffles = 0: the same call): the walk reads the
 * shuffle products behind the lookup products and their evaluations behind the lookups', the expected h(x) takes the
 * three terms per shuffle behind the lookup terms and the opening check the two queries per shuffle.  The shuffles are
 * validated as zg_prover_create_shuffles validates them, circuit->cs_degree included.  zg_verifier_verify_multi
 * of several circuits answers ZG_ERR_UNSUPPORTED for such a verifier; zg_verifier_verify_circuits verifies such proofs. */
int zg_verifier_create_shuffles(zg_ctx *ctx, const zg_circuit *circuit, const zg_shuffle *shuffles, uint32_t n_shuffles,
                                const zg_g1_affine *fixed_commitments, const zg_g1_affine *sigma_commitments,
                                const zg_g1_affine *g0, const zg_g2_affine *g2, const zg_g2_affine *s_g2, const zg_fr *vk_repr,
                                zg_verifier **out);
void zg_verifier_destroy(zg_verifier *v);
/* Verifies `count` proofs (EvmTranscript bytes proofs[b], proof_lens[b] long) against their public inputs
 * instance[b] ([n_instance][instance_len], as zg_prover_prove_batch takes them).  verdicts[b]: 1 = accepted; 0 = the
 * opening equation fails or bytes follow the proof; negative = malformed (short, a coordinate or scalar not below
 * its modulus, a point off the curve or at infinity).  Each verdict is the one a lone verification would give.
 * Proof b's share of the batch equation is weighted by r_b = rand_fr(key, TAG_VERIFY_BATCH, b) (the ChaCha20
 * scalar of the prover's blinding).  `key` MUST come from the caller's CSPRNG: a prover who knows it can choose
 * bad proofs whose errors cancel in the weighted sum.  Returns the zg_status of the call itself. */
int zg_verifier_verify_batch(zg_verifier *v, size_t count, const uint8_t *const *proofs, const size_t *proof_lens,
                             const zg_fr *const *instance, size_t instance_len, const uint8_t key[32], int *verdicts);
/* The same for proofs of `circuits` instances each (zg_prover_prove_multi; verify_proof's `instances: &[&[&[F]]]`):
 * instance[b * circuits + c] = the instance columns of circuit c of proof b.  Verdict classes, weights and bisection are
 * zg_verifier_verify_batch's; circuits = 1 IS that call.  The query tables are built per `circuits` at first use and kept. */
int zg_verifier_verify_multi(zg_verifier *v, size_t count, size_t circuits, const uint8_t *const *proofs,
                             const size_t *proof_lens, const zg_fr *const *instance, size_t instance_len,
                             const uint8_t key[32], int *verdicts);
/* zg_verifier_verify_multi for the proofs of zg_prover_prove_circuits*: the same arguments, verdict classes, weights and
 * bisection, for every circuit the verifier was created for -- shuffle arguments, challenges and advice phases included
 * (zg_verifier_create_shuffles, zg_verifier_set_phases; the proof's order: zg_prover_prove_circuits).  On a circuit without
 * them it IS zg_verifier_verify_multi; circuits = 1 is zg_verifier_verify_batch. */
int zg_verifier_verify_circuits(zg_verifier *v, size_t count, size_t circuits, const uint8_t *const *proofs,
                                const size_t *proof_lens, const zg_fr *const *instance, size_t instance_len,
                                const uint8_t key[32], int *verdicts);
/* Which multi-open argument the proofs handed to zg_verifier_verify_batch / _multi end with (ZG_MULTIOPEN_*, default GWC;
 * VerifierSHPLONK: DESIGN.md section 16).  Verdict classes are the same: a point of the tail that is off the curve, at
 * infinity or not canonical gives a negative verdict, trailing bytes or a failing equation 0.  Query tables are built per
 * (scheme, circuits) at first use and kept.  More than 16 rotation sets or opening points: ZG_ERR_UNSUPPORTED from the
 * verification call.  Any other value: ZG_ERR_INVALID_ARG, nothing changes. */
int zg_verifier_set_multiopen(zg_verifier *v, int scheme);
int zg_verifier_multiopen(const zg_verifier *v);
/* Which transcript the proofs handed to zg_verifier_verify_batch / _multi were written into (ZG_TRANSCRIPT_*, default EVM;
 * the format: zg_prover_set_transcript).  Under ZG_TRANSCRIPT_BLAKE2B a proof is a fixed layout of 32-byte items, so a
 * short proof is malformed before anything is read; every commitment is decompressed by the kernel of zg_g1_decompress
 * (one lane per point) ahead of the replay, which absorbs and squeezes with BLAKE2b on the device.  Verdict classes stay:
 * negative = short, an x not below q (bit 6 included), an x with no point, the identity encoding, a scalar not below r;
 * 0 = a failing equation or trailing bytes; malformed wins over trailing; each verdict is the one a lone verification
 * gives.  Query and offset tables are kept per (transcript, scheme, circuits).  Any other value: ZG_ERR_INVALID_ARG,
 * nothing changes. */
int zg_verifier_set_transcript(zg_verifier *v, int transcript);
int zg_verifier_transcript(const zg_verifier *v);
/* The phases of the proofs handed to zg_verifier_verify_batch: zg_prover_set_phases' arguments, defaults, conditions and
 * getter.  The transcript walk reads each phase's advice commitments, then squeezes that phase's challenges, and the
 * expected h(x) takes a ZG_CHALLENGE query from them.  A verifier without the call reads every advice commitment before
 * the challenges, so it rejects a proof made in several phases.  zg_verifier_verify_multi with more than one circuit is
 * ZG_ERR_UNSUPPORTED for a circuit with a challenge or a phase > 0; zg_verifier_verify_circuits verifies such proofs. */
int zg_verifier_set_phases(zg_verifier *v, const uint8_t *advice_phase, uint32_t n_challenges, const uint8_t *challenge_phase);
int zg_verifier_phases(const zg_verifier *v, uint8_t *advice_phase, uint32_t *n_challenges, uint8_t *challenge_phase);
/* Host helper (no device): *result = 1 iff prod_i e(p[i], q[i]) = 1 in GT (BN254 optimal ate pairing); identity
 * points contribute 1.  The points are taken to be in G1 and G2.  bn256::multi_miller_loop + final_exponentiation. */
int zg_pairing_check(const zg_g1_affine *p, const zg_g2_affine *q, size_t n, int *result);

/* ------------------------------------------------------------------ WNN model (cleartext inference)
 * Replaces Wnn::predict (/root/reference/src/wnn.rs:78-173: thermometer_encoding, mish_mash_hash, encode_image,
 * bloom_filter_lookup, predict) for a batch of images, and the loop of the CLI's compute-accuracy
 * (/root/reference/src/main.rs:186-213) with its argmax (/root/reference/src/utils.rs:35-45): the cleartext model whose
 * inference every proof is about.  The object is built from the fields of `Wnn` (wnn.rs:52-76) as io.rs's load_wnn leaves
 * them; no recorded program is involved.  Integer arithmetic: every output is the reference's, bit for bit.
 *   filters       = (width * height * bits_per_input) / num_filter_inputs, floor (chunks_exact drops a partial chunk)
 *   bit[b*W*H + i*H + j] = image[i*H + j] >= thresholds[(i*H + j) * bits_per_input + b]   (16-bit comparison: a threshold of
 *                   0 is always met, one of 256 never)
 *   filter f's index x = permuted bits f*n .. f*n + n - 1, the first one bit 0, where permuted bit t = bit[input_permutation[t]]
 *                   (any in-range map, not only permutations)
 *   h             = (x * x * x mod p) mod entries^hashes as exact integers; index i = (h / entries^i) mod entries
 *   score[c]      = the number of filters f with bloom_filters[c][f][index i] non-zero for every i < hashes
 * zg_wnn_create checks everything on the host before anything is uploaded: a null pointer, a zero dimension / entries /
 * hashes / p, num_filter_inputs outside 1..64, filters = 0, a permutation entry >= the bit count or a threshold > 256 are
 * ZG_ERR_INVALID_ARG; num_classes > 64, images of more than 16384 pixels, 2^31 input bits or a table of 2^32 (filter, entry) pairs and beyond
 * are ZG_ERR_UNSUPPORTED.
 * Resident size: filters * entries words of 4 bytes (8 beyond 32 classes) + filters * num_filter_inputs * 4 bytes
 * (DESIGN.md section 12).  The model lives on its context and must be destroyed before it. */
typedef struct zg_wnn zg_wnn;
int zg_wnn_create(zg_ctx *ctx, uint32_t num_classes, uint32_t width, uint32_t height, uint32_t bits_per_input,
                  uint32_t num_filter_inputs, uint32_t num_filter_entries, uint32_t num_filter_hashes, uint64_t p,
                  const uint8_t *bloom_filters,        /* [classes][filters][entries], 0 / non-zero (Array3<bool>) */
                  const uint64_t *input_permutation,   /* [width*height*bits_per_input]                              */
                  const uint16_t *thresholds,          /* [width][height][bits_per_input], 0..256                    */
                  zg_wnn **out);
void zg_wnn_destroy(zg_wnn *m);
/* images: [count][width*height] bytes; scores: [count][num_classes].  count = 0 is ZG_OK and launches nothing.  The host
 * form returns when the scores are written; the _dev form takes device pointers and is asynchronous on the context stream. */
int zg_wnn_predict(zg_wnn *m, const uint8_t *images, size_t count, uint64_t *scores);
int zg_wnn_predict_dev(zg_wnn *m, const void *d_images, size_t count, void *d_scores);
/* compute-accuracy: prediction = argmax of utils.rs (the first index of the strict maximum; class 0 when every score is
 * 0), *correct = how many predictions equal their label, confusion[label * num_classes + prediction] counts the pairs.
 * predictions ([count]) and confusion ([classes][classes]) may be NULL.  A label >= num_classes is ZG_ERR_INVALID_ARG
 * (checked before any launch).  Host pointers, blocking. */
int zg_wnn_accuracy(zg_wnn *m, const uint8_t *images, const uint32_t *labels, size_t count,
                    uint32_t *predictions /* [count] or NULL */, uint64_t *correct,
                    uint64_t *confusion   /* [classes][classes] (label, prediction) or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ZG_HALO2_H */
