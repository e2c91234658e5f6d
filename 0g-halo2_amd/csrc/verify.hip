// Batched GWC verification on the device -- replaces halo2_proofs::plonk::verify_proof::<KZGCommitmentScheme<Bn256>,
// VerifierGWC, _, EvmTranscript, AccumulatorStrategy> + DualMSM::check (halo2_proofs v2023_04_20 src/plonk/verifier.rs,
// src/poly/kzg/multiopen/gwc/verifier.rs, src/poly/kzg/strategy.rs) for many proofs of one circuit, each of NC >= 1
// instances of it (verify_proof's `instances: &[&[&[F]]]`; NC = 1: zg_verifier_verify_batch).  A proof of NC instances
// holds the per-circuit commitments and evaluations NC times, circuit-major within each family, and once what the
// circuits share: the random polynomial, h, the fixed and sigma evaluations, one W per point set.
// That order -- families, evaluations, opening queries, point sets, SHPLONK's rotation sets, lengths -- is stated in
// proof_layout.h, for the prover too; set_circuits() maps it to term indices and device tables and derives none of it.
//
// Per proof b the GWC equation is  e(L_b, [s]_2) = e(R_b, [1]_2)  with  L_b = sum_j u^j W_j  and
// R_b = sum_j u^j (z_j W_j + sum_k v^(m_j-1-k) C_jk - e_j G),  j over the opening point sets in first-appearance order,
// k over a set's queries in query order.  Four launches and one host step:
//   verify_replay   one wave per proof: the transcript read back in ONE walk (replay_one) over a format policy, every
//                   point and scalar validated as it is read, the challenges theta, beta, gamma, y, x, v, u squeezed.
//                   KeccakWalk: EvmTranscript, the sponge of keccak.h.  Blake2bWalk (zg_verifier_set_transcript(
//                   ZG_TRANSCRIPT_BLAKE2B)): g1_decompress_kernel of g1_compress.hip first -- one
//                   lane per commitment of the batch, y from x -- then the walk over the decompressed points with
//                   BLAKE2b and little-endian scalars.  No hash code lives in this file.
//   verify_scalars  one wave per proof: x^n, l_0 / l_last / l_blind and the instance evaluations (Lagrange form,
//                   O(instance_len) per query) with one batched inversion, the expected h(x) from the gates, the
//                   permutation and the lookups folded with y, then every term's scalar of L_b and R_b;
//   verify_terms    one workgroup per proof, one lane per term (double-and-add), a tree sum to the pair (L_b, R_b),
//                   then the weighted pair r_b (L_b, R_b), kept for the failure path;
//   verify_fold     one workgroup: L = sum_b r_b L_b, R = sum_b r_b R_b;
//   host            e(L, [s]_2) e(-R, [1]_2) = 1 (pairing.hip), outside the context lock; if it fails, the batch is
//                   bisected over the weighted pairs down to the proofs that fail alone.
#include <array>
#include <cstring>
#include <map>

#include "blake2b.h"
#include "keccak.h"
#include "poly.h"
#include "proof_layout.h"

namespace zg {

bool pairing_product_is_one(const Affine* p, const zg_g2_affine* q, size_t n);
int g1_decompress_dev(zg_ctx* ctx, const uint8_t* d_in, size_t n, Affine* d_out, uint8_t* d_valid);

namespace {

constexpr uint32_t SHARED = 0x80000000u;  // query table: commitment shared by all proofs (fixed, sigma)
constexpr uint32_t HREF = 0x7fffffffu;    // query table: the h commitment sum_i xn^i H_i
constexpr uint32_t IEVAL = 0x80000000u;   // evaluation source: an instance evaluation slot (of the circuit at hand)
constexpr uint32_t FIXEV = 0x40000000u;   // evaluation source: a fixed-query evaluation (shared); else: an advice query's, per circuit
constexpr uint32_t CHALEV = 0x20000000u;  // evaluation source: a challenge of the proof's scalar record (Expression::Challenge)

struct alignas(16) VMono {
    Fe coeff;
    uint32_t n_factors;
    uint32_t factors[ZG_MAX_FACTORS];
    uint32_t pad[3];
};

struct VQuery {
    uint32_t term;  // term index of the commitment, SHARED | index, or HREF
    uint32_t eval;  // index into the proof's evaluations
    uint32_t set;   // opening point set (SHPLONK: rotation set i)
    uint32_t vpow;  // power of v within the set (SHPLONK: j, the commitment's place in its set = its power of y)
    uint32_t pt;    // SHPLONK: the query's (set, point) pair in VArgs::f_pt; FIRST_PT: the commitment's first query
};
constexpr uint32_t FIRST_PT = 0x80000000u;

// (CH_SY: SHPLONK's y, squeezed where GWC squeezes v; CH_CHAL + j: the circuit's challenge j, squeezed behind its phase's advice commitments)
enum { CH_THETA, CH_BETA, CH_GAMMA, CH_Y, CH_X, CH_V, CH_U, CH_SY, CH_CHAL, CH_N = CH_CHAL + ZG_MAX_CHALLENGES };
enum { ST_OK = 1, ST_TRAILING = 0, ST_MALFORMED = -1 };

struct VArgs {
    // circuit
    const VMono* monos;
    const zg_poly* gates;
    const zg_lookup* lookups;
    const zg_shuffle* shuffles;  // NS of them (zg_verifier_create_shuffles)
    const uint32_t* qsrc;   // per circuit query: evaluation index, or IEVAL | instance slot
    const uint32_t* psrc;   // per permutation column: the same, at rotation 0
    const uint32_t* iev_col;
    const Fe* iev_wr;       // omega^rotation of instance slot e
    const VQuery* oq;       // opening queries in order
    const Fe* set_wr;       // omega^rotation of point set j
    const Fe* lag_w;        // omega^r, r = -(bf + 1) .. 0
    const Affine* shared;   // fixed, sigma commitments, g0
    uint32_t n_gates, n_lookups, n_queries, n_iev, n_oq;
    uint32_t A, F, I, P, NL, sets, chunk, qpd, bf, nsets, nAQ, nFQ;
    uint32_t NE, NP, NT, ev_h;  // evaluations (with the expected h(x) last), per-proof points, terms
    // the multi-open argument: nW points end a proof (GWC: one W per point set; SHPLONK: h1, h2), the last nL of them are
    // the left side's terms (every W; h2).  SHPLONK: nS rotation sets over the nT points of T;
    // set i holds the points f_pt[s_first[i] .. s_first[i + 1]) (indices into T, nF pairs in all) and s_mask[i] says
    // which points of T are its own; T is GWC's point sets, so set_wr[t] = omega^rotation of point t
    uint32_t scheme, nW, nL, nS, nT, nF, nwork;
    const uint32_t* s_first;
    const uint32_t* s_mask;
    const uint32_t* f_pt;
    // proofs of NC circuit instances, from proof_layout.h (set_circuits): the points the walk reads between two squeezes,
    // where the random polynomial's commitment stands among a proof's points, and where the families start among its
    // evaluations (circuit c's share follows circuit c-1's: nAQ advice, npz permutation, 5 NL lookup evaluations each)
    uint32_t NC, walk[4], PT_RAND, EV_FIX, EV_SIG, EV_PZ, EV_LK, npz;
    uint32_t NS, EV_SH;  // the shuffles: circuit c's 2 NS evaluations (z, z(wx) per shuffle) follow circuit c-1's from EV_SH on
    // the advice phases (the layout's): walk[0] is read as ph_points[ph] points per phase, each followed by the squeezes of
    // that phase's ph_nchal[ph] challenges, whose indices stand one phase behind the other in ph_chal
    uint32_t n_ph, ph_points[ZG_MAX_PHASES], ph_nchal[ZG_MAX_PHASES], ph_chal[ZG_MAX_CHALLENGES];
    uint32_t log_n;
    Fe omega, ifft_div, delta, vk_repr;
    // batch
    const uint8_t* bytes;
    const uint64_t* off;
    const uint64_t* len;
    const Fe* inst;  // [count][NC][I][ilen]
    uint32_t ilen, count;
    Affine* pts;     // [count][NP]
    // Blake2b transcript: the proofs' commitments gathered for g1_decompress_kernel, its flags, and the length of a proof
    uint8_t* enc;    // [count][NP][32]
    uint8_t* pvalid; // [count][NP]
    uint64_t b2_len;
    Fe* ev;          // [count][NE]
    Fe* ch;          // [count][CH_N]
    int* status;     // [count]
    Fe* qe;          // [count][n_queries + n_iev]: the circuit at hand's
    Fe* tmp;         // [count][2 * ninv]
    uint32_t ninv;
    Fe* sc;          // [count][NT], canonical integers
    const Fe* rb;    // [count], canonical integers
    XYZZ* wpair;     // [count][2]: r_b L_b, r_b R_b
    XYZZ* out;       // [2]
};

template <class P>
__host__ __device__ bool below_modulus(const Fe& v) {
    for (int i = 7; i >= 0; i--) {
        if (v.l[i] < P::p(i)) return true;
        if (v.l[i] > P::p(i)) return false;
    }
    return false;
}
__host__ __device__ Fe be_int(const uint8_t* b) {
    Fe v;
    for (int i = 0; i < 8; i++)
        v.l[i] = (uint32_t)b[31 - 4 * i] | ((uint32_t)b[30 - 4 * i] << 8) | ((uint32_t)b[29 - 4 * i] << 16) |
                 ((uint32_t)b[28 - 4 * i] << 24);
    return v;
}

// A proof as the transcript walk sees it: its bytes, where its points go and -- Blake2b -- whether g1_decompress_kernel
// found them valid.  The pointers live here and not in the policies below: next to a hash state, which is indexed
// dynamically and so kept in scratch, a pointer comes back without its address space and every byte of the proof is
// read with a flat load (measured: the Keccak walk of a tiny-model proof 1.62 ms instead of 1.43).
struct ProofIn {
    const uint8_t* bytes;
    uint64_t len;
    Affine* pts;
    const uint8_t* valid;
};
// What the walk asks of a transcript format: begin (false: the proof cannot be read at all), absorb a common scalar,
// read and absorb the proof's next point into / from pts[i], read and absorb its next scalar, squeeze, and whether the
// proof ended where the walk did.
// EvmTranscript (keccak.h): 64-byte big-endian points, each coordinate below q, on the curve and not the identity (the
// transcript refuses it); 32-byte big-endian scalars below r.
struct KeccakWalk {
    Sponge s;
    uint64_t pos;
    __host__ __device__ bool begin(const ProofIn&, uint64_t) {
        sp_reset(s);
        pos = 0;
        return true;
    }
    __host__ __device__ void common_scalar(const Fe& raw) { sp_int(s, raw); }
    __host__ __device__ bool point(const ProofIn& in, uint32_t i) {
        if (pos + 64 > in.len) return false;
        const uint8_t* b = in.bytes + pos;
        pos += 64;
        const Fe x = be_int(b), y = be_int(b + 32);
        if (!below_modulus<FqParams>(x) || !below_modulus<FqParams>(y)) return false;
        Affine& out = in.pts[i];
        out.x = Fq::from_raw(x);
        out.y = Fq::from_raw(y);
        if (affine_is_identity(out) || !affine_on_curve(out)) return false;
        for (int k = 0; k < 64; k++) sp_byte(s, b[k]);
        return true;
    }
    __host__ __device__ bool scalar(const ProofIn& in, Fe& out) {
        if (pos + 32 > in.len) return false;
        const uint8_t* b = in.bytes + pos;
        pos += 32;
        const Fe v = be_int(b);
        if (!below_modulus<FrParams>(v)) return false;
        out = Fr::from_raw(v);
        for (int k = 0; k < 32; k++) sp_byte(s, b[k]);
        return true;
    }
    __host__ __device__ Fe squeeze() { return sp_squeeze(s); }
    __host__ __device__ bool at_end(const ProofIn& in) const { return pos == in.len; }
};
// halo2's Blake2b transcript (blake2b.h; the format: include/zg_halo2.h, zg_prover_set_transcript).  A proof is a fixed
// layout of 32-byte items, `fixed_len` bytes, so a short one is malformed before anything is read; the commitments are in
// pts already, decompressed by g1_decompress_kernel with their flags (an invalid encoding and the identity are refused
// here, where the transcript would refuse them); scalars are little-endian canonical integers below r.
struct Blake2bWalk {
    Blake2b s;
    uint64_t pos, fixed_len;
    __host__ __device__ bool begin(const ProofIn& in, uint64_t fixed_len_) {
        if (in.len < fixed_len_) return false;
        b2_init_halo2(s);
        pos = 0;
        fixed_len = fixed_len_;
        return true;
    }
    __host__ __device__ void common_scalar(const Fe& raw) {
        b2_byte(s, 2);
        b2_int(s, raw);
    }
    __host__ __device__ bool point(const ProofIn& in, uint32_t i) {
        pos += 32;
        if (!in.valid[i] || affine_is_identity(in.pts[i])) return false;
        b2_byte(s, 1);
        b2_int(s, Fq::to_raw(in.pts[i].x));
        b2_int(s, Fq::to_raw(in.pts[i].y));
        return true;
    }
    __host__ __device__ bool scalar(const ProofIn& in, Fe& out) {
        const uint8_t* b = in.bytes + pos;
        Fe v;
        for (int i = 0; i < 8; i++)
            v.l[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
        pos += 32;
        if (!below_modulus<FrParams>(v)) return false;
        out = Fr::from_raw(v);
        common_scalar(v);
        return true;
    }
    __host__ __device__ Fe squeeze() { return b2_squeeze(s); }
    __host__ __device__ bool at_end(const ProofIn& in) const { return fixed_len == in.len; }
};

// The walk, in the order of proof_layout.h's families: the vk and the instances | walk[0] points (advice), phase by phase
// with the phase's challenges squeezed behind each | theta | walk[1]
// (permuted) | beta, gamma | walk[2] (permutation z, lookup z, random) | y | walk[3] (h pieces) | x | the evaluations |
// GWC: v, one W per point set, u; SHPLONK: y, v, h1, u, h2.  Points land in pts in that order, evaluations in ev.
template <class Walk>
__host__ __device__ void replay_one(const VArgs& a, uint32_t b) {
    const ProofIn in{a.bytes + a.off[b], a.len[b], a.pts + (size_t)b * a.NP, a.pvalid + (size_t)b * a.NP};
    Walk w;
    if (!w.begin(in, a.b2_len)) {
        a.status[b] = ST_MALFORMED;
        return;
    }
    Fe* ev = a.ev + (size_t)b * a.NE;
    Fe* ch = a.ch + (size_t)b * CH_N;
    w.common_scalar(Fr::to_raw(a.vk_repr));
    const Fe* inst = a.inst + (size_t)b * a.NC * a.I * a.ilen;
    for (uint32_t i = 0; i < a.NC * a.I * a.ilen; i++) w.common_scalar(Fr::to_raw(inst[i]));
    bool ok = true;
    uint32_t pi = 0;
    auto points = [&](uint32_t count) {
        for (uint32_t c = 0; c < count && ok; c++) ok = w.point(in, pi++);
    };
    auto squeeze = [&](uint32_t c) {
        if (ok) ch[c] = w.squeeze();
    };
    for (uint32_t ph = 0, cj = 0; ph < a.n_ph; ph++) {
        points(a.ph_points[ph]);
        for (uint32_t e = 0; e < a.ph_nchal[ph]; e++) squeeze(CH_CHAL + a.ph_chal[cj++]);
    }
    squeeze(CH_THETA);
    points(a.walk[1]);
    squeeze(CH_BETA);
    squeeze(CH_GAMMA);
    points(a.walk[2]);
    squeeze(CH_Y);
    points(a.walk[3]);
    squeeze(CH_X);
    for (uint32_t c = 0; c < a.ev_h && ok; c++) ok = w.scalar(in, ev[c]);
    const bool shplonk = a.scheme == ZG_MULTIOPEN_SHPLONK;
    if (shplonk) squeeze(CH_SY);
    squeeze(CH_V);
    points(shplonk ? 1 : a.nW);
    squeeze(CH_U);
    if (shplonk) points(1);
    a.status[b] = !ok ? ST_MALFORMED : !w.at_end(in) ? ST_TRAILING : ST_OK;
}
// One wave per proof, every lane running the same code on the same data (identical stores), so the per-proof work runs
// in uniform control flow.  63 of the 64 lanes are redundant; the layout is kept because the one-lane-per-proof form of
// this kernel and verify_scalars gave wrong field products on the device (the same bodies are right on the host), for a
// reason not found yet.  The two kernels are a small share of a batch's time.
template <class Walk>
__global__ __launch_bounds__(64) void verify_replay(VArgs a) {
    const uint32_t b = blockIdx.x;
    if (b < a.count) replay_one<Walk>(a, b);
}

// in-place inversion of x[0..m) (zeros stay zero) with one field inversion; pre = m scratch elements
__host__ __device__ void batch_inv(Fe* x, Fe* pre, uint32_t m) {
    Fe acc = Fr::one();
    for (uint32_t i = 0; i < m; i++) {
        pre[i] = acc;
        if (!fe_is_zero(x[i])) acc = Fr::mul(acc, x[i]);
    }
    Fe inv = Fr::inv(acc);
    for (uint32_t i = m; i-- > 0;) {
        if (fe_is_zero(x[i])) continue;
        const Fe xi = x[i];
        x[i] = Fr::mul(inv, pre[i]);
        inv = Fr::mul(inv, xi);
    }
}

__host__ __device__ Fe eval_poly(const VArgs& a, const zg_poly& p, const Fe* qe) {
    Fe acc = fe_zero();
    for (uint32_t m = p.first; m < p.first + p.count; m++) {
        const VMono mo = a.monos[m];
        Fe t = mo.coeff;
        for (uint32_t f = 0; f < ZG_MAX_FACTORS; f++) {
            if (f >= mo.n_factors) break;
            const Fe q = qe[mo.factors[f]];
            const Fe r = Fr::mul(t, q);
            t = r;
        }
        acc = Fr::add(acc, t);
    }
    return acc;
}

// (ev: the proof's evaluations; adv: circuit c's advice evaluations among them; iev: its instance evaluations; ch: the
//  proof's challenges)
__host__ __device__ __forceinline__ Fe src_eval(uint32_t src, const Fe* ev, const Fe* adv, const Fe* iev, uint32_t ev_fix, const Fe* ch) {
    return (src & IEVAL) ? iev[src & ~IEVAL] : (src & FIXEV) ? ev[ev_fix + (src & ~FIXEV)] : (src & CHALEV) ? ch[CH_CHAL + (src & ~CHALEV)] : adv[src];
}

__host__ __device__ void scalars_one(const VArgs& a, uint32_t b) {
    Fe* ev = a.ev + (size_t)b * a.NE;
    const Fe* ch = a.ch + (size_t)b * CH_N;
    Fe* qe = a.qe + (size_t)b * (a.n_queries + a.n_iev);
    Fe* iev = qe + a.n_queries;
    Fe* den = a.tmp + (size_t)b * (2 * a.ninv + a.nwork);
    Fe* pre = den + a.ninv;
    Fe* tp = pre + a.ninv;  // SHPLONK: the nT points of T, then v^i z'_i per rotation set
    Fe* vz = tp + a.nT;
    Fe* sc = a.sc + (size_t)b * a.NT;
    const Fe* inst_all = a.inst + (size_t)b * a.NC * a.I * a.ilen;
    const Fe x = ch[CH_X], y = ch[CH_Y], beta = ch[CH_BETA], gamma = ch[CH_GAMMA], theta = ch[CH_THETA];
    const Fe v = ch[CH_V], u = ch[CH_U], one = Fr::one();
    Fe xn = x;
    for (uint32_t i = 0; i < a.log_n; i++) xn = Fr::sqr(xn);

    // denominators: x^n - 1 | x - omega^r for the l's | x omega^rot - omega^i per instance slot and row
    const uint32_t nl = a.bf + 2;
    den[0] = Fr::sub(xn, one);
    for (uint32_t i = 0; i < nl; i++) den[1 + i] = Fr::sub(x, a.lag_w[i]);
    for (uint32_t e = 0; e < a.n_iev; e++) {
        const Fe pt = Fr::mul(x, a.iev_wr[e]);
        Fe wi = one;
        for (uint32_t i = 0; i < a.ilen; i++) {
            den[1 + nl + e * a.ilen + i] = Fr::sub(pt, wi);
            wi = Fr::mul(wi, a.omega);
        }
    }
    // SHPLONK: per (set, point) pair the barycentric denominator prod_(q in S_i, q != p) (p - q), then z_0 = prod_(r in T \ S_0) (u - r)
    const uint32_t d_sh = 1 + nl + a.n_iev * a.ilen;
    const bool shplonk = a.scheme == ZG_MULTIOPEN_SHPLONK;
    if (shplonk) {
        for (uint32_t t = 0; t < a.nT; t++) tp[t] = Fr::mul(x, a.set_wr[t]);
        for (uint32_t i = 0; i < a.nS; i++)
            for (uint32_t f = a.s_first[i]; f < a.s_first[i + 1]; f++) {
                Fe d = one;
                for (uint32_t g = a.s_first[i]; g < a.s_first[i + 1]; g++)
                    if (g != f) d = Fr::mul(d, Fr::sub(tp[a.f_pt[f]], tp[a.f_pt[g]]));
                den[d_sh + f] = d;
            }
        Fe z0 = one;
        for (uint32_t t = 0; t < a.nT; t++)
            if (!(a.s_mask[0] >> t & 1u)) z0 = Fr::mul(z0, Fr::sub(u, tp[t]));
        den[d_sh + a.nF] = z0;
    }
    batch_inv(den, pre, d_sh + (shplonk ? a.nF + 1 : 0));  // (the same denominators serve every circuit of the proof)
    // l_i(x) = (x^n - 1)/n * omega^i / (x - omega^i)
    const Fe num = Fr::mul(Fr::sub(xn, one), a.ifft_div);
    Fe llast = fe_zero(), l0 = fe_zero(), lblind = fe_zero();
    for (uint32_t i = 0; i < nl; i++) {
        const Fe li = Fr::mul(Fr::mul(num, a.lag_w[i]), den[1 + i]);
        if (i == 0) llast = li;
        else if (i + 1 == nl) l0 = li;
        else lblind = Fr::add(lblind, li);
    }
    const Fe lactive = Fr::sub(one, Fr::add(llast, lblind));
    // expected h(x): gates, permutation, lookups folded with y (the prover's order) -- circuit 0's terms, then circuit
    // 1's, and so on, ONE Horner value carried through all of them -- over x^n - 1
    Fe acc = fe_zero();
#define FOLD(val) acc = Fr::add(Fr::mul(acc, y), (val))
    for (uint32_t circ = 0; circ < a.NC; circ++) {
        const Fe* inst = inst_all + (size_t)circ * a.I * a.ilen;
        const Fe* adv = ev + circ * a.nAQ;
        // instance column c at x omega^rot: (x^n - 1)/n * sum_i inst_i omega^i / (x omega^rot - omega^i)
        for (uint32_t e = 0; e < a.n_iev; e++) {
            const Fe* col = inst + (size_t)a.iev_col[e] * a.ilen;
            Fe sum = fe_zero(), wi = one;
            for (uint32_t i = 0; i < a.ilen; i++) {
                sum = Fr::add(sum, Fr::mul(Fr::mul(col[i], wi), den[1 + nl + e * a.ilen + i]));
                wi = Fr::mul(wi, a.omega);
            }
            iev[e] = Fr::mul(sum, num);
        }
        for (uint32_t q = 0; q < a.n_queries; q++) qe[q] = src_eval(a.qsrc[q], ev, adv, iev, a.EV_FIX, ch);
        for (uint32_t g = 0; g < a.n_gates; g++) FOLD(eval_poly(a, a.gates[g], qe));
        if (a.sets > 0) {
            const Fe* pz = ev + a.EV_PZ + circ * a.npz;  // set s: z at 3s, z(wx) at 3s + 1, z(w^last x) at 3s + 2
            FOLD(Fr::mul(Fr::sub(one, pz[0]), l0));
            const Fe zl = pz[3 * (a.sets - 1)];
            FOLD(Fr::mul(Fr::sub(Fr::sqr(zl), zl), llast));
            for (uint32_t s = 1; s < a.sets; s++) FOLD(Fr::mul(Fr::sub(pz[3 * s], pz[3 * (s - 1) + 2]), l0));
            Fe cd0 = Fr::mul(beta, x);
            for (uint32_t s = 0; s < a.sets; s++) {
                Fe left = pz[3 * s + 1], right = pz[3 * s], cd = cd0;
                const uint32_t c0 = s * a.chunk, c1 = c0 + a.chunk > a.P ? a.P : c0 + a.chunk;
                for (uint32_t c = c0; c < c1; c++) {
                    const Fe ce = src_eval(a.psrc[c], ev, adv, iev, a.EV_FIX, ch);
                    const Fe sig = ev[a.EV_SIG + c];
                    left = Fr::mul(left, Fr::add(Fr::add(Fr::mul(beta, sig), ce), gamma));
                    right = Fr::mul(right, Fr::add(Fr::add(ce, cd), gamma));
                    cd = Fr::mul(cd, a.delta);
                }
                cd0 = cd;
                FOLD(Fr::mul(Fr::sub(left, right), lactive));
            }
        }
        const Fe* lk = ev + a.EV_LK + circ * 5 * a.NL;
        for (uint32_t l = 0; l < a.NL; l++) {
            const zg_lookup L = a.lookups[l];
            Fe ai = fe_zero(), ti = fe_zero();
            for (uint32_t e = 0; e < ZG_MAX_LOOKUP_WIDTH; e++) {
                if (e >= L.width) break;
                ai = Fr::add(Fr::mul(ai, theta), eval_poly(a, L.inputs[e], qe));
                ti = Fr::add(Fr::mul(ti, theta), eval_poly(a, L.tables[e], qe));
            }
            const Fe* e5 = lk + 5 * l;  // z, z(wx), a', a'(w^-1 x), s'
            FOLD(Fr::mul(Fr::sub(one, e5[0]), l0));
            FOLD(Fr::mul(Fr::sub(Fr::sqr(e5[0]), e5[0]), llast));
            const Fe lft = Fr::mul(Fr::mul(Fr::add(e5[2], beta), Fr::add(e5[4], gamma)), e5[1]);
            const Fe rgt = Fr::mul(Fr::mul(Fr::add(ai, beta), Fr::add(ti, gamma)), e5[0]);
            FOLD(Fr::mul(Fr::sub(lft, rgt), lactive));
            const Fe ams = Fr::sub(e5[2], e5[4]);
            FOLD(Fr::mul(ams, l0));
            FOLD(Fr::mul(Fr::mul(Fr::sub(e5[2], e5[3]), ams), lactive));
        }
        // the shuffles: l_0 (1 - z), l_last (z^2 - z), l_active (z(wx) (s + gamma) - z (a + gamma))
        const Fe* sh = ev + a.EV_SH + circ * 2 * a.NS;
        for (uint32_t j = 0; j < a.NS; j++) {
            const zg_shuffle S = a.shuffles[j];
            Fe ai = fe_zero(), si = fe_zero();
            for (uint32_t e = 0; e < ZG_MAX_LOOKUP_WIDTH; e++) {
                if (e >= S.width) break;
                ai = Fr::add(Fr::mul(ai, theta), eval_poly(a, S.inputs[e], qe));
                si = Fr::add(Fr::mul(si, theta), eval_poly(a, S.shuffles[e], qe));
            }
            const Fe z = sh[2 * j], zn = sh[2 * j + 1];
            FOLD(Fr::mul(Fr::sub(one, z), l0));
            FOLD(Fr::mul(Fr::sub(Fr::sqr(z), z), llast));
            FOLD(Fr::mul(Fr::sub(Fr::mul(zn, Fr::add(si, gamma)), Fr::mul(z, Fr::add(ai, gamma))), lactive));
        }
    }
#undef FOLD
    ev[a.ev_h] = Fr::mul(acc, den[0]);

    // term scalars: u^j v^k on each commitment (x_n^i more on the h pieces), -sum u^j e_j on g0, u^j and u^j z_j on W_j
    for (uint32_t t = 0; t < a.NT; t++) sc[t] = fe_zero();
    const uint32_t T_SHARED = a.NP + a.nL, T_G0 = a.NT - 1, PT_H = a.PT_RAND + 1, PT_W = PT_H + a.qpd;
    Fe g0 = fe_zero();
    if (shplonk) {
        // the Lagrange basis of every set at u, prod_(q != p) (u - q) / prod_(q != p) (p - q), in the denominators' place;
        // v^i z'_i with z'_0 = 1, z'_i = z_i / z_0, z_i = prod_(r in T \ S_i) (u - r)
        for (uint32_t i = 0; i < a.nS; i++)
            for (uint32_t f = a.s_first[i]; f < a.s_first[i + 1]; f++) {
                Fe l = den[d_sh + f];
                for (uint32_t g = a.s_first[i]; g < a.s_first[i + 1]; g++)
                    if (g != f) l = Fr::mul(l, Fr::sub(u, tp[a.f_pt[g]]));
                den[d_sh + f] = l;
            }
        Fe vi = one;
        for (uint32_t i = 0; i < a.nS; i++) {
            Fe z = one;
            for (uint32_t t = 0; t < a.nT; t++)
                if (!(a.s_mask[i] >> t & 1u)) z = Fr::mul(z, Fr::sub(u, tp[t]));
            vz[i] = i ? Fr::mul(vi, Fr::mul(z, den[d_sh + a.nF])) : one;
            vi = Fr::mul(vi, v);
        }
    }
    const Fe sy = ch[shplonk ? CH_SY : CH_V];
    for (uint32_t q = 0; q < a.n_oq; q++) {
        const VQuery oq = a.oq[q];
        // GWC: u^j v^k on the commitment and the evaluation.  SHPLONK: v^i z'_i y^j on the commitment, once, and on
        // R_ij(u), of which this query's evaluation is the share of one point
        const Fe coef = shplonk ? Fr::mul(vz[oq.set], Fr::pow_u64(sy, oq.vpow)) : Fr::mul(Fr::pow_u64(u, oq.set), Fr::pow_u64(v, oq.vpow));
        if (shplonk) {
            g0 = Fr::sub(g0, Fr::mul(Fr::mul(coef, ev[oq.eval]), den[d_sh + (oq.pt & ~FIRST_PT)]));
            if (!(oq.pt & FIRST_PT)) continue;
        } else {
            g0 = Fr::sub(g0, Fr::mul(coef, ev[oq.eval]));
        }
        if (oq.term == HREF) {
            Fe c = coef;
            for (uint32_t i = 0; i < a.qpd; i++) {
                sc[PT_H + i] = Fr::add(sc[PT_H + i], c);
                c = Fr::mul(c, xn);
            }
        } else {
            const uint32_t t = (oq.term & SHARED) ? T_SHARED + (oq.term & ~SHARED) : oq.term;
            sc[t] = Fr::add(sc[t], coef);
        }
    }
    sc[T_G0] = g0;
    if (shplonk) {  // R_b = ... - Z_0 h1 + u h2 with Z_0 = prod_(r in S_0) (u - r); the left side is h2
        Fe Z0 = one;
        for (uint32_t f = a.s_first[0]; f < a.s_first[1]; f++) Z0 = Fr::mul(Z0, Fr::sub(u, tp[a.f_pt[f]]));
        sc[PT_W] = Fr::neg(Z0);
        sc[PT_W + 1] = u;
        sc[a.NP] = one;
    } else {
        Fe uj = one;
        for (uint32_t j = 0; j < a.nsets; j++) {
            sc[a.NP + j] = uj;
            sc[PT_W + j] = Fr::add(sc[PT_W + j], Fr::mul(uj, Fr::mul(x, a.set_wr[j])));
            uj = Fr::mul(uj, u);
        }
    }
    for (uint32_t t = 0; t < a.NT; t++) sc[t] = Fr::to_raw(sc[t]);
}
__global__ __launch_bounds__(64) void verify_scalars(VArgs a) {
    const uint32_t b = blockIdx.x;
    if (b < a.count && a.status[b] == ST_OK) scalars_one(a, b);
}

constexpr uint32_t TERMS_WG = 128;

__device__ void tree_sum(XYZZ* sl, XYZZ* sr, uint32_t tid) {
    for (uint32_t h = TERMS_WG / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
            sl[tid] = xyzz_add(sl[tid], sl[tid + h]);
            sr[tid] = xyzz_add(sr[tid], sr[tid + h]);
        }
    }
    __syncthreads();
}

// workgroup b: proof b's (L_b, R_b); lanes 0 and 1 then weight them by r_b (a proof that did not parse: the identity)
__global__ __launch_bounds__(TERMS_WG) void verify_terms(VArgs a) {
    __shared__ XYZZ sl[TERMS_WG], sr[TERMS_WG];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const bool live = a.status[b] == ST_OK;
    XYZZ accl = xyzz_identity(), accr = xyzz_identity();
    if (live) {
        const Affine* pts = a.pts + (size_t)b * a.NP;
        const Fe* sc = a.sc + (size_t)b * a.NT;
        const uint32_t PT_L = a.NP - a.nL;  // (the left side's points end the proof: every W of GWC, SHPLONK's h2)
        for (uint32_t t = tid; t < a.NT; t += TERMS_WG) {
            const bool left = t >= a.NP && t < a.NP + a.nL;
            const Affine p = t < a.NP ? pts[t] : left ? pts[PT_L + t - a.NP] : a.shared[t - a.NP - a.nL];
            const XYZZ m = xyzz_mul_raw(p, sc[t].l);
            if (left) accl = xyzz_add(accl, m);
            else accr = xyzz_add(accr, m);
        }
    }
    sl[tid] = accl;
    sr[tid] = accr;
    tree_sum(sl, sr, tid);
    if (tid < 2) {
        const XYZZ s = tid == 0 ? sl[0] : sr[0];
        a.wpair[2 * b + tid] = live ? xyzz_mul_raw(xyzz_to_affine(s), a.rb[b].l) : xyzz_identity();
    }
}

__global__ __launch_bounds__(TERMS_WG) void verify_fold(VArgs a) {
    __shared__ XYZZ sl[TERMS_WG], sr[TERMS_WG];
    const uint32_t tid = threadIdx.x;
    XYZZ accl = xyzz_identity(), accr = xyzz_identity();
    for (uint32_t b = tid; b < a.count; b += TERMS_WG) {
        accl = xyzz_add(accl, a.wpair[2 * b]);
        accr = xyzz_add(accr, a.wpair[2 * b + 1]);
    }
    sl[tid] = accl;
    sr[tid] = accr;
    tree_sum(sl, sr, tid);
    if (tid == 0) {
        a.out[0] = sl[0];
        a.out[1] = sr[0];
    }
}

Fe fe_of(const zg_fr& x) {
    Fe r;
    std::memcpy(&r, &x, sizeof(r));
    return r;
}

}  // namespace
}  // namespace zg

using namespace zg;

struct zg_verifier {
    zg_ctx* ctx = nullptr;
    VArgs a{};
    zg_g2_affine g2{}, s_g2{};
    std::vector<void*> owned;  // circuit arrays
    ProofShape shape;                    // what the layout of a proof of NC circuits is built from
    int scheme = ZG_MULTIOPEN_GWC;       // zg_verifier_set_multiopen
    int transcript = ZG_TRANSCRIPT_EVM;  // zg_verifier_set_transcript
    // zg_verifier_set_phases (shape.advice_phase / challenge_phase hold the setting): the challenges the circuit's
    // expressions name, and the setting's number, which the cached tables are keyed by
    uint32_t n_used = 0;
    int phase_gen = 0;
    bool phased() const { return !shape.challenge_phase.empty() || build_phases() > 1; }
    uint32_t build_phases() const {
        uint32_t last = 0;
        for (uint8_t ph : shape.advice_phase) last = ph > last ? ph : last;
        return last + 1;
    }
    struct Table {
        ProofLayout lay;
        const VQuery* oq = nullptr;  // the layout's queries under this verifier's handles, on the device
        uint32_t n_oq = 0;
        // SHPLONK: the rotation sets (VArgs)
        uint32_t nF = 0;
        const uint32_t *s_first = nullptr, *s_mask = nullptr, *f_pt = nullptr;
    };
    std::map<std::array<int, 3>, Table> tables;  // the layouts made so far, by (scheme, circuits, phase setting)
    const Table* table = nullptr;                // the one in use (set_circuits)
    // batch buffers, grown on demand (cap: proofs; pts / ev / sc: elements, their size per proof follows NC)
    size_t cap = 0, bytes_cap = 0, inst_cap = 0, tmp_cap = 0, pts_cap = 0, ev_cap = 0, sc_cap = 0;
    std::vector<void*> batch;
};

namespace {

template <class T>
int upload(zg_verifier* v, const T** dst, const std::vector<T>& src) {
    void* p = nullptr;
    ZG_HIP(hipMalloc(&p, (src.empty() ? 1 : src.size()) * sizeof(T)));
    v->owned.push_back(p);
    if (!src.empty()) ZG_HIP(hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return ZG_OK;
}

template <class T>
int grow(zg_verifier* v, T** dst, size_t elems) {
    void* p = nullptr;
    ZG_HIP(hipMalloc(&p, (elems ? elems : 1) * sizeof(T)));
    v->batch.push_back(p);
    *dst = static_cast<T*>(p);
    return ZG_OK;
}

void free_batch(zg_verifier* v) {
    for (void* p : v->batch) (void)hipFree(p);
    v->batch.clear();
    v->cap = v->bytes_cap = v->inst_cap = v->tmp_cap = v->pts_cap = v->ev_cap = v->sc_cap = 0;
}

// batch buffers for `count` proofs of `bytes` bytes in all, `inst` instance values and `tmp` inversion scratch elements
int ensure(zg_verifier* v, size_t count, size_t bytes, size_t inst, size_t tmp) {
    VArgs& a = v->a;
    if (count <= v->cap && bytes <= v->bytes_cap && inst <= v->inst_cap && tmp <= v->tmp_cap && count * a.NP <= v->pts_cap &&
        count * a.NE <= v->ev_cap && count * a.NT <= v->sc_cap)
        return ZG_OK;
    free_batch(v);
    count = std::max(count, (size_t)1);
    bytes = std::max(bytes, (size_t)1);
    inst = std::max(inst, (size_t)1);
    tmp = std::max(tmp, (size_t)1);
    ZG_TRY(grow(v, (uint8_t**)&a.bytes, bytes));
    ZG_TRY(grow(v, (uint64_t**)&a.off, count));
    ZG_TRY(grow(v, (uint64_t**)&a.len, count));
    ZG_TRY(grow(v, (Fe**)&a.inst, inst));
    ZG_TRY(grow(v, &a.pts, count * a.NP));
    ZG_TRY(grow(v, &a.enc, count * a.NP * 32));
    ZG_TRY(grow(v, &a.pvalid, count * a.NP));
    ZG_TRY(grow(v, &a.ev, count * a.NE));
    ZG_TRY(grow(v, &a.ch, count * CH_N));
    ZG_TRY(grow(v, &a.status, count));
    ZG_TRY(grow(v, &a.qe, count * (a.n_queries + a.n_iev)));
    ZG_TRY(grow(v, &a.sc, count * a.NT));
    ZG_TRY(grow(v, (Fe**)&a.rb, count));
    ZG_TRY(grow(v, &a.wpair, count * 2));
    ZG_TRY(grow(v, &a.out, 2));
    ZG_TRY(grow(v, &a.tmp, tmp));
    v->cap = count;
    v->bytes_cap = bytes;
    v->inst_cap = inst;
    v->tmp_cap = tmp;
    v->pts_cap = count * a.NP;
    v->ev_cap = count * a.NE;
    v->sc_cap = count * a.NT;
    return ZG_OK;
}

Fe omega_pow(const Fe& omega, const Fe& omega_inv, int64_t r) {
    return Fr::pow_u64(r >= 0 ? omega : omega_inv, (uint64_t)(r >= 0 ? r : -r));
}

// The layout of a proof of NC circuit instances (proof_layout.h, built once per scheme and NC) into v->a, with its opening
// queries as a VQuery table.  The verifier's handle of a commitment is its term index: a proof's own points stand first,
// in the layout's order, the key's fixed and sigma commitments are SHARED, h is HREF; a layout point is a point set.
int set_circuits(zg_verifier* v, uint32_t NC) {
    VArgs& a = v->a;
    const bool shplonk = v->scheme == ZG_MULTIOPEN_SHPLONK;
    const std::array<int, 3> table_key = {v->scheme, (int)NC, v->phase_gen};
    auto it = v->tables.find(table_key);
    if (it == v->tables.end()) {
        zg_verifier::Table t;
        t.lay = build_layout(v->shape, NC, shplonk);
        const ProofLayout& l = t.lay;
        auto term = [&](const ProofLayout::Query& q) {
            return q.fam == FIXED ? SHARED | q.index : q.fam == SIGMA ? SHARED | (a.F + q.index) : q.fam == H ? HREF : l.point_index(q.fam, q.circuit, q.index);
        };
        std::vector<VQuery> oq;
        if (shplonk) {
            ZG_REQUIRE(l.rotations.size() <= PC_MAX_POINTS, ZG_ERR_UNSUPPORTED, "zg_verifier: %zu opening points (max %u)", l.rotations.size(),
                       PC_MAX_POINTS);
            ZG_REQUIRE(l.rsets.size() <= HC_MAX_SETS, ZG_ERR_UNSUPPORTED, "zg_verifier: %zu rotation sets (max %u)", l.rsets.size(), HC_MAX_SETS);
            std::vector<uint32_t> s_first(1, 0), s_mask, f_pt;
            for (const ProofLayout::RotationSet& s : l.rsets) {
                s_mask.push_back(0);
                for (uint32_t p : s.points) s_mask.back() |= 1u << p;
                f_pt.insert(f_pt.end(), s.points.begin(), s.points.end());
                s_first.push_back((uint32_t)f_pt.size());
            }
            // a repeated (commitment, point) pair counts once; the commitment's own scalar goes with its first query
            std::vector<char> seen(l.coms.size(), 0);
            for (const ProofLayout::Query& q : l.queries) {
                if (q.com == ProofLayout::NONE) continue;
                const ProofLayout::Com& c = l.coms[q.com];
                uint32_t f = s_first[c.set];
                while (f_pt[f] != q.point) f++;
                oq.push_back({term(q), q.eval, c.set, c.place, f | (seen[q.com] ? 0u : FIRST_PT)});
                seen[q.com] = 1;
            }
            t.nF = (uint32_t)f_pt.size();
            ZG_TRY(upload(v, &t.s_first, s_first));
            ZG_TRY(upload(v, &t.s_mask, s_mask));
            ZG_TRY(upload(v, &t.f_pt, f_pt));
        } else {
            // v-powers run down within a set: the first query of a set of m gets v^(m-1)
            for (const ProofLayout::Query& q : l.queries) oq.push_back({term(q), q.eval, q.point, 0, 0});
            for (const std::vector<uint32_t>& set : l.at)
                for (size_t k = 0; k < set.size(); k++) oq[set[k]].vpow = (uint32_t)(set.size() - 1 - k);
        }
        ZG_TRY(upload(v, &t.oq, oq));
        t.n_oq = (uint32_t)oq.size();
        if (!a.set_wr) {  // (the points do not depend on NC or the scheme)
            std::vector<Fe> set_wr;
            const int64_t n = (int64_t)1 << a.log_n;
            for (int64_t r : l.rotations) set_wr.push_back(Fr::pow_u64(a.omega, (uint64_t)(((r % n) + n) % n)));
            ZG_TRY(upload(v, &a.set_wr, set_wr));
        }
        it = v->tables.emplace(table_key, std::move(t)).first;
    }
    const zg_verifier::Table& t = it->second;
    const ProofLayout& l = t.lay;
    v->table = &t;
    a.NC = NC;
    a.scheme = (uint32_t)v->scheme;
    a.walk[0] = l.pt[ADVICE].count;
    a.n_ph = (uint32_t)l.phases.size();
    for (uint32_t ph = 0, cj = 0, at = l.pt[ADVICE].first; ph < a.n_ph; at = l.phases[ph++].end) {
        a.ph_points[ph] = l.phases[ph].end - at;
        a.ph_nchal[ph] = (uint32_t)l.phases[ph].challenges.size();
        for (uint32_t j : l.phases[ph].challenges) a.ph_chal[cj++] = j;
    }
    a.walk[1] = l.pt[PERMUTED].count;
    a.walk[2] = l.pt[PERM_Z].count + l.pt[LOOKUP_Z].count + l.shuffle_pt.count + l.pt[RANDOM].count;
    a.EV_SH = l.shuffle_ev.first;
    a.walk[3] = l.pt[H_PIECE].count;
    a.PT_RAND = l.pt[RANDOM].first;
    a.EV_FIX = l.ev[EV_FIXED].first; a.EV_SIG = l.ev[EV_SIGMA].first; a.EV_PZ = l.ev[EV_PERM].first; a.EV_LK = l.ev[EV_LOOKUP].first;
    a.npz = l.ev[EV_PERM].count / NC;
    a.ev_h = l.ev[EV_H].first;
    a.NE = a.ev_h + 1;
    a.nsets = (uint32_t)l.rotations.size();
    a.nT = shplonk ? a.nsets : 0;
    a.nW = l.pt[OPENING].count;
    a.nL = shplonk ? 1 : a.nW;  // (the left side's terms: every W; h2)
    a.NP = l.n_points();
    a.NT = a.NP + a.nL + a.F + a.P + 1;
    a.b2_len = l.bytes(true);
    a.oq = t.oq;
    a.n_oq = t.n_oq;  // (SHPLONK's table holds a repeated (commitment, point) pair once)
    a.nS = (uint32_t)l.rsets.size(); a.nF = t.nF; a.nwork = a.nT + a.nS;
    a.s_first = t.s_first; a.s_mask = t.s_mask; a.f_pt = t.f_pt;
    return ZG_OK;
}

int verifier_create(zg_verifier* v, const zg_circuit* cs, const zg_shuffle* shuffles_in, uint32_t n_shuffles, const zg_g1_affine* fixed_c,
                    const zg_g1_affine* sigma_c, const zg_g1_affine* g0, const zg_fr* vk_repr) {
    VArgs& a = v->a;
    const uint32_t n_log = cs->k;
    const uint64_t n = 1ull << n_log;
    a.log_n = n_log;
    a.A = cs->n_advice; a.F = cs->n_fixed; a.I = cs->n_instance; a.P = cs->n_perm_columns; a.NL = cs->n_lookups;
    a.bf = cs->blinding_factors;
    a.chunk = cs->cs_degree - 2;
    a.sets = a.P ? (a.P + a.chunk - 1) / a.chunk : 0;
    a.qpd = cs->cs_degree - 1;
    a.nAQ = cs->n_advice_queries; a.nFQ = cs->n_fixed_queries;
    a.n_gates = cs->n_gates; a.n_lookups = cs->n_lookups; a.n_queries = cs->n_queries;
    a.omega = host_domain_omega(n_log);
    const Fe omega_inv = Fr::inv(a.omega);
    a.ifft_div = Fr::inv(Fr::from_u64(n));
    a.delta = fr_delta();
    a.vk_repr = fe_of(*vk_repr);
    ProofShape& sh = v->shape;
    sh.A = a.A; sh.F = a.F; sh.P = a.P; sh.NL = a.NL; sh.sets = a.sets; sh.qpd = a.qpd; sh.bf = a.bf; sh.log_n = a.log_n;
    sh.NS = a.NS = n_shuffles;
    for (uint32_t i = 0; i < a.nAQ; i++) sh.advice_queries.push_back({cs->advice_queries[i].column, cs->advice_queries[i].rotation});
    for (uint32_t i = 0; i < a.nFQ; i++) sh.fixed_queries.push_back({cs->fixed_queries[i].column, cs->fixed_queries[i].rotation});

    // where each circuit query's evaluation comes from
    std::vector<uint32_t> iev_col;
    std::vector<Fe> iev_wr;
    std::vector<std::pair<uint32_t, int32_t>> iev_key;
    auto inst_slot = [&](uint32_t col, int32_t rot) {
        for (size_t e = 0; e < iev_key.size(); e++)
            if (iev_key[e].first == col && iev_key[e].second == rot) return (uint32_t)e | IEVAL;
        iev_key.push_back({col, rot});
        iev_col.push_back(col);
        iev_wr.push_back(omega_pow(a.omega, omega_inv, rot));
        return (uint32_t)(iev_key.size() - 1) | IEVAL;
    };
    auto source = [&](uint32_t kind, uint32_t col, int32_t rot, uint32_t* out) {
        if (kind == ZG_CHALLENGE) {
            if (col >= ZG_MAX_CHALLENGES || rot != 0) return false;
            v->n_used = std::max(v->n_used, col + 1);
            *out = CHALEV | col;
            return true;
        }
        if (kind == ZG_INSTANCE) {
            *out = inst_slot(col, rot);
            return true;
        }
        const zg_query* list = kind == ZG_ADVICE ? cs->advice_queries : cs->fixed_queries;
        const uint32_t cnt = kind == ZG_ADVICE ? a.nAQ : a.nFQ, base = kind == ZG_ADVICE ? 0 : FIXEV;
        bool found = false;
        for (uint32_t i = 0; i < cnt; i++)
            if (list[i].column == col && list[i].rotation == rot) {
                *out = base + i;
                found = true;
            }
        return found;
    };
    std::vector<uint32_t> qsrc(a.n_queries), psrc(a.P);
    for (uint32_t q = 0; q < a.n_queries; q++)
        ZG_REQUIRE(source(cs->queries[q].kind, cs->queries[q].column, cs->queries[q].rotation, &qsrc[q]),
                   ZG_ERR_INVALID_ARG, "zg_verifier_create: query %u is not among the circuit's column queries", q);
    sh.challenge_phase.assign(v->n_used, 0);  // (the default: every challenge behind phase 0's commitments)
    for (uint32_t c = 0; c < a.P; c++)
        ZG_REQUIRE(cs->perm_columns[c].kind != ZG_CHALLENGE && source(cs->perm_columns[c].kind, cs->perm_columns[c].column, 0, &psrc[c]), ZG_ERR_INVALID_ARG,
                   "zg_verifier_create: permutation column %u has no query at the current row", c);
    a.n_iev = (uint32_t)iev_col.size();

    std::vector<Fe> lag_w;
    for (int64_t r = -(int64_t)(a.bf + 1); r <= 0; r++) lag_w.push_back(omega_pow(a.omega, omega_inv, r));

    std::vector<VMono> monos(cs->n_monomials);
    for (uint32_t m = 0; m < cs->n_monomials; m++) {
        VMono& d = monos[m];
        std::memset(&d, 0, sizeof(d));
        d.coeff = fe_of(cs->monomials[m].coeff);
        d.n_factors = cs->monomials[m].n_factors;
        ZG_REQUIRE(d.n_factors <= ZG_MAX_FACTORS, ZG_ERR_INVALID_ARG, "zg_verifier_create: monomial %u too long", m);
        for (uint32_t f = 0; f < d.n_factors; f++) {
            d.factors[f] = cs->monomials[m].factors[f];
            ZG_REQUIRE(d.factors[f] < a.n_queries, ZG_ERR_INVALID_ARG, "zg_verifier_create: bad factor in monomial %u", m);
        }
    }
    std::vector<zg_poly> gates(cs->gates, cs->gates + cs->n_gates);
    std::vector<zg_lookup> lookups(cs->lookups, cs->lookups + cs->n_lookups);
    auto poly_ok = [&](const zg_poly& p) { return (uint64_t)p.first + p.count <= cs->n_monomials; };
    for (const zg_poly& g : gates) ZG_REQUIRE(poly_ok(g), ZG_ERR_INVALID_ARG, "zg_verifier_create: gate out of range");
    for (const zg_lookup& l : lookups) {
        ZG_REQUIRE(l.width <= ZG_MAX_LOOKUP_WIDTH, ZG_ERR_INVALID_ARG, "zg_verifier_create: lookup too wide");
        for (uint32_t e = 0; e < l.width; e++)
            ZG_REQUIRE(poly_ok(l.inputs[e]) && poly_ok(l.tables[e]), ZG_ERR_INVALID_ARG,
                       "zg_verifier_create: lookup polynomial out of range");
    }
    std::vector<zg_shuffle> shuffles(shuffles_in, shuffles_in + n_shuffles);  // (validated: shuffles_ok)
    for (uint32_t i = 0; i < a.nAQ; i++)
        ZG_REQUIRE(cs->advice_queries[i].column < a.A, ZG_ERR_INVALID_ARG, "zg_verifier_create: bad advice query");
    for (uint32_t i = 0; i < a.nFQ; i++)
        ZG_REQUIRE(cs->fixed_queries[i].column < a.F, ZG_ERR_INVALID_ARG, "zg_verifier_create: bad fixed query");
    for (uint32_t c : iev_col) ZG_REQUIRE(c < a.I, ZG_ERR_INVALID_ARG, "zg_verifier_create: bad instance query");
    std::vector<Affine> shared(a.F + a.P + 1);
    if (a.F) std::memcpy(shared.data(), fixed_c, a.F * sizeof(Affine));
    if (a.P) std::memcpy(shared.data() + a.F, sigma_c, a.P * sizeof(Affine));
    std::memcpy(&shared[a.F + a.P], g0, sizeof(Affine));

    ZG_TRY(upload(v, &a.monos, monos));
    ZG_TRY(upload(v, &a.gates, gates));
    ZG_TRY(upload(v, &a.lookups, lookups));
    ZG_TRY(upload(v, &a.shuffles, shuffles));
    ZG_TRY(upload(v, &a.qsrc, qsrc));
    ZG_TRY(upload(v, &a.psrc, psrc));
    ZG_TRY(upload(v, &a.iev_col, iev_col));
    ZG_TRY(upload(v, &a.iev_wr, iev_wr));
    ZG_TRY(upload(v, &a.lag_w, lag_w));
    ZG_TRY(upload(v, &a.shared, shared));
    return set_circuits(v, 1);
}

}  // namespace

extern "C" {

int zg_verifier_create(zg_ctx* ctx, const zg_circuit* cs, const zg_g1_affine* fixed_commitments,
                       const zg_g1_affine* sigma_commitments, const zg_g1_affine* g0, const zg_g2_affine* g2,
                       const zg_g2_affine* s_g2, const zg_fr* vk_repr, zg_verifier** out) {
    return zg_verifier_create_shuffles(ctx, cs, nullptr, 0, fixed_commitments, sigma_commitments, g0, g2, s_g2, vk_repr, out);
}

int zg_verifier_create_shuffles(zg_ctx* ctx, const zg_circuit* cs, const zg_shuffle* shuffles, uint32_t n_shuffles,
                                const zg_g1_affine* fixed_commitments, const zg_g1_affine* sigma_commitments, const zg_g1_affine* g0,
                                const zg_g2_affine* g2, const zg_g2_affine* s_g2, const zg_fr* vk_repr, zg_verifier** out) {
    ZG_REQUIRE(ctx && cs && g0 && g2 && s_g2 && vk_repr && out, ZG_ERR_INVALID_ARG, "zg_verifier_create: null argument");
    ZG_TRY(shuffles_ok("zg_verifier_create_shuffles", cs, shuffles, n_shuffles));  // (the prover's checks, cs_degree included)
    ZG_REQUIRE((fixed_commitments || cs->n_fixed == 0) && (sigma_commitments || cs->n_perm_columns == 0),
               ZG_ERR_INVALID_ARG, "zg_verifier_create: null commitments");
    ZG_REQUIRE(cs->k >= 1 && cs->k <= 28 && cs->cs_degree >= 3, ZG_ERR_UNSUPPORTED, "zg_verifier_create: k = %u, degree %u",
               cs->k, cs->cs_degree);
    ZG_ENTER(ctx);
    zg_verifier* v = new zg_verifier();
    v->ctx = ctx;
    v->g2 = *g2;
    v->s_g2 = *s_g2;
    const int st = verifier_create(v, cs, shuffles, n_shuffles, fixed_commitments, sigma_commitments, g0, vk_repr);
    if (st != ZG_OK) {
        zg_verifier_destroy(v);
        return st;
    }
    *out = v;
    return ZG_OK;
}

void zg_verifier_destroy(zg_verifier* v) {
    if (!v) return;
    {
        std::lock_guard<std::recursive_mutex> lock(v->ctx->mu);
        (void)hipSetDevice(v->ctx->device);
        (void)hipStreamSynchronize(v->ctx->stream);
        free_batch(v);
        for (void* p : v->owned) (void)hipFree(p);
    }
    delete v;
}

int zg_verifier_set_multiopen(zg_verifier* v, int scheme) {
    ZG_REQUIRE(v, ZG_ERR_INVALID_ARG, "zg_verifier_set_multiopen: null verifier");
    ZG_REQUIRE(scheme == ZG_MULTIOPEN_GWC || scheme == ZG_MULTIOPEN_SHPLONK, ZG_ERR_INVALID_ARG, "zg_verifier_set_multiopen: scheme %d", scheme);
    ZG_ENTER(v->ctx);
    v->scheme = scheme;
    return ZG_OK;
}

int zg_verifier_multiopen(const zg_verifier* v) { return v ? v->scheme : ZG_MULTIOPEN_GWC; }

int zg_verifier_set_transcript(zg_verifier* v, int transcript) {
    ZG_REQUIRE(v, ZG_ERR_INVALID_ARG, "zg_verifier_set_transcript: null verifier");
    ZG_REQUIRE(transcript == ZG_TRANSCRIPT_EVM || transcript == ZG_TRANSCRIPT_BLAKE2B, ZG_ERR_INVALID_ARG,
               "zg_verifier_set_transcript: transcript %d", transcript);
    ZG_ENTER(v->ctx);
    v->transcript = transcript;
    return ZG_OK;
}

int zg_verifier_transcript(const zg_verifier* v) { return v ? v->transcript : ZG_TRANSCRIPT_EVM; }

int zg_verifier_set_phases(zg_verifier* v, const uint8_t* advice_phase, uint32_t n_challenges, const uint8_t* challenge_phase) {
    ZG_REQUIRE(v, ZG_ERR_INVALID_ARG, "zg_verifier_set_phases: null verifier");
    const char* why = phases_error(v->a.A, advice_phase, v->n_used, n_challenges, challenge_phase, ZG_MAX_PHASES, ZG_MAX_CHALLENGES);
    ZG_REQUIRE(!why, ZG_ERR_INVALID_ARG, "zg_verifier_set_phases: %s", why);
    ZG_ENTER(v->ctx);
    v->shape.advice_phase.assign(advice_phase, advice_phase + v->a.A);
    v->shape.challenge_phase.assign(challenge_phase, challenge_phase + n_challenges);
    v->phase_gen++;  // (the tables made so far state another order: new ones at the next verification)
    return ZG_OK;
}

int zg_verifier_phases(const zg_verifier* v, uint8_t* advice_phase, uint32_t* n_challenges, uint8_t* challenge_phase) {
    if (!v) return 0;
    for (uint32_t c = 0; advice_phase && c < v->a.A; c++) advice_phase[c] = c < v->shape.advice_phase.size() ? v->shape.advice_phase[c] : 0;
    if (n_challenges) *n_challenges = (uint32_t)v->shape.challenge_phase.size();
    for (size_t j = 0; challenge_phase && j < v->shape.challenge_phase.size(); j++) challenge_phase[j] = v->shape.challenge_phase[j];
    return (int)v->build_phases();
}

int zg_verifier_verify_batch(zg_verifier* v, size_t count, const uint8_t* const* proofs, const size_t* proof_lens,
                             const zg_fr* const* instance, size_t instance_len, const uint8_t key[32], int* verdicts) {
    return zg_verifier_verify_multi(v, count, 1, proofs, proof_lens, instance, instance_len, key, verdicts);
}

// zg_verifier_verify_multi keeps to circuits without challenges, later phases and shuffles when a proof holds several
// circuits (`general` = false); zg_verifier_verify_circuits is the same body without the two refusals
static int verify_multi_impl(bool general, zg_verifier* v, size_t count, size_t circuits, const uint8_t* const* proofs,
                             const size_t* proof_lens, const zg_fr* const* instance, size_t instance_len, const uint8_t key[32],
                             int* verdicts) {
    ZG_REQUIRE(v && key && (count == 0 || (proofs && proof_lens && verdicts && (instance || v->a.I == 0))),
               ZG_ERR_INVALID_ARG, "zg_verifier_verify_batch: null argument");
    ZG_REQUIRE(circuits >= 1 && circuits <= 1024, ZG_ERR_INVALID_ARG, "zg_verifier_verify_multi: proofs of %zu circuits", circuits);
    ZG_REQUIRE(general || circuits == 1 || !v->phased(), ZG_ERR_UNSUPPORTED,
               "zg_verifier_verify_multi: proofs of several circuits are not verified for a circuit with challenges or advice phases "
               "(zg_verifier_verify_circuits)");
    ZG_REQUIRE(general || circuits == 1 || v->a.NS == 0, ZG_ERR_UNSUPPORTED,
               "zg_verifier_verify_multi: proofs of several circuits are not verified for a circuit with shuffles (zg_verifier_verify_circuits)");
    ZG_REQUIRE(count < (1u << 24) && instance_len < (1u << 24), ZG_ERR_UNSUPPORTED,
               "zg_verifier_verify_batch: %zu proofs of %zu instance rows", count, instance_len);
    if (count == 0) return ZG_OK;
    zg_ctx* ctx = v->ctx;
    std::vector<int> status(count);
    std::vector<XYZZ> wpair(2 * count);
    XYZZ acc[2];
    {
        // the device part holds the context (and this verifier's buffers); the host pairings below do not
        ZG_ENTER(ctx);
        VArgs& a = v->a;
        ZG_TRY(set_circuits(v, (uint32_t)circuits));
        const size_t one_inst = (size_t)a.I * instance_len, per_inst = circuits * one_inst;
        std::vector<uint64_t> off(count), len(count);
        size_t total = 0;
        for (size_t b = 0; b < count; b++) {
            ZG_REQUIRE(proofs[b] || proof_lens[b] == 0, ZG_ERR_INVALID_ARG, "zg_verifier_verify_batch: proof %zu is null", b);
            for (size_t c = 0; c < circuits; c++)
                ZG_REQUIRE(per_inst == 0 || instance[b * circuits + c], ZG_ERR_INVALID_ARG, "zg_verifier_verify_batch: instance %zu is null",
                           b * circuits + c);
            off[b] = total;
            len[b] = proof_lens[b];
            total += proof_lens[b];
        }
        const bool blake2b = v->transcript == ZG_TRANSCRIPT_BLAKE2B;
        std::vector<uint8_t> bytes(total ? total : 1);
        // Blake2b: every proof's commitments side by side for the decompression kernel (a short proof: zeros, never read)
        std::vector<uint8_t> enc(blake2b ? count * a.NP * 32 : 0);
        std::vector<Fe> inst(count * per_inst);
        std::vector<Fe> rb(count);
        uint32_t kw[8];
        std::memcpy(kw, key, 32);
        for (size_t b = 0; b < count; b++) {
            if (proof_lens[b]) std::memcpy(bytes.data() + off[b], proofs[b], proof_lens[b]);
            if (blake2b && proof_lens[b] >= a.b2_len)
                for (uint32_t pt = 0; pt < a.NP; pt++) std::memcpy(&enc[(b * a.NP + pt) * 32], proofs[b] + 32 * (size_t)v->table->lay.item_of_point(pt), 32);
            for (size_t c = 0; c < circuits && per_inst; c++)
                std::memcpy(inst.data() + b * per_inst + c * one_inst, instance[b * circuits + c], one_inst * sizeof(Fe));
            rb[b] = Fr::to_raw(rand_fr_host(kw, TAG_VERIFY_BATCH, b));
            if (fe_is_zero(rb[b])) rb[b].l[0] = 1;  // (a zero weight would hide the proof; probability 2^-254)
        }
        // inversion scratch per proof: x^n - 1, the bf + 2 Lagrange denominators, one per instance slot and row (twice)
        // (SHPLONK: one more per (set, point) pair and z_0; behind the two halves its nT points and nS set weights)
        a.ninv = 1 + (a.bf + 2) + a.n_iev * (uint32_t)instance_len + (a.scheme == ZG_MULTIOPEN_SHPLONK ? a.nF + 1 : 0);
        ZG_TRY(ensure(v, count, total, count * per_inst, count * (2 * (size_t)a.ninv + a.nwork)));
        a.count = (uint32_t)count;
        a.ilen = (uint32_t)instance_len;
        hipStream_t st = ctx->stream;
        ZG_HIP(hipMemcpyAsync((void*)a.bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st));
        ZG_HIP(hipMemcpyAsync((void*)a.off, off.data(), count * 8, hipMemcpyHostToDevice, st));
        ZG_HIP(hipMemcpyAsync((void*)a.len, len.data(), count * 8, hipMemcpyHostToDevice, st));
        if (per_inst) ZG_HIP(hipMemcpyAsync((void*)a.inst, inst.data(), inst.size() * sizeof(Fe), hipMemcpyHostToDevice, st));
        ZG_HIP(hipMemcpyAsync((void*)a.rb, rb.data(), count * sizeof(Fe), hipMemcpyHostToDevice, st));
        if (blake2b) {
            ZG_HIP(hipMemcpyAsync(a.enc, enc.data(), enc.size(), hipMemcpyHostToDevice, st));
            ZG_TRY(g1_decompress_dev(ctx, a.enc, count * a.NP, a.pts, a.pvalid));
            ZG_LAUNCH(ctx, "verify_replay", (double)total, verify_replay<Blake2bWalk>, dim3((uint32_t)count), dim3(64), 0, a);
        } else {
            ZG_LAUNCH(ctx, "verify_replay", (double)total, verify_replay<KeccakWalk>, dim3((uint32_t)count), dim3(64), 0, a);
        }
        ZG_LAUNCH(ctx, "verify_scalars", (double)count * a.NE * 32, verify_scalars, dim3((uint32_t)count), dim3(64), 0, a);
        ZG_LAUNCH(ctx, "verify_terms", (double)count * a.NT * 96, verify_terms, dim3((uint32_t)count), dim3(TERMS_WG), 0, a);
        ZG_LAUNCH(ctx, "verify_fold", (double)count * 256, verify_fold, dim3(1), dim3(TERMS_WG), 0, a);
        ZG_HIP(hipGetLastError());
        ZG_HIP(hipMemcpyAsync(status.data(), a.status, count * sizeof(int), hipMemcpyDeviceToHost, st));
        ZG_HIP(hipMemcpyAsync(wpair.data(), a.wpair, 2 * count * sizeof(XYZZ), hipMemcpyDeviceToHost, st));
        ZG_HIP(hipMemcpyAsync(acc, a.out, sizeof(acc), hipMemcpyDeviceToHost, st));
        ZG_HIP(hipStreamSynchronize(st));
    }

    // e(L, [s]_2) e(-R, [1]_2) = 1 over a set of proofs, from their weighted pairs
    const zg_g2_affine q[2] = {v->s_g2, v->g2};
    auto holds = [&](const XYZZ& l, const XYZZ& r) {
        const Affine ps[2] = {xyzz_to_affine(l), affine_neg(xyzz_to_affine(r))};
        return pairing_product_is_one(ps, q, 2);
    };
    std::vector<size_t> live;
    for (size_t b = 0; b < count; b++) {
        verdicts[b] = status[b];
        if (status[b] == ST_OK) live.push_back(b);
    }
    if (live.empty() || holds(acc[0], acc[1])) return ZG_OK;
    // The batch fails: bisect.  A range that is known to fail is split; a half whose weighted sum holds is accepted
    // (with the CSPRNG weights a failing proof cannot be cancelled by the others but with probability ~2^-254, the
    // batch check's own soundness); a failing range of one proof is rejected -- r_b != 0, so that is the lone check.
    // k bad proofs among n cost about k log2(n) pairings instead of n.
    auto range_holds = [&](size_t lo, size_t hi) {
        XYZZ l = xyzz_identity(), r = xyzz_identity();
        for (size_t i = lo; i < hi; i++) {
            l = xyzz_add(l, wpair[2 * live[i]]);
            r = xyzz_add(r, wpair[2 * live[i] + 1]);
        }
        return holds(l, r);
    };
    std::vector<std::pair<size_t, size_t>> failing = {{0, live.size()}};
    while (!failing.empty()) {
        const auto [lo, hi] = failing.back();
        failing.pop_back();
        if (hi - lo == 1) {
            verdicts[live[lo]] = 0;
            continue;
        }
        const size_t mid = lo + (hi - lo) / 2;
        if (range_holds(lo, mid)) {
            failing.push_back({mid, hi});  // (the whole fails and this half holds: the other half fails)
        } else {
            failing.push_back({lo, mid});
            if (!range_holds(mid, hi)) failing.push_back({mid, hi});
        }
    }
    return ZG_OK;
}

int zg_verifier_verify_multi(zg_verifier* v, size_t count, size_t circuits, const uint8_t* const* proofs, const size_t* proof_lens,
                             const zg_fr* const* instance, size_t instance_len, const uint8_t key[32], int* verdicts) {
    return verify_multi_impl(false, v, count, circuits, proofs, proof_lens, instance, instance_len, key, verdicts);
}

int zg_verifier_verify_circuits(zg_verifier* v, size_t count, size_t circuits, const uint8_t* const* proofs, const size_t* proof_lens,
                                const zg_fr* const* instance, size_t instance_len, const uint8_t key[32], int* verdicts) {
    return verify_multi_impl(true, v, count, circuits, proofs, proof_lens, instance, instance_len, key, verdicts);
}

}  // extern "C"
