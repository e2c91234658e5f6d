// The prover object and its proving key, as the files that work on a prover see them: prover.hip (the object and its key),
// prove_batch.hip (create_proof), shard.hip (point-range shards), check.hip and witness.hip.  Internal: nothing here is ABI.
#pragma once

#include <memory>

#include "poly.h"
#include "check.h"
#include "proof_layout.h"

namespace zg {

// The layout of a proof of N circuits under one multi-open argument (proof_layout.h) in the prover's device list
// formats.  The prover's handle of a commitment is its polynomial index (zg_prover::ix_*; `circuit << 16 | index` in a
// proof of several circuits), of a layout point its number as the ProofConst::points slot.  Made at the first proof that
// needs it (ProveBatch::opening_plan) and kept as long as the slots.
struct OpenPlan {
    ProofLayout lay;
    // evaluation e of the layout lands in row ev_row[e] of the slots' evaluations (its circuit's; the proof's own slot when
    // N = 1) at place ev_at[e]: transcript order, or (N > 1) a circuit's n_per own evaluations in every row and behind
    // them, in row 0 only, what the proof holds once: fixed, random, sigma, h
    std::vector<uint32_t> ev_row, ev_at;
    uint32_t n_per = 0, n_row = 0, distinct_polys = 0;
    std::vector<uint32_t> idx;  // poly_dot's lists: the polynomials of a row's n_row places, their point slots behind them
    std::vector<uint32_t> slots;  // 0 .. points: the slot of every opening point, for the Kate divisions
    // GWC: point set s opens the entries lists[firsts[s] .. + counts[s]) (N = 1: 512 entries apart)
    // SHPLONK: per point r of T the commitments of every set that holds r, then (list T) every commitment once for L,
    // then the place of h1's coefficient; set_mask[i]: the points of rotation set i
    std::vector<uint32_t> lists, firsts, counts, com_entry, set_mask;
    size_t sh_ncoef = 0;  // coefficients per proof (both halves use [0, ..))
};

// ------------------------------------------------------------------ proving key on the device
// What keygen_pk derives, resident in HBM, shared (read-only) by every prover forked from the one that built it.
struct PkDev {
    int device = 0;
    uint32_t k = 0, ext_k = 0, cs_degree = 0, bf = 0, qpd = 0;
    uint32_t n = 0, en = 0, usable = 0;
    uint32_t F = 0, A = 0, I = 0, P = 0, NL = 0, sets = 0, chunk = 0;
    // Challenges (Expression::Challenge, ZG_CHALLENGE queries): challenge j is the instance-like column IU + j of a proof,
    // the constant polynomial -- I = IU + NC counts them, IU is the caller's n_instance: what is hashed and uploaded.  The
    // circuit image on the device names that column in the query's place; q_chal says which queries were challenges
    // (ConstraintSystem::degree counts them as degree 0: classify_terms).
    uint32_t IU = 0, NC = 0;
    std::vector<uint8_t> q_chal;
    // The shuffle arguments (zg_prover_create_shuffles): NS of them, each a DLookup whose `tables` are
    // the shuffle expressions, on the host and on the device.  Shuffle j's product z_j is polynomial ix_sz + j of a proof
    // and coset slab A + I + sets + 3 NL + j.
    uint32_t NS = 0;
    std::vector<DLookup> shuffles;
    const DLookup* d_shuffles = nullptr;
    std::vector<zg_query> advice_queries, fixed_queries;
    DevCircuit dc{};
    std::vector<void*> owned;  // device allocations freed with the key
    // evaluate_h on nine 29-bit limbs: the coset slabs, l-polynomials, t_eval and the monomial coefficients it
    // reads are kept in the 2^261 Montgomery form (x * 2^5 of the library form); ZG_EVALH9=0 turns it off
    bool hat = true;
    bool grouped = true;  // the terms after the gates are weighted by powers of y and summed per l-polynomial (ZG_EVALH_GROUPED)
    DMono* monos_hat = nullptr;
    zg_poly* gates_hat = nullptr;
    uint32_t* gate_common = nullptr;
    zg_poly* gate_uni = nullptr;
    Fe* uni_coef = nullptr;
    uint32_t* gate_slab = nullptr;  // per gate: index of its U(fixed cell) coset in gate_slabs, or 0xffffffff
    struct SlabJob { uint32_t gate, query, first, count; };
    std::vector<SlabJob> slab_jobs;  // filled when the gates are factored, run once the fixed cosets exist
    Fe vk_repr{};
    Fe omega{}, omega_inv{}, ifft_div{}, delta_inv{};
    // g_coset, the generator of the extended coset: the creating context's at zg_prover_create* (zg_ctx_set_coset_generator),
    // a primitive cube root of unity -- so zeta^2 = zeta^-1 is the other one.  "zeta" below and in the kernels is THIS value.
    Fe zeta{};
    Fe shift(int zpow) const { return zpow == 1 ? zeta : Fr::sqr(zeta); }  // zeta^zpow, zpow = 1 or 2
    Fe *fixed_val = nullptr, *sigma_val = nullptr, *omega_tw = nullptr;
    Fe* sh_polys = nullptr;  // coefficient forms [F + P][n]: fixed, then sigma
    // The extended domain evaluate_h works on.  Either EvaluationDomain's own coset zeta * <omega_(2^ext_k)> (8n points
    // for degree 6), or -- split -- two cosets that together hold just the (degree - 1) * n points the quotient needs:
    // zeta * <omega_(m1 n)> and zeta^2 * <omega_(m2 n)>, m1 + m2 = degree - 1 (4n + n).  Every coset slab exists per part;
    // the second part is there for the terms of degree > m1 + 1 only (QTerms below): the others' share of the quotient has
    // degree < m1 n and the first part fixes it alone, so a witness polynomial no high term reads is not transformed there.
    struct Dom {
        uint32_t ek = 0, en = 0;
        int zpow = 1;  // the coset shift is zeta^zpow
        // sigma_sc: sigma_cos' column col times (delta^col zeta^zpow)^-1, what evaluate_h's scaled permutation term reads
        // in sigma_cos' place (evalh_perm_scaled; null otherwise)
        Fe *fixed_cos = nullptr, *sigma_cos = nullptr, *sigma_sc = nullptr, *l0 = nullptr, *llast = nullptr, *lactive = nullptr,
           *gate_slabs = nullptr, *t_eval = nullptr, *ext_tw = nullptr;
    };
    Dom dom[3];           // [0]: the single coset; [1], [2]: the two parts of the split domain (when it applies)
    uint32_t nparts = 1;  // 1, or 3 when the split domain is prepared too
    uint32_t NG = 0;
    // The quotient's terms by degree, as ConstraintSystem::degree counts them (classify_terms, prover.hip): a term of
    // degree <= m1 + 1 is low, the others high.  `active`: the key has a split domain, at least one low term, and
    // ProofConst::eh_ypow holds the powers of y the gates' weights need -- the quotient may then take the high terms
    // alone on the second part (ProveBatch::quotient_queue).
    struct QTerms {
        bool active = false;
        std::vector<uint8_t> gate_hi, set_hi, lk_hi;  // per gate / permutation set (product term) / lookup (product term)
        std::vector<uint8_t> part2;                   // per coset slab of a proof (zg_prover::ncos): a high term reads it
        uint32_t* gate_cls = nullptr;                 // EvalHArgs::gate_cls, on the device
        uint32_t tail_lo = 0, tail_hi = 0, set_mask = 0;
        uint64_t lk_mask = 0;
    } qt;
    CheckInfo ck;        // the witness check's share of the key (check.hip): made at the first zg_prover_check_*
    ~PkDev() {
        (void)hipSetDevice(device);
        for (void* q : owned) (void)hipFree(q);
    }
};

inline ProofShape proof_shape(const PkDev& k) {
    ProofShape s;
    s.A = k.A; s.F = k.F; s.P = k.P; s.NL = k.NL; s.sets = k.sets; s.qpd = k.qpd; s.bf = k.bf; s.log_n = k.k;
    s.NS = k.NS;
    for (const zg_query& q : k.advice_queries) s.advice_queries.push_back({q.column, q.rotation});
    for (const zg_query& q : k.fixed_queries) s.fixed_queries.push_back({q.column, q.rotation});
    return s;
}


// ------------------------------------------------------------------ the prover's pinned arena
// ONE block of coherent, mapped host memory that kernels write and the host reads right after an event (alloc_slots), in
// this order: the commitments of a phase (128 B each), the evaluations and behind them the lookups' error words, the
// staging range for small host->device transfers (a bump allocator, reset at the start of every batch), and a zeroed
// margin of 4096 bytes whose last 128 hold the gate words.
struct PinnedArena {
    static constexpr size_t MARGIN = 4096;
    char* host = nullptr;
    char* dev = nullptr;  // the same memory as the device addresses it (hipHostGetDevicePointer)
    size_t cap = 0, evals_at = 0, errors_at = 0, stage_begin = 0;
    size_t stage_at = 0;  // the staging range's bump pointer
    template <class T>
    T* dev_view(T* h) const { return reinterpret_cast<T*>(dev + ((const char*)h - host)); }
    XYZZ* results() const { return reinterpret_cast<XYZZ*>(host); }
    Fe* evals() const { return reinterpret_cast<Fe*>(host + evals_at); }
    uint32_t* lookup_errors() const { return reinterpret_cast<uint32_t*>(host + errors_at); }
    size_t stage_end() const { return cap - MARGIN; }
    void stage_reset() { stage_at = stage_begin; }
    bool stage_has(size_t bytes) const { return stage_at + bytes <= stage_end(); }
    void* stage_take(size_t bytes) {  // 64-byte aligned; nullptr when the range is full
        const size_t off = (stage_at + 63) & ~size_t(63);
        if (off + bytes > stage_end()) return nullptr;
        stage_at = off + bytes;
        return host + off;
    }
    // gate_word()[0] = the last gate opened (a sequence number); gave_up_word() = the gate that gave up waiting, if any
    uint32_t* gate_word() const { return reinterpret_cast<uint32_t*>(host + cap - 128); }
    uint32_t* gave_up_word() const { return gate_word() + 16; }
};

}  // namespace zg

// ------------------------------------------------------------------ prover object
// One context (stream + workspace), one proving key (possibly shared), `cap` proof slots: every per-proof buffer is
// [cap] x its single-proof size, proof-major, so that one launch serves every proof of a lock-step batch.
struct zg_prover {
    zg_ctx* ctx = nullptr;
    std::shared_ptr<zg::PkDev> pk;
    zg_bases *g = nullptr, *gl = nullptr;
    // base tables the prover registered itself (zg_prover_create): owned jointly with its forks, freed with the last
    // of them; null when the caller registered the tables (zg_prover_create_shared) and keeps them alive
    struct OwnedBases {
        zg_bases *g = nullptr, *gl = nullptr;
        ~OwnedBases() {
            if (g) zg_bases_free(g);
            if (gl) zg_bases_free(gl);
        }
    };
    std::shared_ptr<OwnedBases> owned_bases;
    bool use_side = true;   // coefficient / coset forms on a side stream (latency) or inline (throughput)
    // what a LONE proof (latency form) borrows from the throughput form once the circuit is large enough for the work
    // to outweigh the launches (from k: K_LAT_SPLIT_K)
    bool lat_split = false;
    uint32_t naf_gl_w = 0;  // digit width of the run-form commitments' free-position form, 0 = windows (naf_gl_default)
    // point-range shard of the commitments (zg_prover_set_shard): this prover's base sets hold points
    // [shard_lo, shard_lo + shard_n) of the SRS; partial commitments of all ranks are exchanged and summed
    uint32_t shard_lo = 0, shard_n = 0, world = 1, rank = 0;
    zg_exchange_fn exchange = nullptr;
    void* exchange_user = nullptr;
    // ... or, with a communicator of the collective library (zg_prover_set_shard_rccl), all-gathered and summed on the
    // device: the phase's partial sums never visit the host before they are whole
    void* rccl_comm = nullptr;
    zg::XYZZ* gathered = nullptr;  // [world][maxv * cap]
    size_t gathered_cap = 0;   // the slot count it is sized for (zg_prover_set_batch regrows it)
    // per-proof buffers, [cap] slots each (alloc_slots)
    uint32_t cap = 0;
    std::vector<void*> slot_owned;
    uint32_t npp = 0;  // per-proof coefficient polynomials: advice, instance, perm z, lookup z, a'/s', random, h pieces, h
    uint32_t ncos = 0; // per-proof coset slabs: advice, instance, perm z, lookup z, a'/s'
    // indices into the coefficient-polynomial space (PolySet: < nsh = F + P shared, the rest per proof)
    uint32_t ix_fixed = 0, ix_sigma = 0, ix_adv = 0, ix_inst = 0, ix_pz = 0, ix_lz = 0, ix_perm = 0, ix_random = 0,
             ix_hpiece = 0, ix_hpoly = 0, nsh = 0;
    uint32_t ix_sz = 0;  // the shuffle products: behind a'/s' among the polynomials and among the coset slabs
    // the shuffle products' rows [cap][NS][n], their grand product's terms [cap * NS][n] each and its scratch
    zg::Fe *sz = nullptr, *snum = nullptr, *sden = nullptr, *stmp = nullptr;
    zg::Fe* pp = nullptr;  // [cap][npp][n]
    struct DomBuf {
        zg::Fe *cos = nullptr /* [cap][ncos][en] */, *h = nullptr /* [cap][en] */;
    };
    DomBuf dbuf[3];
    zg::Fe* split_tmp = nullptr;  // [cap][3 * dom[2].en]
    zg::Fe* h_hi = nullptr;       // the high terms' quotient on the first part (pk->qt.active): [cap][dom[1].en]
    bool qterms = true;  // zg_prover_set_quotient_terms: 0 = every term on both parts, as without low terms
    zg::Fe *adv_val = nullptr /* [cap][A][n] */, *inst_val = nullptr /* [cap][I][n] */;
    zg::Fe *cin = nullptr, *ctab = nullptr /* [cap * NL][n] each */, *perm = nullptr /* [cap][2NL + 1][n]: a'_l, s'_l, random */,
       *zs = nullptr /* [cap][S + NL + 1][n] */;
    zg::Fe *num = nullptr, *den = nullptr, *tmp = nullptr, *pw = nullptr, *wpoly = nullptr, *raw = nullptr,
       *sraw = nullptr, *sort_fe = nullptr, *ktmp = nullptr;
    uint32_t *sort_u32 = nullptr, *d_err = nullptr;
    zg::XYZZ* xyzz = nullptr;
    uint32_t maxv = 0, max_points = 0, max_evals = 0;
    zg::ProofConst* d_pc = nullptr;
    std::vector<zg::ProofConst> hpc;
    uint32_t* d_idx = nullptr;  // index lists (circuit only: the same for every proof)
    // a proof of several circuits: its opening lists over (slot, polynomial) pairs, sized for `cap` circuits
    uint32_t* d_mlists = nullptr;
    size_t mlists_cap = 0;
    // The multi-open argument (zg_prover_set_multiopen): GWC, or SHPLONK with its own buffers (alloc_slots, sized with the
    // slots): h1 [cap][n], the two combinations' index lists, their per-proof coefficients (unpacked nine-limb values) and
    // the interpolants' low coefficients
    int multiopen = 0;
    int transcript = 0;  // zg_prover_set_transcript: ZG_TRANSCRIPT_EVM, or halo2's Blake2b transcript with compressed points
    // zg_prover_set_phases: the phase of every advice column (empty: one phase) and of every challenge squeezed (at least
    // pk->NC of them; only the first pk->NC have a pseudo-column)
    std::vector<uint8_t> advice_phase, challenge_phase;
    uint32_t n_phases = 1;
    zg::Fe* d_chal = nullptr;  // [cap][NC][2]: a challenge as its value / coefficient rows hold it, and as its coset slabs do
    bool phased() const { return n_phases > 1 || !challenge_phase.empty(); }
    zg::Fe* sh_h1 = nullptr;
    uint32_t* sh_lists = nullptr;
    zg::F9* sh_coef = nullptr;
    zg::Fe* sh_corr = nullptr;
    size_t sh_terms = 0;  // opening queries of `cap` circuits: sh_lists holds 2 * sh_terms + 16 entries, sh_coef sh_terms + cap + 16
    std::map<uint32_t*, std::vector<uint32_t>> uploaded_lists;  // what h2d_list left at each destination
    std::map<std::pair<int, uint32_t>, zg::OpenPlan> plans;     // by (multi-open argument, circuits in a proof)
    std::vector<size_t> inst_filled;  // per slot: rows of inst_val that may be non-zero
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_err = nullptr;
    // One event per WAIT of a proof (the five commitment phases and the evaluations): with the gate (below) the next phase's
    // launches -- and its commit's event record -- are queued before the host waits for this one, so they cannot share one.
    static constexpr int N_WAITS = 6;
    hipEvent_t evs[N_WAITS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // The gate of a lone proof (ZG_LAT_GATE, ProveBatch::run): a word of the pinned arena that gate_pull_kernel polls and
    // the host writes once the next challenge is staged -- the next phase is then already in the queue behind that kernel.
    // (PinnedArena::gate_word / gave_up_word)
    uint32_t gate_seq = 0;
    // (what the last COMPLETED proof looked like -- ProveBatch::form_sig: a first proof in a form creates twiddle tables
    //  and workspace, with stream synchronisations the gate must not stand in front of; only a repeat is gated)
    uint64_t warm_sig = 0;
    uint64_t gate_stats[4] = {0, 0, 0, 0};  // zg_prover_gate_stats
    zg::PinnedArena pin;
    bool have_last = false;
    bool in_flight = false;   // a batch was started and did not reach its end (an error return): work may still be queued
    bool last_split = false;  // which extended domain the last proof used (zg_prover_fetch)
    bool last_by_degree = false;  // ... and whether it took the quotient's terms by degree (the first part's h is reused then)
    uint32_t last_nb = 0;
    double phase_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace zg {

int prover_drain(zg_prover* p);  // waits for everything queued on the prover's streams
// what zg_prover_prove* and zg_prover_check* ask of a batch's arguments (who: the entry's name, what: "proofs" / "witnesses")
int batch_args_ok(const char* who, const char* what, const zg_prover* p, size_t count, const zg_fr* const* instance, size_t instance_len);
// advice columns of a batch into the prover's slots: host columns are uploaded, foreign device columns copied, a slot that
// already holds its columns (zg_prover_advice_slot) is left alone
int advice_into_slots(zg_prover* p, uint32_t nb, const zg_fr* const* advice_host, void* const* advice_dev);
// the per-proof scalars of the batch, as the host holds them now, to the device (prove_batch.hip: through the staging arena)
int upload_consts(zg_prover* p, uint32_t nb);
// evaluate_h's host side (prover.hip)
uint32_t evalh_terms(const PkDev& pk);
bool evalh_perm_scaled(const PkDev& pk);  // the key holds sigma_sc and ProofConst has room for the circuit's columns
void evalh_consts(ProofConst& c, const Fe& y, const PkDev& pk);
EvalHArgs evalh_args(const zg_prover* p, uint32_t di);
// shard.hip: ONE all-gather of a phase's partial sums (p->xyzz) over the prover's communicator, then the additions into `out`
int shard_gather_sum(zg_prover* p, size_t count, XYZZ* out);

}  // namespace zg
