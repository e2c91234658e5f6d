// create_proof for one circuit instance on one MI355X -- replaces
// halo2_proofs::plonk::create_proof::<KZGCommitmentScheme<Bn256>, ProverGWC, _, _, EvmTranscript, _>
// as Wnn::proof calls it (/root/reference/src/wnn.rs:232-262; upstream v2023_04_20 src/plonk/prover.rs).
//
// Proofs are made in lock-step batches: one launch sequence serves `nb` circuit instances at once (a single proof
// is the batch of one), each with its own Fiat-Shamir transcript on the host.
//
// Everything between "advice columns assigned" and "proof bytes" stays in HBM: columns, coefficient
// forms, extended cosets, lookup/permutation products, h(X).  The host only sees what the Fiat-Shamir
// transcript needs -- commitments (one 128-B XYZZ point each), evaluations (32 B each).  Even
// lookup::prover::permute_expression_pair (a sort + BTreeMap walk upstream) runs on the device
// (sort.hip).  Work that does not depend on the next challenge (iNTTs, coset NTTs) runs on a side
// stream while the main stream works through the commitment MSM and the host hashes.
#include <algorithm>
#include <chrono>
#include <map>

#include "prover.h"
#include "field9.h"
#include "transcript.h"

using namespace zg;

namespace {

Fe rotate_omega(const PkDev& k, const Fe& x, int32_t rot) {
    Fe w = rot >= 0 ? Fr::pow_u64(k.omega, (uint64_t)rot) : Fr::pow_u64(k.omega_inv, (uint64_t)(-(int64_t)rot));
    return Fr::mul(x, w);
}

// ZG_LAT_GATE (ProveBatch::run).  OFF unless asked for: a kernel that waits for the host is only safe while every stream
// of the process has a hardware queue of its own (GPU_MAX_HW_QUEUES, default 4): packets of streams that share a queue
// run in order, so this prover's side stream -- which the host waits for before it opens the next gate -- may sit behind
// another stream's wait for work that itself sits behind the gate.  The kernel's time limit turns that cycle into a
// stall and a second, plain run of the proof (prove_batch_impl), never into a hang or a wrong proof.
constexpr int LAT_GATE_DEFAULT = 0;
constexpr int LAT_PULL_DEFAULT = 1;  // (ZG_LAT_PULL: a lone proof's small uploads by a one-wave kernel instead of a copy command)
// Small host->device transfers go through the staging range of the pinned arena (PinnedArena): hipMemcpyAsync from
// pageable memory blocks the calling thread until the stream has drained up to the copy, which serialises host and
// GPU inside a proof and throttles concurrent proof streams.  Each region is written once per batch.
void* stage(zg_prover* p, const void* src, size_t bytes) {
    void* dst = p->pin.stage_take(bytes);
    if (dst) memcpy(dst, src, bytes);
    return dst;  // (nullptr: the caller falls back to a direct copy)
}
// Index lists that only depend on the circuit (which polynomial is opened where) come out the same for every
// proof: upload one when its content differs from what that destination already holds.
int h2d_list(zg_prover* p, uint32_t* d_dst, const std::vector<uint32_t>& list) {
    std::vector<uint32_t>& held = p->uploaded_lists[d_dst];
    if (held == list) return ZG_OK;
    const void* s = stage(p, list.data(), list.size() * 4);
    ZG_HIP(hipMemcpyAsync(d_dst, s ? s : list.data(), list.size() * 4, hipMemcpyHostToDevice, p->ctx->stream));
    if (!s) ZG_HIP(hipStreamSynchronize(p->ctx->stream));  // (the source was pageable memory of the caller)
    held = list;
    return ZG_OK;
}
// (a lone proof's version of a small upload: ONE wave reads the staged bytes through the device's view of the pinned arena
//  and writes them where they go -- a kernel dispatch instead of a copy command behind every transcript step)
__global__ void pull_kernel(const uint4* __restrict__ src_mapped, uint4* __restrict__ dst, uint32_t n16) {
    for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src_mapped[i];
}
// The gate: ONE workgroup that waits until the host has written `seq` into the gate word (mapped, coherent host memory),
// then copies the scalars the host staged BEFORE that store to where the kernels read them -- wait and upload in one
// dispatch.  (hipStreamWaitValue32 + pull_kernel, the first version, were two: on this runtime the stream wait is itself
// a spinning kernel, __amd_rocclr_streamOpsWait.)  Every wave reaches the end: a gate nobody opens within `max_ticks` of
// the 100 MHz clock gives up, says so in *gave_up (the host then fails the proof) and leaves dst alone.
__global__ void gate_pull_kernel(const uint32_t* gate, uint32_t seq, uint32_t* gave_up, uint64_t max_ticks, const uint4* __restrict__ src_mapped,
                                 uint4* __restrict__ dst, uint32_t n16) {
    __shared__ uint32_t open;
    if (threadIdx.x == 0) {
        const uint64_t t0 = wall_clock64();
        uint32_t got = 1;
        // (open at `seq` OR LATER, in the sequence numbers' modular order: where nothing stands between two gates -- a circuit
        //  without lookups or permutation queues nothing behind theta and needs no device result before beta -- the host may
        //  have opened the NEXT gate before this kernel's first look at the word)
        while ((int32_t)(__hip_atomic_load(gate, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - seq) < 0) {
            if (wall_clock64() - t0 > max_ticks) {
                got = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!got) __hip_atomic_store(gave_up, seq | 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);  // (any non-zero word)
        open = got;
    }
    __syncthreads();
    if (!open) return;
    for (uint32_t i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src_mapped[i];
}
constexpr uint64_t GATE_MAX_TICKS = 400000000ull;  // 4 s: a host thread that is merely descheduled comes back sooner
int h2d(zg_prover* p, void* d_dst, const void* src, size_t bytes) {
    const void* s = stage(p, src, bytes);
    const int pull = knob(K_LAT_PULL);
    if (s && p->use_side && (pull < 0 ? LAT_PULL_DEFAULT : pull) != 0 && bytes % 16 == 0 && bytes <= (1u << 16) && ((uintptr_t)d_dst & 15u) == 0) {
        const uint4* dev_view = p->pin.dev_view(reinterpret_cast<const uint4*>(s));
        ZG_LAUNCH(p->ctx, "pull", (double)bytes * 2, pull_kernel, dim3(1), dim3(256), 0, dev_view, (uint4*)d_dst, (uint32_t)(bytes / 16));
        ZG_HIP(hipGetLastError());
        return ZG_OK;
    }
    ZG_HIP(hipMemcpyAsync(d_dst, s ? s : src, bytes, hipMemcpyHostToDevice, p->ctx->stream));
    if (!s) ZG_HIP(hipStreamSynchronize(p->ctx->stream));
    return ZG_OK;
}
// the bit-position table of a base set for the throughput form's commitments of full-size scalars (the sorted a' / s'
// columns and the products in their run form, the random vectors), else the base set itself
// (a lone proof keeps the window tables: from the 0.27 GB bit-position table, which no cache holds, its few waves wait on
//  the gathers -- 3.27 against 3.01 ms with the same bucket count)
static const zg_bases* naf_of(const zg_prover* p, const zg_bases* b) {
    const zg_bases* d = bases_dense(b);
    return d && d->naf_w && !p->ctx->msm_pair ? d : b;
}

// the table of g for the all-random commitments (the quotient pieces, the opening quotients): its bit-position table in
// the throughput form, recoded at the width the table was made for
static const zg_bases* dense_g(const zg_prover* p) { return naf_of(p, p->g); }

// Commitments of a phase: one MSM launch sequence over m.batch = groups x per scalar vectors (msm_dev), against this
// prover's point range of the base sets; the XYZZ results go to the host behind it.
// (out_at, last: a phase made of several launch sequences -- the runs of an advice phase's columns -- leaves sequence
//  after sequence in the results and records the event behind the last)
int commit(zg_prover* p, MsmJob m, int wait_ix, size_t out_at = 0, bool last = true) {
    ZG_REQUIRE(out_at + m.batch <= p->maxv * (size_t)p->cap, ZG_ERR_INVALID_ARG, "zg_prover: %zu commitments in one phase", out_at + m.batch);
    ZG_REQUIRE(out_at == 0 || !p->rccl_comm, ZG_ERR_UNSUPPORTED, "zg_prover: advice phases on a point-range shard");
    // The last kernel of the MSM writes its sums straight into the pinned host buffer the transcript reads (the memory is
    // mapped into the device's address space): no copy command between the MSM and the host -- a command costs a lone
    // proof its dispatch latency on top of its run time, ~9 us per commitment phase.  Only the in-library RCCL exchange
    // keeps the sums on the device (all-gather and the additions follow on this stream) and copies the result out.
    XYZZ* h_out = p->pin.dev_view(p->pin.results()) + out_at;
    m.scalars += p->shard_lo;
    m.n = p->shard_n;
    m.out = p->rccl_comm ? p->xyzz : h_out;
    ZG_TRY(msm_dev(p->ctx, m));
    if (p->rccl_comm) ZG_TRY(shard_gather_sum(p, m.batch, h_out));  // (over xGMI, on this stream)
    if (last) ZG_HIP(hipEventRecord(p->evs[wait_ix], p->ctx->stream));
    return ZG_OK;
}
// ... and waits for ONLY that launch sequence; with a sharded SRS the partial commitments of all ranks are exchanged
// (all-gather) and summed here -- EC addition is not a reduction operator of the collective library
int wait_points(zg_prover* p, size_t count, std::vector<Jac>& out, int wait_ix) {
    // (hipEventSynchronize already polls: the events are created without hipEventBlockingSync.  A hand-written
    //  hipEventQuery loop in its place never saw the event complete on this runtime -- round 3, gpurun_out/r3_t3.log --
    //  and bought nothing: the wait was never a sleep.)
    ZG_HIP(hipEventSynchronize(p->evs[wait_ix]));
    const XYZZ* local = p->pin.results();
    out.resize(count);
    if (p->world <= 1 || p->rccl_comm) {  // (whole sums already: a lone prover, or gathered and added on the device)
        xyzz_batch_normalise(local, count, reinterpret_cast<zg_g1*>(out.data()));
        return ZG_OK;
    }
    ZG_REQUIRE(p->exchange != nullptr, ZG_ERR_INVALID_ARG, "zg_prover: sharded prover without an exchange function");
    std::vector<XYZZ> all((size_t)p->world * count);
    const int st = p->exchange(p->exchange_user, local, count * sizeof(XYZZ), all.data());
    ZG_REQUIRE(st == 0, ZG_ERR_HIP, "zg_prover: the exchange function failed with %d", st);
    return zg_xyzz_sum_ranks(all.data(), p->world, count, reinterpret_cast<zg_g1*>(out.data()));
}

}  // namespace

// the per-proof scalars of the batch, as the host holds them now, to the device (behind the work already queued)
int zg::upload_consts(zg_prover* p, uint32_t nb) { return h2d(p, p->d_pc, p->hpc.data(), (size_t)nb * sizeof(ProofConst)); }

extern "C" {

// create_proof for `nb` circuit instances in lock step: every kernel launch below serves all nb proofs (grid rows /
// vector groups per proof, scalars from d_pc[b]); the host keeps one transcript per proof and hands each its own
// challenges.  nb = 1 is the single-proof path (zg_prover_prove / _dev): there is no other.
// advice_host / advice_dev: per proof, one of them may be given (host columns are uploaded, foreign device columns
// copied into the proof's slot); both null = the slot already holds the columns (zg_prover_advice_slot).
// Host-side timeline of a batch (development aid, compiled in with -DZG_TICKS: `make EXTRA=-DZG_TICKS`): every ZG_TICK
// records a label and the time since the batch began; the list goes to stderr when the batch is done.
#ifdef ZG_TICKS
struct TickLog {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<std::pair<const char*, double>> v;
    void tick(const char* l) { v.emplace_back(l, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count()); }
    ~TickLog() {
        double prev = 0;
        for (auto& e : v) {
            fprintf(stderr, "tick %9.1f us  +%7.1f  %s\n", e.second, e.second - prev, e.first);
            prev = e.second;
        }
    }
};
#define ZG_TICK(l) ticks.tick(l)
#else
#define ZG_TICK(l) ((void)0)
#endif

// One lock-step batch of create_proofs (upstream plonk/prover.rs, `create_proof`): the state its phases share, and ONE member
// function per phase -- round 3 had all of it in a single 510-line function.  A phase queues its kernels
// on the prover's stream(s), waits for what the transcript needs (commitments as points, evaluations), feeds every proof's
// EvmTranscript and leaves the next challenges in p->hpc[] / on the device (upload_consts).  Order and contents of the phases
// are upstream's:
//   load_inputs        instance + advice columns in place, blinding rows, the vanishing argument's random polynomial
//   commit_advice      advice commitments, phase by phase with the phase's challenges behind each (zg_prover_set_phases;
//                      one phase and no challenge unless the circuit says otherwise)   -> theta
//   commit_permuted    lookup::commit_permuted (+ the random polynomial)    -> beta, gamma
//   commit_products    permutation::commit, lookup::commit_product          -> y
//   opening_plan       (no device work) which polynomial is evaluated and opened where: proof_layout.h's order of the
//                      proof in this prover's list formats, made once per prover, argument and circuits in a proof
//   quotient           evaluate_h, h(X) in pieces, their commitments        -> x
//   evaluations        eval_polynomial at x omega^rot                       -> v
//   openings           ProverGWC::create_proof, or ProverSHPLONK's (shplonk_*)
//   finish             proof bytes and statuses out
// A nonzero return leaves p->in_flight set: the next batch drains the streams before it reuses the slots.
struct ProveBatch {
    using clk = std::chrono::steady_clock;
    // ---- the call
    zg_prover* p;
    const zg_fr* const* advice_host;
    void* const* advice_dev;
    const zg_fr* const* instance;
    size_t instance_len;
    const uint8_t* keys;
    uint8_t* const* proofs;
    size_t proof_cap;
    size_t* proof_lens;
    int* statuses;
    // zg_prover_prove_phased: the caller's witness synthesis, called at the head of every advice phase
    zg_phase_fn phase_fn = nullptr;
    void* phase_user = nullptr;
    // ---- shapes
    const PkDev& pk;
    zg_ctx* ctx;
    hipStream_t st;
    uint32_t nb, n, k, ek, bf, usable, A, I, P, NL, S, Q;
    uint32_t NS;  // shuffle arguments (PkDev::NS)
    uint32_t IU, NC;  // (I = IU + NC: the caller's instance columns, then the challenges' constant columns -- PkDev::NC)
    // the challenges squeezed so far, [nb][nch] (zero where not yet squeezed): what a phase's callback is handed
    uint32_t nch;
    std::vector<zg_fr> chal;
    std::vector<Fe> chal_vals;
    // A proof of SEVERAL circuit instances (create_proof's `circuits` slice, zg_prover_prove_multi): the nb slots are the
    // circuits and there is ONE transcript, tr[0]; after every squeeze the same challenges go into every slot's scalars.
    // The slots meet in three places: the transcript's order (the absorb halves), the quotient (fold_quotients: one h,
    // one set of pieces) and the multiopen argument (lists over (circuit, polynomial) pairs, one W per point set).
    // What the proof holds once -- h and its pieces, the openings -- is computed for `nq` = 1 slot, and `ntr` = 1.
    bool multi = false;
    uint32_t ntr, nq;
    bool hat;
    bool split;         // extended-domain parts of this proof: the split pair in the throughput configuration, the single coset otherwise
    bool phase_cosets;  // the coset forms of a phase's columns: on the side stream while that phase's commitments run (latency
                        // form), or all at once before evaluate_h (throughput form)
    uint32_t dlo, dhi;
    // The quotient's terms by degree (PkDev::QTerms): the second part of the split domain sees the high terms only -- and
    // only the polynomials they read.  Not for a proof of several circuits, whose slots' quotients are folded per part.
    bool by_degree;
    size_t pp_bs, adv_bs, inst_bs, perm_bs, zs_bs, pw_bs, wp_bs;  // strides between consecutive proofs
    // side stream: coefficient / coset forms of committed columns are computed there while the main stream runs the
    // commitment MSM (p->use_side == false: everything stays on the main stream -- the throughput configuration, where other
    // proofs in flight fill the gaps and every extra HIP stream costs a hardware queue)
    zg_ctx* sx;
    hipStream_t ss;
    double parts_en, ext_unit;  // (profile charges: SURVEY.md 8d counts one coeff_to_extended as (n + 2^ext_k) * 32 B whatever parts it is computed on)
    // ---- state carried from phase to phase
    PolySet polys;
    std::vector<Transcript> tr;  // (EvmTranscript or halo2's Blake2b one: zg_prover_set_transcript)
    std::vector<int> status;
    std::vector<Jac> pts;
    Fe* random_row = nullptr;  // (proof 0's; proof b's is perm_bs further)
    Fe* adv = nullptr;
    Cols base_cols;
    std::vector<Jac> random_commit;
    bool have_random = false;
    const OpenPlan* plan = nullptr;  // which polynomial is evaluated and opened where (opening_plan())
    uint32_t npoints = 0;            // distinct opening points: ProofConst::points slots, GWC's point sets, SHPLONK's T
    uint32_t* d_hlist = nullptr;
    const Fe* ev_all = nullptr;
    uint32_t* h_err = nullptr;  // the lookups' error words on the host
    uint32_t prod_per = 0;      // commitments per proof of the products phase (the random polynomial rides there without lookups)
    // ---- SHPLONK (zg_prover_set_multiopen): per proof what the second half needs of the first
    const bool shplonk;
    struct SProof { Fe y, v; std::vector<std::vector<Fe>> R; };  // R[i]: sum_j y^j R_ij(X), coefficients
    std::vector<SProof> sproof;
    // ---- the gate (run())
    enum Wait { W_ADVICE, W_PERMUTED, W_PRODUCTS, W_QUOTIENT, W_EVALS, W_GWC };
    bool gated = false, armed = false;
    bool no_gate = false;       // (the second run of a proof whose gate gave up)
    bool gate_gave_up = false;  // finish(): a gate kernel ran into its time limit -- the proof was made on stale scalars
    uint32_t gates_armed = 0;
    void* gate_slot = nullptr;
    zg_ctx::GateHold hold;  // what a blocking call inside a queued-ahead phase needs to let the gate go (common.h)
    clk::time_point t_start, t_prev;
#ifdef ZG_TICKS
    TickLog ticks;
#endif

    ProveBatch(zg_prover* p_, size_t count, const zg_fr* const* advice_host_, void* const* advice_dev_, const zg_fr* const* instance_,
               size_t instance_len_, const uint8_t* keys_, uint8_t* const* proofs_, size_t proof_cap_, size_t* proof_lens_, int* statuses_,
               bool multi_ = false)
        : p(p_), advice_host(advice_host_), advice_dev(advice_dev_), instance(instance_), instance_len(instance_len_), keys(keys_),
          proofs(proofs_), proof_cap(proof_cap_), proof_lens(proof_lens_), statuses(statuses_), pk(*p_->pk), ctx(p_->ctx),
          st(p_->ctx->stream), nb((uint32_t)count), multi(multi_), ntr(multi_ ? 1u : (uint32_t)count), nq(ntr), tr(ntr),
          status(count, ZG_OK), shplonk(p_->multiopen == ZG_MULTIOPEN_SHPLONK) {
        n = pk.n; k = pk.k; ek = pk.ext_k; bf = pk.bf; usable = pk.usable;
        A = pk.A; I = pk.I; P = pk.P; NL = pk.NL; S = pk.sets; Q = pk.qpd;
        IU = pk.IU; NC = pk.NC; NS = pk.NS;
        nch = (uint32_t)p->challenge_phase.size();
        chal.assign((size_t)nb * nch, zg_fr{});
        for (Transcript& t : tr) t.blake2b = p->transcript == ZG_TRANSCRIPT_BLAKE2B;
        hat = pk.hat;
        split = pk.nparts == 3 && (!p->use_side || p->lat_split);
        phase_cosets = p->use_side || !split;
        dlo = split ? 1u : 0u;
        dhi = split ? 3u : 1u;
        by_degree = split && pk.qt.active && p->qterms && !multi;
        pp_bs = (size_t)p->npp * n; adv_bs = (size_t)A * n; inst_bs = (size_t)I * n; perm_bs = (size_t)(2 * NL + 1) * n;
        zs_bs = (size_t)(S + NL + 1) * n; pw_bs = (size_t)p->max_points * n; wp_bs = (size_t)2 * p->max_points * n;
        polys.sh = pk.sh_polys; polys.pp = p->pp; polys.nsh = p->nsh; polys.n = n; polys.pp_bs = pp_bs;
        sx = p->use_side ? ctx->side : ctx;
        ss = sx->stream;
        parts_en = 0.0;
        for (uint32_t di = dlo; di < dhi; di++) parts_en += (double)pk.dom[di].en;
        ext_unit = ((double)n + (double)((size_t)1 << ek)) * 32.0;
        t_start = t_prev = clk::now();
    }

    Fe* pp_at(uint32_t ix) const { return p->pp + (size_t)(ix - p->nsh) * n; }  // proof 0's polynomial ix (>= nsh)
    Transcript& T(uint32_t b) { return tr[multi ? 0 : b]; }                     // the transcript slot b writes into
    // a challenge into every slot's scalars: each proof's own, or the one proof's for all its circuits
    void squeeze_into(Fe ProofConst::*field) {
        for (uint32_t b = 0; b < nb; b++) p->hpc[b].*field = b < ntr ? tr[b].squeeze() : p->hpc[0].*field;
    }
    void lap(int slot) {
        auto now = clk::now();
        p->phase_ms[slot] = std::chrono::duration<double, std::milli>(now - t_prev).count();
        t_prev = now;
    }
    int fork() {  // side stream continues after everything queued on the main stream so far
        if (!p->use_side) return ZG_OK;
        ZG_HIP(hipEventRecord(p->ev_fork, st));
        ZG_HIP(hipStreamWaitEvent(ss, p->ev_fork, 0));
        return ZG_OK;
    }
    int join() {  // main stream continues after everything queued on the side stream so far
        if (!p->use_side) return ZG_OK;
        ZG_HIP(hipEventRecord(p->ev_join, ss));
        ZG_HIP(hipStreamWaitEvent(st, p->ev_join, 0));
        return ZG_OK;
    }
    // the commitments of a phase: `per` scalar vectors per proof (`stride` apart, proof b's `outer` after proof b-1's), all
    // against `bases` in their plain form unless the caller says otherwise
    MsmJob phase_msm(const zg_bases* bases, const Fe* scalars, size_t stride, size_t per, size_t outer, uint32_t slots = 0) const {
        MsmJob m;
        m.bases = bases; m.split = per;
        m.scalars = scalars; m.stride = stride; m.per = per; m.outer = outer;
        m.batch = (size_t)(slots ? slots : nb) * per;
        return m;
    }
    // two-level layouts of the transforms: `per` arrays per proof
    static Grouping grouping(uint32_t per, size_t in_outer, size_t out_outer) {
        Grouping g;
        g.per = per; g.in_outer = in_outer; g.out_outer = out_outer;
        return g;
    }
    // coefficient forms (ix0 .. ix0 + per) of every proof -> their slabs on each part of the extended domain
    // (by degree: the second part gets only the polynomials a high term reads -- PkDev::QTerms::part2 -- in runs of
    //  neighbours, each to its own slab; the others' whole unit is then charged to the first part's launch)
    int to_cosets(zg_ctx* c, uint32_t ix0, uint32_t per) {
        const uint8_t* keep = by_degree ? pk.qt.part2.data() + (ix0 - p->ix_adv) : nullptr;
        uint32_t dropped = 0;
        for (uint32_t i = 0; keep && i < per; i++) dropped += keep[i] ? 0u : 1u;
        for (uint32_t di = dlo; di < dhi; di++) {
            const PkDev::Dom& d = pk.dom[di];
            const double share = (double)d.en / parts_en;
            for (uint32_t r0 = 0; r0 < per;) {
                uint32_t r1 = per;
                if (keep && di == 2) {
                    if (!keep[r0]) { r0++; continue; }
                    for (r1 = r0; r1 < per && keep[r1];) r1++;
                }
                const uint32_t cnt = r1 - r0;
                const Grouping g = grouping(cnt, pp_bs, (size_t)p->ncos * d.en);
                c->unit_next = (double)nb * ext_unit * (cnt * share + (keep && di == 1 ? dropped * (1.0 - share) : 0.0));
                ZG_TRY(coeff_to_coset_dev(c, pp_at(ix0 + r0), n, n, p->dbuf[di].cos + (size_t)(ix0 + r0 - p->ix_adv) * d.en, d.en,
                                          (size_t)nb * cnt, d.ek, hat, pk.shift(d.zpow), &g));
                r0 = r1;
            }
        }
        return ZG_OK;
    }

    // The phases of create_proof, each in two halves: X_queue() puts the phase's device work on the streams (it needs only
    // the circuit and what the device already holds -- every challenge reaches the kernels through d_pc), X_absorb() waits
    // for the phase's results, writes them into the transcripts and PUBLISHES the next challenge (publish(): hpc -> d_pc).
    //
    // Plain order: queue, absorb, queue, absorb ...  A lone proof with the gate (ZG_LAT_GATE) queues the NEXT phase before
    // it absorbs this one: arm() reserves a staging slot and puts gate_pull_kernel on the stream (it waits for the gate
    // word, then copies the slot to d_pc), the next phase's launches follow behind it, and publish() fills the slot and
    // opens the gate -- between the host having a challenge and the device using it stands one store, not a launch
    // sequence.  What follows the grand products' totals is never queued ahead: it starts with the HOST inverting them.
    int run() {
        const int st_run = run_phases();
        p->gate_stats[0] += gated ? 1 : 0;
        p->gate_stats[1] += gates_armed;
        p->gate_stats[3] += hold.yields;
        // An error that surfaced BEHIND a failed gate (a time limit, a yield) is the stale scalars' doing, not the caller's:
        // drain what was queued and let prove_batch_impl make the proof again in the plain order.
        if (st_run != ZG_OK && !gate_gave_up && gate_failed()) {
            open_gate();
            (void)prover_drain(p);
            p->in_flight = false;
            gate_gave_up = true;
        }
        if (gate_gave_up) p->gate_stats[2]++;
        if (st_run != ZG_OK) p->warm_sig = 0;  // (whatever way a proof failed: the next one is a first proof)
        return st_run;
    }
    int run_phases() {
        begin();
        ZG_TRY(load_inputs());
        gated = gate_wanted();
        if (p->phased()) ZG_TRY(opening_plan());  // (no device work: the layout states the phases)
        ZG_TRY(advice_queue());
        if (!gated) {
            ZG_TRY(advice_absorb());
            ZG_TRY(permuted_queue());
            ZG_TRY(permuted_absorb());
            ZG_TRY(products_terms_queue());
            ZG_TRY(products_queue());
            ZG_TRY(products_absorb());
            ZG_TRY(opening_plan());
            ZG_TRY(quotient_queue());
            ZG_TRY(quotient_absorb());
            ZG_TRY(evaluations_queue());
            ZG_TRY(evaluations_absorb());
            ZG_TRY(openings_queue());
        } else {
            ZG_TRY(arm());
            ZG_TRY(permuted_queue());    // behind theta
            ZG_TRY(advice_absorb());
            ZG_TRY(arm());
            ZG_TRY(products_terms_queue());  // behind beta, gamma
            ZG_TRY(permuted_absorb());
            ZG_TRY(products_queue());  // (starts with the host's share of the grand products: never queued ahead)
            ZG_TRY(opening_plan());
            ZG_TRY(arm());
            ZG_TRY(quotient_queue());    // behind y
            ZG_TRY(products_absorb());
            ZG_TRY(arm());
            ZG_TRY(evaluations_queue());  // behind x
            ZG_TRY(quotient_absorb());
            ZG_TRY(arm());
            ZG_TRY(openings_queue());    // behind v
            ZG_TRY(evaluations_absorb());
        }
        ZG_TRY(openings_absorb());
        return finish();
    }

    // ---- the gate
    uint64_t form_sig() const {
        // (everything that shapes the proof's allocation requests and launch sequence: a proof whose signature differs from
        //  the last completed one's is a FIRST proof -- it may create tables and workspace, with synchronisations -- and is
        //  never gated: scheduling form, domain split, digit tables, batch, instance length, and the tuning generation,
        //  which every zg_tuning_set bumps)
        return 1u | (uint64_t)p->use_side << 1 | (uint64_t)split << 2 | (uint64_t)by_degree << 6 | (uint64_t)(p->g->full_table.load() != nullptr) << 3 |
               (uint64_t)(p->gl->full_table.load() != nullptr) << 4 | (uint64_t)ctx->msm_pair << 5 | (uint64_t)(nb & 0xFFu) << 8 |
               (uint64_t)(instance_len & 0xFFFFu) << 16 | (uint64_t)tuning_generation() << 32;
    }
    bool gate_wanted() {
        const int v = knob(K_LAT_GATE);
        if (shplonk) return false;  // (its second half starts from h1 on the host: the plain order)
        if (p->phased() || phase_fn) return false;  // (a phase's witness starts from the challenges on the host)
        if (pk.NS) return false;  // (a circuit with shuffles: the plain order)
        if (no_gate || (v < 0 ? LAT_GATE_DEFAULT : v) == 0 || !p->use_side || nb != 1 || p->world > 1 || p->rccl_comm) return false;
        if (p->warm_sig != form_sig()) return false;  // (first-use allocations and their synchronisations are behind us)
        // (a runtime that completes every launch before it submits the next one would never reach publish())
        const bool serialising = runtime_serialises_launches();
        // room in the staging arena for the five gated uploads and the index lists behind them
        const size_t need = 5 * ((size_t)nb * sizeof(ProofConst) + 64) + (256u << 10);
        if (serialising || sizeof(ProofConst) % 16 != 0 || !p->pin.stage_has(need)) return false;
        *p->pin.gave_up_word() = 0;  // (no gate kernel is in flight between proofs)
        return true;
    }
    int arm() {
        const size_t bytes = (size_t)nb * sizeof(ProofConst);
        // (gate_wanted() checked the arena's room: a phase queued ahead WITHOUT its gate would run on the previous challenge)
        gate_slot = gated && !armed ? p->pin.stage_take(bytes) : nullptr;
        ZG_REQUIRE(gate_slot != nullptr, ZG_ERR_INVALID_ARG, "zg_prover_prove: no room to arm the gate");
        if (++p->gate_seq == 0) ++p->gate_seq;
        armed = true;  // (from here on somebody has to open it: ~ProveBatch)
        hold.word = p->pin.gate_word();
        hold.seq = p->gate_seq;
        ctx->gate_hold = &hold;  // (... or gate_yield(), from a blocking call of the phase queued behind it)
        if (ctx->side) ctx->side->gate_hold = &hold;
        const uint4* dev_view = p->pin.dev_view(reinterpret_cast<const uint4*>(gate_slot));
        // (ZG_LAT_GATE=2, for the tests: the proof's first gate is never opened by publish() and gives up after 0.2 s)
        const bool lost = knob(K_LAT_GATE) == 2 && gates_armed == 0;
        gates_armed++;
        ZG_LAUNCH(ctx, "gate_pull", (double)bytes * 2, gate_pull_kernel, dim3(1), dim3(256), 0, p->pin.dev_view(p->pin.gate_word()),
                  lost ? p->gate_seq + 0x40000000u : p->gate_seq, p->pin.dev_view(p->pin.gave_up_word()), lost ? GATE_MAX_TICKS / 20 : GATE_MAX_TICKS, dev_view, (uint4*)p->d_pc, (uint32_t)(bytes / 16));
        ZG_HIP(hipGetLastError());
        return ZG_OK;
    }
    void open_gate() {
        if (!armed) return;
        __atomic_store_n(p->pin.gate_word(), p->gate_seq, __ATOMIC_SEQ_CST);
        armed = false;
        hold.word = nullptr;
    }
    // a gate kernel ran into its time limit, or a blocking call let one go early: phases ran on the previous challenge
    bool gate_failed() const { return gated && (*p->pin.gave_up_word() != 0 || hold.yielded); }
    // the per-proof scalars as the host holds them now -> d_pc: through the armed gate, else behind the work already queued
    int publish() {
        if (!armed) return upload_consts(p, nb);
        memcpy(gate_slot, p->hpc.data(), (size_t)nb * sizeof(ProofConst));
        open_gate();  // (a gate that gate_yield() already opened copied the previous scalars: gate_failed(), the proof is re-made)
        return ZG_OK;
    }
    // (an error return between arm() and publish(): the queue must drain whatever it then computes)
    ~ProveBatch() {
        open_gate();
        if (ctx->gate_hold == &hold) ctx->gate_hold = nullptr;
        if (ctx->side && ctx->side->gate_hold == &hold) ctx->side->gate_hold = nullptr;
    }

    void begin() {
        p->have_last = false;
        // (the previous batch left through an error return: drain what it queued before its staging arena and slots are reused)
        if (p->in_flight) (void)prover_drain(p);
        p->in_flight = true;
        p->pin.stage_reset();
    }

    int load_inputs() {
        ZG_TRY(advice_into_slots(p, nb, advice_host, advice_dev));

        // ---- vk + instance values into the transcripts; instance polynomials
        for (uint32_t b = 0; b < nb; b++) {
            memset(&p->hpc[b], 0, sizeof(ProofConst));
            memcpy(p->hpc[b].key, keys + 32 * (size_t)b, 32);
            if (b < ntr) tr[b].common_scalar(pk.vk_repr);
        }
        ZG_TRY(upload_consts(p, nb));
        // vanishing::Argument::commit's random polynomial depends on no challenge: generate it now and
        // commit it inside the permuted-lookup batch (coefficient basis `g` next to `g_lagrange` vectors)
        random_row = p->perm + (size_t)(2 * NL) * n;  // (proof 0's; proof b's is perm_bs further)
        // (the same launch draws the blinding rows of the advice columns: commit_lagrange's input below)
        adv = p->adv_val;
        ZG_TRY(poly_random_and_blind(ctx, p->d_pc, nb, random_row, perm_bs, pp_at(p->ix_random), pp_bs, n, TAG_RANDOM_POLY, adv, adv_bs,
                                     n, A, usable, bf + 1, TAG_ADVICE_BLIND));
        if (I) {
            for (uint32_t b = 0; b < nb; b++) {
                Fe* iv = p->inst_val + b * inst_bs;
                if (p->inst_filled[b] > instance_len) ZG_HIP(hipMemsetAsync(iv, 0, inst_bs * 32, st));  // (zeroed at create)
                p->inst_filled[b] = instance_len;
                for (uint32_t c = 0; c < IU; c++) {
                    const zg_fr* src = instance_len ? instance[b] + (size_t)c * instance_len : nullptr;
                    for (size_t i = 0; i < instance_len; i++) T(b).common_scalar(to_fe(&src[i]));
                    if (instance_len) ZG_TRY(h2d(p, iv + (size_t)c * n, src, instance_len * 32));
                }
            }
        }
        base_cols.fixed = pk.fixed_val; base_cols.advice = adv; base_cols.instance = p->inst_val;
        base_cols.log_size = k; base_cols.rot_scale = 1;
        base_cols.adv_bs = adv_bs; base_cols.inst_bs = inst_bs;
        return ZG_OK;
    }

    // ---- the advice phases.  One phase, no challenge, no callback: the launches and waits are what they were.
    // the columns of phase `ph` in runs of neighbours: (first column, count)
    std::vector<std::pair<uint32_t, uint32_t>> phase_runs(uint32_t ph) const {
        std::vector<std::pair<uint32_t, uint32_t>> runs;
        if (!p->phased()) {
            if (A) runs.push_back({0u, A});
            return runs;
        }
        for (uint32_t c : plan->lay.phases[ph].columns) {
            if (!runs.empty() && runs.back().first + runs.back().second == c) runs.back().second++;
            else runs.push_back({c, 1u});
        }
        return runs;
    }
    // the caller's witness of a phase (zg_prover_prove_phased): usable rows of the phase's columns, written on this stream
    // or before the callback returns
    int phase_witness(uint32_t ph) {
        if (!phase_fn) return ZG_OK;
        std::vector<void*> slots(nb);
        for (uint32_t b = 0; b < nb; b++) slots[b] = p->adv_val + b * adv_bs;
        const int st_fn = phase_fn(phase_user, ph, nb, chal.data(), slots.data());
        if (st_fn != 0) {
            (void)prover_drain(p);
            p->in_flight = false;
            for (uint32_t b = 0; b < ntr; b++) proof_lens[b] = 0;
            ZG_REQUIRE(false, ZG_ERR_INVALID_ARG, "%s: the callback returned %d in phase %u",
                       multi ? "zg_prover_prove_circuits_phased" : "zg_prover_prove_phased", st_fn, ph);
        }
        return ZG_OK;
    }
    int advice_phase_queue(uint32_t ph) {
        ZG_TRY(phase_witness(ph));
        ZG_TRY(fork());
        if (ph == 0 && IU) {
            const Grouping g = grouping(IU, inst_bs, pp_bs);
            ZG_TRY(ntt_batch_to_dev(sx, p->inst_val, pp_at(p->ix_inst), n, (size_t)nb * IU, k, pk.omega_inv, &pk.ifft_div, &g));
            if (phase_cosets) ZG_TRY(to_cosets(sx, p->ix_inst, IU));
        }
        // ---- advice: commit (Lagrange basis), one launch sequence per run of neighbouring columns, one event for the phase
        const auto runs = phase_runs(ph);
        size_t at = 0;
        for (size_t r = 0; r < runs.size(); r++) {
            const uint32_t c0 = runs[r].first, cnt = runs[r].second;
            ZG_TRY(commit(p, phase_msm(p->gl, adv + (size_t)c0 * n, n, cnt, adv_bs), W_ADVICE, at, r + 1 == runs.size()));
            at += (size_t)nb * cnt;
            const Grouping g = grouping(cnt, adv_bs, pp_bs);
            ZG_TRY(ntt_batch_to_dev(sx, adv + (size_t)c0 * n, pp_at(p->ix_adv + c0), n, (size_t)nb * cnt, k, pk.omega_inv, &pk.ifft_div, &g));
            if (phase_cosets) ZG_TRY(to_cosets(sx, p->ix_adv + c0, cnt));
        }
        ZG_TICK("advice: queued");
        return ZG_OK;
    }
    // the phase's points into the transcripts (run r of proof b behind run r of proof b - 1, as the MSMs left them), then
    // its challenges: squeezed, recorded for the next callback and written into their pseudo-columns
    int advice_phase_absorb(uint32_t ph) {
        const auto runs = phase_runs(ph);
        size_t total = 0;
        for (const auto& r : runs) total += (size_t)nb * r.second;
        if (total) {
            ZG_TRY(wait_points(p, total, pts, W_ADVICE));
            ZG_TICK("advice: points on the host");
            for (uint32_t b = 0; b < nb; b++) {
                size_t at = 0;
                for (const auto& r : runs) {
                    for (uint32_t c = 0; c < r.second; c++) T(b).write_point(pts[at + (size_t)b * r.second + c]);
                    at += (size_t)nb * r.second;
                }
            }
        }
        if (!p->phased()) return ZG_OK;
        const std::vector<uint32_t>& squeezed = plan->lay.phases[ph].challenges;
        if (squeezed.empty()) return ZG_OK;
        ChalFill f;
        std::vector<Fe>& vals = chal_vals;  // [nb][NC][2]: the value as the rows hold it, and as the coset slabs do
        vals.resize((size_t)nb * (NC ? NC : 1) * 2, fe_zero());
        for (uint32_t j : squeezed) {
            Fe c{};
            for (uint32_t b = 0; b < nb; b++) {
                if (b < ntr) c = tr[b].squeeze();  // (multi: ONE squeeze, the same value in every circuit's row and column)
                memcpy(&chal[(size_t)b * nch + j], &c, 32);
                if (j < NC) {
                    vals[((size_t)b * NC + j) * 2] = c;
                    vals[((size_t)b * NC + j) * 2 + 1] = hat ? Fr::mul(c, Fr9Params::c261_fe()) : c;
                }
            }
            if (j < NC) f.chal[f.count++] = j;
        }
        if (!f.count) return ZG_OK;
        // (every phase stages and uploads the array as it stands, behind the fills of the phase before on this stream)
        ZG_TRY(h2d(p, p->d_chal, vals.data(), vals.size() * sizeof(Fe)));
        f.col0 = IU;
        f.val = p->inst_val; f.val_bs = inst_bs;
        f.coef = pp_at(p->ix_inst + IU); f.coef_bs = pp_bs;
        f.n = n;
        for (uint32_t di = dlo; di < dhi; di++) {
            f.cos[f.nparts] = p->dbuf[di].cos + (size_t)(A + IU) * pk.dom[di].en;
            f.cos_bs[f.nparts] = (size_t)p->ncos * pk.dom[di].en;
            f.en[f.nparts++] = pk.dom[di].en;
        }
        f.vals = p->d_chal; f.stride = NC;
        return poly_challenge_fill(ctx, f, nb);
    }
    int advice_queue() { return advice_phase_queue(0); }
    int advice_absorb() {
        ZG_TRY(advice_phase_absorb(0));
        for (uint32_t ph = 1; ph < p->n_phases; ph++) {
            ZG_TRY(advice_phase_queue(ph));
            ZG_TRY(advice_phase_absorb(ph));
        }
        squeeze_into(&ProofConst::theta);
        ZG_TICK("theta");
        ZG_TRY(publish());
        ZG_TICK("theta uploaded");
        lap(0);
        return ZG_OK;
    }

    int permuted_queue() {
        // ---- lookups: commit_permuted (+ the random polynomial's commitment)
        if (NL) {
            // permute_expression_pair on the device: canonical keys (written by the compression kernel itself, with
            // the sentinel padding), bitonic sort of inputs and tables, scan-based construction of s' (sort.hip).
            // raw rows [0, m) = inputs -> a', [m, 2m) = tables, m = nb * NL, row b * NL + l = lookup l of proof b.
            const uint32_t m = nb * NL;
            Fe *raw_in = p->raw, *raw_tab = p->raw + (size_t)m * n;
            uint32_t* d_err = p->sort_u32 + (size_t)2 * m * n + 2 * m;  // behind permute_pairs' scratch: zeroed by the same fill
            ZG_TRY(poly_lookup_compress(ctx, pk.dc, base_cols, p->d_pc, nb, p->cin, p->ctab, n, raw_in, raw_tab, usable));
            auto t_sort = clk::now();
            ZG_TRY(poly_sort_keys(ctx, p->raw, n, 2 * m));
            ZG_TRY(poly_permute_pairs(ctx, raw_in, raw_tab, p->sraw, n, usable, m, p->sort_u32, p->sort_fe, d_err));
            // perm[2l] = a'_l, perm[2l+1] = s'_l (Montgomery form) on the usable rows, then the blinding tail
            // (blinding: a' rows get tag 2, s' rows tag 3, index = lookup * (bf+1) + j)
            ZG_TRY(poly_permuted_finish(ctx, p->d_pc, nb, raw_in, p->sraw, p->perm, perm_bs, n, usable, bf + 1, NL, TAG_PERMUTED_INPUT,
                                        TAG_PERMUTED_TABLE));
            p->phase_ms[7] = std::chrono::duration<double, std::milli>(clk::now() - t_sort).count();
            ZG_TRY(fork());
            // the lookups' error words leave on the side stream, beside the commitments (an event of their own)
            h_err = p->pin.lookup_errors();
            ZG_HIP(hipMemcpyAsync(h_err, d_err, m * sizeof(uint32_t), hipMemcpyDeviceToHost, ss));
            ZG_HIP(hipEventRecord(p->ev_err, ss));
            // (a' and s' are sorted: equal neighbours everywhere, so the run form leaves one entry per distinct value)
            const zg_bases *cgl = naf_of(p, p->gl), *cg = cgl == p->gl ? p->g : naf_of(p, p->g);  // (both or neither)
            const uint64_t sorted_runs = cgl->run_table && 2 * NL < 64 ? (1ull << (2 * NL)) - 1ull : 0ull;
            MsmJob msm = phase_msm(cgl, p->perm, n, 2 * NL + 1, perm_bs);
            msm.bases_b = cg; msm.split = 2 * NL;  // (the random polynomial, last of each group, against g)
            msm.run_mask = sorted_runs; msm.naf_width = p->naf_gl_w;
            ZG_TRY(commit(p, msm, W_PERMUTED));
            {
                const Grouping g = grouping(2 * NL, perm_bs, pp_bs);
                ZG_TRY(ntt_batch_to_dev(sx, p->perm, pp_at(p->ix_perm), n, (size_t)nb * 2 * NL, k, pk.omega_inv, &pk.ifft_div, &g));
            }
            if (phase_cosets) ZG_TRY(to_cosets(sx, p->ix_perm, 2 * NL));
        }
        ZG_TICK("permuted: queued");
        return ZG_OK;
    }
    int permuted_absorb() {
        random_commit.resize(nb);
        have_random = false;
        if (NL) {
            ZG_TRY(wait_points(p, (size_t)nb * (2 * NL + 1), pts, W_PERMUTED));
            ZG_HIP(hipEventSynchronize(p->ev_err));
            ZG_TICK("permuted: points on the host");
            for (uint32_t b = 0; b < nb; b++) {
                for (uint32_t l = 0; l < NL; l++)
                    if (h_err[b * NL + l] && status[b] == ZG_OK) {
                        set_error("zg_prover_prove: lookup %u of %s %u has an input outside its table (ConstraintSystemFailure)", l,
                                  multi ? "circuit" : "proof", b);
                        status[b] = ZG_ERR_CONSTRAINT;
                        if (multi) status[0] = ZG_ERR_CONSTRAINT;  // (the one proof fails, as upstream's `?` does)
                    }
                const Jac* q = &pts[(size_t)b * (2 * NL + 1)];
                for (uint32_t i = 0; i < 2 * NL; i++) T(b).write_point(q[i]);
                random_commit[b] = q[2 * NL];
            }
            have_random = true;
            if (ntr == 1 && status[0] != ZG_OK && gate_failed()) return ZG_ERR_HIP;  // (error words from behind a failed gate: run() re-makes the proof)
            if (ntr == 1 && status[0] != ZG_OK) {  // a lone proof stops here, as upstream's `?` does
                open_gate();  // (whatever was queued ahead runs out on stale scalars: nobody reads its results)
                (void)prover_drain(p);
                if (statuses) statuses[0] = status[0];
                proof_lens[0] = 0;
                p->in_flight = false;
                return status[0];
            }
        }
        squeeze_into(&ProofConst::beta);
        squeeze_into(&ProofConst::gamma);
        ZG_TICK("beta, gamma");
        ZG_TRY(publish());
        ZG_TICK("beta, gamma uploaded");
        lap(1);
        return ZG_OK;
    }

    // ---- permutation products (sets chained through z[n - bf - 1]) and lookup products
    // (in two parts: the terms and the running products up to their totals need beta and gamma only; what follows the
    //  totals begins, in the latency form, with the HOST inverting them -- it cannot be queued ahead of anything)
    int products_terms_queue() {
        const uint32_t mb = S + NL;
        if (S) ZG_TRY(poly_perm_terms(ctx, pk.dc, base_cols, p->d_pc, nb, pk.sigma_val, pk.omega_tw, p->num, p->den, mb, n));
        // (a'_l / s'_l are interleaved in `perm`: two views with a stride of two columns)
        ZG_TRY(poly_lookup_terms(ctx, p->d_pc, nb, p->cin, p->ctab, p->perm, p->perm + n, (size_t)2 * n, perm_bs, p->num, p->den, mb, S, n, NL));
        // all running products of the batch in one scan sequence; per proof the S permutation sets are chained
        // through row n - bf - 1, the lookup products start from one
        if (mb) ZG_TRY(poly_grand_product(ctx, p->num, p->den, nullptr, p->zs, p->tmp, n, nb * mb, S, n - bf - 1, mb, zs_bs, 1));
        ZG_TICK("product terms: queued");
        return ZG_OK;
    }
    int products_queue() {
        const uint32_t mb = S + NL;
        if (mb) {
            ZG_TRY(poly_grand_product(ctx, p->num, p->den, nullptr, p->zs, p->tmp, n, nb * mb, S, n - bf - 1, mb, zs_bs, 2));
            ZG_TRY(poly_blind_rows2(ctx, p->d_pc, nb, p->zs, zs_bs, n, S, TAG_PERM_Z, NL, TAG_LOOKUP_Z, n - bf, bf));  // (lz follows pz)
            // The products stay constant wherever a row changes nothing (every padding row of the circuit): they are
            // committed in the run form, sum_i (z_i - z_{i+1}) Q_i over the running sums Q of g_lagrange.
            const zg_bases *cgl = naf_of(p, p->gl), *cg = cgl == p->gl ? p->g : naf_of(p, p->g);
            const uint64_t z_runs = cgl->run_table && mb < 64 ? (1ull << mb) - 1ull : 0ull;
            ZG_TRY(fork());
            prod_per = mb;
            if (!have_random) {  // no lookups: the random polynomial rides here instead (row mb of zs)
                for (uint32_t b = 0; b < nb; b++)
                    ZG_HIP(hipMemcpyAsync(p->zs + b * zs_bs + (size_t)mb * n, random_row + b * perm_bs, (size_t)n * 32, hipMemcpyDeviceToDevice, st));
                prod_per = mb + 1;
            }
            MsmJob msm = phase_msm(cgl, p->zs, n, prod_per, zs_bs);
            if (!have_random) msm.bases_b = cg, msm.split = mb;
            msm.run_mask = z_runs; msm.naf_width = p->naf_gl_w;
            ZG_TRY(commit(p, msm, W_PRODUCTS, 0, NS == 0));
            {
                const Grouping g = grouping(mb, zs_bs, pp_bs);
                ZG_TRY(ntt_batch_to_dev(sx, p->zs, pp_at(p->ix_pz), n, (size_t)nb * mb, k, pk.omega_inv, &pk.ifft_div, &g));
            }
            if (phase_cosets) ZG_TRY(to_cosets(sx, p->ix_pz, mb));
        } else if (!have_random) {  // neither lookups nor permutation: commit the random polynomial on its own
            prod_per = 1;
            ZG_TRY(commit(p, phase_msm(p->g, random_row, n, 1, perm_bs), W_PRODUCTS, 0, NS == 0));
        } else {
            prod_per = 0;
        }
        if (NS) ZG_TRY(shuffles_queue());
        ZG_TICK("products: queued");
        return ZG_OK;
    }
    // ---- the shuffle products (shuffle::Argument::commit_product): terms, ONE grand-product sequence and ONE MSM launch
    // sequence over the nb * NS columns, behind the phase's other commitments in the results; then the way of a lookup
    // product -- coefficients, cosets -- on the side stream
    int shuffles_queue() {
        const size_t sz_bs = (size_t)NS * n;
        ZG_TRY(poly_shuffle_terms(ctx, pk.dc, pk.d_shuffles, NS, base_cols, p->d_pc, nb, p->snum, p->sden, n));
        ZG_TRY(poly_grand_product(ctx, p->snum, p->sden, nullptr, p->sz, p->stmp, n, nb * NS, 0, n - bf - 1, NS, sz_bs, 0));
        ZG_TRY(poly_blind_rows2(ctx, p->d_pc, nb, p->sz, sz_bs, n, NS, TAG_SHUFFLE_Z, 0, TAG_SHUFFLE_Z, n - bf, bf));
        ZG_TRY(fork());
        ZG_TRY(commit(p, phase_msm(p->gl, p->sz, n, NS, sz_bs), W_PRODUCTS, (size_t)nb * prod_per, true));
        const Grouping g = grouping(NS, sz_bs, pp_bs);
        ZG_TRY(ntt_batch_to_dev(sx, p->sz, pp_at(p->ix_sz), n, (size_t)nb * NS, k, pk.omega_inv, &pk.ifft_div, &g));
        if (phase_cosets) ZG_TRY(to_cosets(sx, p->ix_sz, NS));
        return ZG_OK;
    }
    int products_absorb() {
        const uint32_t mb = S + NL;
        if (NS) return products_absorb_shuffles();
        if (mb) {
            ZG_TRY(wait_points(p, (size_t)nb * prod_per, pts, W_PRODUCTS));
            ZG_TICK("products: points on the host");
            // (a slot's commitments are [S permutation z | NL lookup z]; the proof of several circuits writes the two families
            //  as two passes over the circuits, as upstream commits them)
            for (uint32_t pass = 0; pass < (multi ? 2u : 1u); pass++)
                for (uint32_t b = 0; b < nb; b++) {
                    const Jac* q = &pts[(size_t)b * prod_per];
                    const uint32_t i0 = multi && pass ? S : 0, i1 = multi && !pass ? S : mb;
                    for (uint32_t i = i0; i < i1; i++) T(b).write_point(q[i]);
                    if (!have_random) random_commit[b] = q[mb];
                }
        } else if (!have_random) {
            ZG_TRY(wait_points(p, nb, pts, W_PRODUCTS));
            for (uint32_t b = 0; b < nb; b++) random_commit[b] = pts[b];
        }
        have_random = true;
        for (uint32_t b = 0; b < ntr; b++) tr[b].write_point(random_commit[b]);  // (multi: ONE random polynomial, slot 0's, from key 0)
        Fe y{};
        for (uint32_t b = 0; b < nb; b++) {
            if (b < ntr) y = tr[b].squeeze();
            evalh_consts(p->hpc[b], y, pk);
        }
        if (multi) fold_weights(y);
        ZG_TICK("y");
        ZG_TRY(publish());
        ZG_TICK("y uploaded");
        lap(2);
        return ZG_OK;
    }

    // (with shuffles: the phase's results are [nb][prod_per] permutation z, lookup z and -- where it rides here -- the
    //  random polynomial, then [nb][NS] shuffle z; the transcript takes permutation z, lookup z, shuffle z, random)
    int products_absorb_shuffles() {
        const uint32_t mb = S + NL;
        ZG_TRY(wait_points(p, (size_t)nb * (prod_per + NS), pts, W_PRODUCTS));
        // (a proof per slot takes its three families in turn; the proof of several circuits takes each family as a pass over
        //  the circuits, as upstream commits them)
        auto family = [&](uint32_t b, uint32_t fam) {  // slot b's permutation z (0), lookup z (1) or shuffle z (2)
            const Jac* q = fam < 2 ? &pts[(size_t)b * prod_per + (fam ? S : 0)] : &pts[(size_t)nb * prod_per + (size_t)b * NS];
            const uint32_t cnt = fam == 0 ? S : fam == 1 ? NL : NS;
            for (uint32_t i = 0; i < cnt; i++) T(b).write_point(q[i]);
        };
        if (multi) {
            for (uint32_t fam = 0; fam < 3; fam++)
                for (uint32_t b = 0; b < nb; b++) family(b, fam);
        } else {
            for (uint32_t b = 0; b < nb; b++)
                for (uint32_t fam = 0; fam < 3; fam++) family(b, fam);
        }
        for (uint32_t b = 0; b < nb && !have_random; b++) random_commit[b] = pts[(size_t)b * prod_per + mb];
        have_random = true;
        for (uint32_t b = 0; b < ntr; b++) tr[b].write_point(random_commit[b]);  // (multi: ONE random polynomial, slot 0's, from key 0)
        Fe y{};
        for (uint32_t b = 0; b < nb; b++) {
            if (b < ntr) y = tr[b].squeeze();
            evalh_consts(p->hpc[b], y, pk);
        }
        if (multi) fold_weights(y);
        ZG_TICK("y");
        ZG_TRY(publish());
        lap(2);
        return ZG_OK;
    }

    // multi: the weights of the slots' quotients in the proof's.  upstream's evaluate_h carries its Horner value in y from
    // one circuit into the next, so with m terms per circuit (gates, permutation, 5 per lookup, 3 per shuffle) and h_c the
    // quotient of circuit c alone, h = sum_c y^(m (N - 1 - c)) h_c: Horner in Y = y^m over the circuits, circuit 0 first.
    void fold_weights(const Fe& y) {
        const uint32_t m = pk.dc.n_gates + (S ? 2 + (S - 1) + S : 0) + 5 * NL + 3 * NS;
        const Fe Y = Fr::pow_u64(y, m);
        Fe w = Fr::one();
        for (uint32_t c = nb; c-- > 0;) {
            p->hpc[c].fold_w = w;
            w = Fr::mul(w, Y);
        }
    }

    int quotient_queue() {
        ZG_TRY(join());  // evaluate_h reads every coset the side stream produced
        // (throughput configuration: nothing overlaps, so every witness polynomial goes to its cosets here, in one batch per
        //  coset, instead of phase by phase)
        if (!phase_cosets && !NC) ZG_TRY(to_cosets(ctx, p->ix_adv, p->ncos));
        if (!phase_cosets && NC) {  // (the challenges' slabs are filled, not transformed: the columns on either side of them)
            ZG_TRY(to_cosets(ctx, p->ix_adv, A + IU));
            ZG_TRY(to_cosets(ctx, p->ix_pz, p->ncos - (A + I)));
        }
        // ---- evaluate_h (+ division by X^n - 1) on every part of the extended domain, back to coefficients, h pieces
        for (uint32_t di = dlo; di < dhi; di++) {
            const EvalHArgs a = evalh_args(p, di);
            // (by degree: all terms and, beside them, the high ones on the first part; the high ones alone on the second)
            const EvalHMode mode = !by_degree ? EH_ALL : di == 1 ? EH_BOTH : EH_HIGH;
            ZG_TRY(poly_evaluate_h(ctx, a, pk.dom[di].en, nb, A + I + pk.F, (double)((size_t)1 << ek) * ((double)pk.dom[di].en / parts_en), mode));
        }
        // the shuffles' terms, which stand last: a pass over h on every part (and over the high terms' sum where it is kept)
        for (uint32_t di = dlo; NS && di < dhi; di++) {
            EvalHArgs a = evalh_args(p, di);
            if (!(by_degree && di == 1)) a.h_hi = nullptr;
            const Fe* sz_cos = p->dbuf[di].cos + (size_t)(p->ix_sz - p->ix_adv) * pk.dom[di].en;
            ZG_TRY(poly_shuffle_h(ctx, a, pk.d_shuffles, NS, sz_cos, pk.dom[di].en, nb));
        }
        // multi: the slots' quotients into slot 0's, on each part, BEFORE the transforms back: those, the pieces and their
        // commitments then exist once (nq = 1)
        if (multi)
            for (uint32_t di = dlo; di < dhi; di++) ZG_TRY(poly_fold_slots(ctx, p->d_pc, nb, p->dbuf[di].h, pk.dom[di].en, pk.dom[di].en));
        p->have_last = true;
        p->last_split = split;
        p->last_by_degree = by_degree;
        p->last_nb = nb;
        const double ext_inv_unit = (double)nq * 2.0 * (double)((size_t)1 << ek) * 32.0;  // (ext -> coeff, 2 * 8n * 32 B)
        if (!split) {
            ctx->unit_next = ext_inv_unit;
            ZG_TRY(coset_to_coeff_dev(ctx, p->dbuf[0].h, ek, (size_t)Q * n, pp_at(p->ix_hpiece), hat, pk.zeta, nq, pk.dom[0].en, pp_bs));
        } else {
            // h = A + (X^L1 - c1) B:  A (degree < L1) from the first coset, where X^L1 = c1 = shift1^L1;  B (degree < L2)
            // from the second, where X^L1 = c2 and X^L2 = e are constants too:  B = (h - A) / (c2 - c1) there, with A
            // folded modulo X^L2 - e before it is evaluated on those L2 points.
            const PkDev::Dom &d1 = pk.dom[1], &d2 = pk.dom[2];
            const uint32_t L1 = d1.en, L2 = d2.en;
            const Fe zeta = pk.zeta, zeta2 = Fr::sqr(zeta);
            const Fe c1 = Fr::pow_u64(zeta, L1), c2 = Fr::pow_u64(zeta2, L1), e = Fr::pow_u64(zeta2, L2);
            Fe* hp = pp_at(p->ix_hpiece);
            const size_t tb = (size_t)3 * L2;
            Fe *fold = p->split_tmp, *a2 = fold + L2, *bc = a2 + L2;
            ctx->unit_next = ext_inv_unit;  // (the three transforms of the split form stand for ONE extended_to_coeff)
            //
            // By degree, h = h_lo + h_hi with deg h_lo < L1 (both are polynomials when the statement holds: every term
            // vanishes on H by itself).  A is as before -- all terms on the first coset, so A = h_lo + A_h with
            // A_h = h_hi mod (X^L1 - c1) -- but only h_hi reaches past L1: B = (h_hi - A_h) / (c2 - c1) on the second coset,
            // from the high terms there and A_h, the coefficients of the high terms on the first coset (ONE more transform
            // of L1 points, into the first coset's h, which A has left).  h = A - c1 B + X^L1 B all the same.
            ZG_TRY(coset_to_coeff_dev(ctx, p->dbuf[1].h, d1.ek, L1, hp, hat, zeta, nq, L1, pp_bs));  // A, in place of the low pieces
            const Fe* af = hp;
            size_t af_bs = pp_bs;
            if (by_degree) {
                ctx->unit_next = 0.0;
                ZG_TRY(coset_to_coeff_dev(ctx, p->h_hi, d1.ek, L1, p->dbuf[1].h, hat, zeta, nq, L1, L1));  // A_h
                af = p->dbuf[1].h;
                af_bs = L1;
            }
            ZG_TRY(poly_fold(ctx, nq, af, af_bs, L2, L1 / L2, e, fold, tb));                       // A (A_h) mod (X^L2 - e)
            ctx->unit_next = 0.0;
            ZG_TRY(coeff_to_coset_dev(ctx, fold, tb, L2, a2, tb, nq, d2.ek, false, zeta2));            // A on the second coset
            const Fe unhat = hat ? Fr::inv(Fr::from_u64(32)) : Fr::one();
            ZG_TRY(poly_diff_scale(ctx, nq, p->dbuf[2].h, L2, unhat, a2, tb, Fr::inv(Fr::sub(c2, c1)), a2, tb, L2));  // B on the second coset
            ctx->unit_next = 0.0;
            ZG_TRY(coset_to_coeff_dev(ctx, a2, d2.ek, L2, bc, false, zeta2, nq, tb, tb));              // B
            ZG_TRY(poly_split_combine(ctx, nq, hp, pp_bs, bc, tb, L2, c1, L1));                    // h = A - c1 B + X^L1 B
        }
        ctx->msm_dense_hint = true;  // (the quotient pieces are random vectors: every digit of every window is an addition)
        const int st_h = commit(p, phase_msm(dense_g(p), pp_at(p->ix_hpiece), n, Q, pp_bs, nq), W_QUOTIENT);
        ctx->msm_dense_hint = false;
        ZG_TRY(st_h);
        ZG_TICK("h: queued");
        return ZG_OK;
    }
    // (h's commitments, then x and the opening points: needs opening_plan())
    int quotient_absorb() {
        ZG_TRY(wait_points(p, (size_t)nq * Q, pts, W_QUOTIENT));
        ZG_TICK("h: points on the host");
        for (uint32_t b = 0; b < nq; b++)
            for (uint32_t i = 0; i < Q; i++) tr[b].write_point(pts[(size_t)b * Q + i]);
        Fe x{};
        for (uint32_t b = 0; b < nb; b++) {
            ProofConst& c = p->hpc[b];
            if (b < ntr) x = tr[b].squeeze();
            c.xn = Fr::pow_u64(x, n);
            for (uint32_t i = 0; i < npoints; i++) c.points[i] = rotate_omega(pk, x, (int32_t)plan->lay.rotations[i]);
        }
        ZG_TICK("x");
        ZG_TRY(publish());
        ZG_TICK("x uploaded");
        lap(3);
        return ZG_OK;
    }

    // ---- which polynomial is evaluated and opened where: proof_layout.h states it, the three functions below put it into
    // the device list formats (OpenPlan), once per prover, argument and number of circuits in a proof
    int opening_plan() {
        ZG_REQUIRE(!shplonk || p->sh_h1 != nullptr, ZG_ERR_INVALID_ARG, "zg_prover_prove: no SHPLONK buffers (zg_prover_set_multiopen)");
        const std::pair<int, uint32_t> key(p->multiopen, multi ? nb : 1u);
        auto it = p->plans.find(key);
        if (it == p->plans.end()) {
            OpenPlan pl;
            ProofShape shape = proof_shape(pk);
            shape.advice_phase = p->advice_phase;
            shape.challenge_phase = p->challenge_phase;
            pl.lay = build_layout(shape, key.second, shplonk);
            ZG_TRY(plan_evaluations(pl));
            ZG_TRY(shplonk ? plan_shplonk(pl) : plan_gwc(pl));
            it = p->plans.emplace(key, std::move(pl)).first;
        }
        plan = &it->second;
        npoints = (uint32_t)plan->lay.rotations.size();
        ZG_REQUIRE(!shplonk || (size_t)ntr * plan->sh_ncoef <= p->sh_terms + p->cap, ZG_ERR_UNSUPPORTED,
                   "zg_prover_prove: %zu opening queries (room for %zu)", plan->lay.queries.size(), p->sh_terms);
        return ZG_OK;
    }
    // the prover's handles: a commitment's polynomial (with its circuit's slot above it in a list entry)
    uint32_t poly_of(Family fam, uint32_t index) const {
        const uint32_t base[] = {p->ix_adv, p->ix_perm, p->ix_pz, p->ix_lz, p->ix_random, 0, 0, p->ix_fixed, p->ix_sigma, p->ix_hpoly, p->ix_sz};
        return base[fam] + index;
    }
    uint32_t entry_of(Family fam, uint32_t circuit, uint32_t index) const { return circuit << 16 | poly_of(fam, index); }
    int plan_evaluations(OpenPlan& pl) const {
        const ProofLayout& l = pl.lay;
        const uint32_t E = (uint32_t)l.evals.size();
        auto once = [&](const ProofLayout::Query& q) { return l.N > 1 && (q.fam == FIXED || q.fam == RANDOM || q.fam == SIGMA || q.fam == H); };
        uint32_t n_once = 0;
        for (const ProofLayout::Query& q : l.evals) n_once += once(q) ? 1 : 0;
        pl.n_per = (E - n_once) / l.N;
        pl.n_row = pl.n_per + n_once;
        ZG_REQUIRE(l.rotations.size() <= p->max_points, ZG_ERR_UNSUPPORTED, "zg_prover_prove: %u distinct rotations are queried (max %u)",
                   (uint32_t)l.rotations.size(), p->max_points);
        ZG_REQUIRE(pl.n_row <= p->max_evals, ZG_ERR_UNSUPPORTED, "zg_prover_prove: too many evaluations");
        pl.idx.assign(2 * (size_t)pl.n_row, 0);
        std::vector<uint32_t> at_per(l.N, 0);
        uint32_t at_once = pl.n_per;
        for (const ProofLayout::Query& q : l.evals) {  // (transcript order)
            pl.ev_row.push_back(once(q) ? 0 : q.circuit);
            pl.ev_at.push_back(once(q) ? at_once++ : at_per[q.circuit]++);
            pl.idx[pl.ev_at.back()] = poly_of(q.fam, q.index);
            pl.idx[pl.n_row + pl.ev_at.back()] = q.point;
        }
        std::vector<uint32_t> seen(pl.idx.begin(), pl.idx.begin() + pl.n_row);
        std::sort(seen.begin(), seen.end());
        pl.distinct_polys = (uint32_t)(std::unique(seen.begin(), seen.end()) - seen.begin());
        for (uint32_t i = 0; i < l.rotations.size(); i++) pl.slots.push_back(i);
        return ZG_OK;
    }
    // ProverGWC::create_proof's point sets: one per opening point, its queries in order.  A proof of several circuits
    // lists (circuit, polynomial) pairs, each list as long as it has to be (N = 32 of the zero_g circuit puts about a
    // thousand polynomials at x); a lone circuit's lists are 512 entries apart
    int plan_gwc(OpenPlan& pl) const {
        const ProofLayout& l = pl.lay;
        const bool several = l.N > 1;
        ZG_REQUIRE(!several || (l.queries.size() <= p->mlists_cap && p->nsh + p->npp <= 0x10000u), ZG_ERR_UNSUPPORTED,
                   "zg_prover_prove_multi: %zu opening queries (room for %zu)", l.queries.size(), p->mlists_cap);
        for (const std::vector<uint32_t>& set : l.at) {
            ZG_REQUIRE(several || set.size() <= 512, ZG_ERR_UNSUPPORTED, "zg_prover_prove: more than 512 polynomials opened at one point");
            pl.firsts.push_back(several ? (uint32_t)pl.lists.size() : 512 * (uint32_t)pl.counts.size());
            pl.lists.resize(pl.firsts.back(), 0);
            for (uint32_t qi : set) pl.lists.push_back(entry_of(l.queries[qi].fam, l.queries[qi].circuit, l.queries[qi].index));
            pl.counts.push_back((uint32_t)set.size());
        }
        if (!several) pl.lists.resize(512 * l.at.size(), 0);
        ZG_REQUIRE(l.at.size() <= HC_MAX_SETS, ZG_ERR_UNSUPPORTED, "zg_prover_prove: %u opening points", (uint32_t)l.at.size());
        return ZG_OK;
    }
    // ProverSHPLONK::create_proof (v2023_04_20 src/poly/kzg/multiopen/shplonk/prover.rs): the lists of
    // both combinations from the layout's rotation sets -- per point r of T the commitments of every set that holds r,
    // and for L every commitment once
    int plan_shplonk(OpenPlan& pl) const {
        const ProofLayout& l = pl.lay;
        ZG_REQUIRE(p->nsh + p->npp <= 0x10000u, ZG_ERR_UNSUPPORTED, "zg_prover_prove: %u polynomials", p->nsh + p->npp);
        ZG_REQUIRE(l.rsets.size() <= HC_MAX_SETS, ZG_ERR_UNSUPPORTED, "zg_prover_prove: %zu rotation sets (max %u)", l.rsets.size(), HC_MAX_SETS);
        ZG_REQUIRE(l.rotations.size() <= PC_MAX_POINTS, ZG_ERR_UNSUPPORTED, "zg_prover_prove: %zu opening points", l.rotations.size());
        for (const ProofLayout::Com& c : l.coms) pl.com_entry.push_back(entry_of(c.fam, c.circuit, c.index));
        for (const ProofLayout::RotationSet& s : l.rsets) {
            pl.set_mask.push_back(0);
            for (uint32_t r : s.points) pl.set_mask.back() |= 1u << r;
        }
        auto list_sets = [&](uint32_t mask) {  // the commitments of the sets that hold one of `mask`'s points, as one list
            pl.firsts.push_back((uint32_t)pl.lists.size());
            for (size_t i = 0; i < l.rsets.size(); i++)
                if (pl.set_mask[i] & mask)
                    for (uint32_t c : l.rsets[i].coms) pl.lists.push_back(pl.com_entry[c]);
            pl.counts.push_back((uint32_t)pl.lists.size() - pl.firsts.back());
        };
        for (uint32_t r = 0; r < l.rotations.size(); r++) list_sets(1u << r);
        pl.sh_ncoef = std::max(pl.lists.size(), l.coms.size() + 1);
        list_sets(~0u);
        pl.lists.push_back(0);  // (the place of h1's coefficient: it is no polynomial of the set)
        ZG_REQUIRE(pl.lists.size() <= 2 * p->sh_terms + 16, ZG_ERR_UNSUPPORTED, "zg_prover_prove: %zu opening queries (room for %zu)",
                   l.queries.size(), p->sh_terms);
        return ZG_OK;
    }
    int evaluations_queue() {
        // vanishing.evaluate: h(X) = sum_i xn^i h_i(X)
        d_hlist = p->d_idx + (size_t)4 * p->max_evals;
        {
            std::vector<uint32_t> list(Q);
            for (uint32_t i = 0; i < Q; i++) list[i] = p->ix_hpiece + (Q - 1 - i);
            ZG_TRY(h2d_list(p, d_hlist, list));
            ZG_TRY(poly_horner_combine_xn(ctx, polys, p->d_pc, nq, d_hlist, Q, pp_at(p->ix_hpoly), pp_bs, n));
        }
        ZG_TRY(poly_powers(ctx, p->d_pc, nq, npoints, n, p->pw, pw_bs));  // (multi: one x, one table of powers)
        const uint32_t E = plan->n_row, n_per = plan->n_per;
        ZG_TRY(h2d_list(p, p->d_idx, plan->idx));
        // (the evaluations too are written where the host reads them: no copy command behind the kernel)
        if (!multi) {
            ZG_TRY(poly_dot(ctx, polys, nb, n, p->d_idx, p->d_idx + E, p->pw, pw_bs, E, p->pin.dev_view(p->pin.evals()), p->max_evals,
                            plan->distinct_polys, npoints));
        } else {
            // every circuit's own evaluations, then -- once, slot 0 -- the shared ones: all against the one table of powers
            ZG_TRY(poly_dot(ctx, polys, nb, n, p->d_idx, p->d_idx + E, p->pw, 0, n_per, p->pin.dev_view(p->pin.evals()), p->max_evals, 0, npoints));
            ZG_TRY(poly_dot(ctx, polys, 1, n, p->d_idx + n_per, p->d_idx + E + n_per, p->pw, 0, E - n_per, p->pin.dev_view(p->pin.evals()) + n_per,
                            p->max_evals, 0, npoints));
        }
        ev_all = p->pin.evals();
        ZG_HIP(hipEventRecord(p->evs[W_EVALS], st));
        ZG_TICK("evals: queued");
        return ZG_OK;
    }
    // evaluation e of the layout, of the proof whose (first) slot is b
    const Fe& ev(uint32_t b, uint32_t e) const { return ev_all[(size_t)(b + plan->ev_row[e]) * p->max_evals + plan->ev_at[e]]; }
    // (the evaluations into the transcripts in the layout's order, then v and each point set's v-weighted evaluation)
    int evaluations_absorb() {
        ZG_HIP(hipEventSynchronize(p->evs[W_EVALS]));
        ZG_TICK("evals on the host");
        const ProofLayout& l = plan->lay;
        for (uint32_t b = 0; b < ntr; b++)
            for (uint32_t e = 0; e < l.n_scalars(); e++) tr[b].write_scalar(ev(b, e));
        if (shplonk) return shplonk_numerator_tables();
        for (uint32_t b = 0; b < ntr; b++) {
            const Fe v = tr[b].squeeze();
            for (uint32_t s = 0; s < nb; s++)
                if (multi || s == b) p->hpc[s].v = v;
            for (uint32_t s = 0; s < npoints; s++) {  // eval_batch of a set: Horner in v over its queries' evaluations, in order
                Fe eval_batch = fe_zero();
                for (uint32_t qi : l.at[s]) eval_batch = Fr::add(Fr::mul(eval_batch, v), ev(b, l.queries[qi].eval));
                p->hpc[b].subs[s] = eval_batch;
            }
        }
        ZG_TICK("v");
        ZG_TRY(publish());
        ZG_TICK("v uploaded");
        lap(4);
        return ZG_OK;
    }

    int openings_queue() {
        if (shplonk) return shplonk_h1_queue();
        // poly_batch of every point set in one launch: set s -> wpoly[2s]
        // (their own region of d_idx, behind the evaluation lists: nothing else writes there between proofs)
        uint32_t* d_lists = multi ? p->d_mlists : d_hlist + 64;
        const uint32_t nsets = npoints;
        ZG_TRY(h2d_list(p, d_lists, plan->lists));
        if (multi)
            ZG_TRY(poly_combine_pairs(ctx, polys, p->d_pc, d_lists, plan->firsts.data(), plan->counts.data(), nsets, p->wpoly, (size_t)2 * n, n));
        else
            ZG_TRY(poly_horner_combine_sets(ctx, polys, p->d_pc, nb, d_lists, 512, plan->counts.data(), nsets, p->wpoly, (size_t)2 * n, wp_bs, n));
        // one batched kate_division: poly s at wpoly[2s], quotient at wpoly[2s+1]
        ZG_TRY(poly_kate_division(ctx, p->d_pc, nq, plan->slots.data(), nsets, p->wpoly, (size_t)2 * n, wp_bs, p->wpoly + n, (size_t)2 * n,
                                  wp_bs, p->ktmp, n));
        // the witness polynomials sit at odd slots: stride 2n
        ctx->msm_dense_hint = true;  // (so are the opening quotients)
        const int st_w = commit(p, phase_msm(dense_g(p), p->wpoly + n, (size_t)2 * n, nsets, wp_bs, nq), W_GWC);
        ctx->msm_dense_hint = false;
        ZG_TRY(st_w);
        ZG_TICK("gwc: queued");
        return ZG_OK;
    }
    int openings_absorb() {
        if (shplonk) return shplonk_finish();
        const uint32_t nsets = npoints;
        ZG_TRY(wait_points(p, (size_t)nq * nsets, pts, W_GWC));
        ZG_TICK("gwc: points on the host");
        for (uint32_t b = 0; b < nq; b++)
            for (uint32_t s = 0; s < nsets; s++) tr[b].write_point(pts[(size_t)b * nsets + s]);
        return ZG_OK;
    }

    // x[i] <- 1 / x[i] with ONE field inversion (Montgomery's trick; no entry is zero: differences of distinct points)
    static void invert_all(std::vector<Fe>& x) {
        std::vector<Fe> pre(x.size());
        Fe acc = Fr::one();
        for (size_t i = 0; i < x.size(); i++) {
            pre[i] = acc;
            acc = Fr::mul(acc, x[i]);
        }
        Fe inv = Fr::inv(acc);
        for (size_t i = x.size(); i-- > 0;) {
            const Fe xi = x[i];
            x[i] = Fr::mul(inv, pre[i]);
            inv = Fr::mul(inv, xi);
        }
    }
    static F9 coef9(const Fe& c) { return f9_unpack(Fr::mul(c, Fr9Params::c261_fe())); }
    // the two tables of a half, every proof's, to the device (behind the work already queued)
    int shplonk_upload(const std::vector<F9>& coef, const std::vector<Fe>& corr) {
        std::vector<F9> padded(coef);
        while (padded.size() * sizeof(F9) % 16) padded.push_back(F9{});  // (whole 16-byte words: h2d's kernel form)
        ZG_TRY(h2d(p, p->sh_coef, padded.data(), padded.size() * sizeof(F9)));
        return h2d(p, p->sh_corr, corr.data(), corr.size() * sizeof(Fe));
    }
    // y, v, then per proof the numerators' coefficients: y^j v^i c_(i,r) on commitment j of set i in the list of point r,
    // c_(i,r) = 1 / prod_(p in S_i, p != r) (r - p), and the low coefficients of sum_(i: r in S_i) v^i c_(i,r) R_i(X),
    // R_i = sum_j y^j R_ij the interpolant of the y-combined evaluations on S_i (the host holds them: eval_batch's place)
    int shplonk_numerator_tables() {
        const uint32_t np = ntr, nT = npoints;
        const ProofLayout& l = plan->lay;
        const std::vector<ProofLayout::RotationSet>& ssets = l.rsets;
        const size_t sh_ncoef = plan->sh_ncoef;
        sproof.assign(np, SProof{});
        std::vector<F9> coef((size_t)np * sh_ncoef, F9{});
        std::vector<Fe> corr((size_t)np * nT * PC_MAX_POINTS, fe_zero());
        for (uint32_t b = 0; b < np; b++) {
            SProof& sp = sproof[b];
            sp.y = tr[b].squeeze();
            sp.v = tr[b].squeeze();
            const Fe* pt = p->hpc[b].points;
            sp.R.resize(ssets.size());
            std::vector<std::vector<Fe>> cinv(ssets.size());
            {  // every c_(i,a) of the proof under one inversion
                std::vector<Fe> den;
                for (const ProofLayout::RotationSet& s : ssets)
                    for (size_t a = 0; a < s.points.size(); a++) {
                        Fe d = Fr::one();
                        for (size_t c = 0; c < s.points.size(); c++)
                            if (c != a) d = Fr::mul(d, Fr::sub(pt[s.points[a]], pt[s.points[c]]));
                        den.push_back(d);
                    }
                invert_all(den);
                size_t at = 0;
                for (size_t i = 0; i < ssets.size(); i++) {
                    cinv[i].assign(den.begin() + at, den.begin() + at + ssets[i].points.size());
                    at += ssets[i].points.size();
                }
            }
            Fe vi = Fr::one();
            for (size_t i = 0; i < ssets.size(); i++, vi = Fr::mul(vi, sp.v)) {
                const ProofLayout::RotationSet& s = ssets[i];
                const size_t m = s.points.size();
                sp.R[i].assign(m, fe_zero());
                for (size_t a = 0; a < m; a++) {
                    Fe e = fe_zero(), yj = Fr::one();  // the y-combined evaluation at this point
                    for (uint32_t c : s.coms) {
                        e = Fr::add(e, Fr::mul(yj, ev(b, l.queries[l.coms[c].queries[a]].eval)));
                        yj = Fr::mul(yj, sp.y);
                    }
                    // e c_(i,a) prod_(c != a) (X - p_c) into R_i
                    std::vector<Fe> num(1, Fr::mul(e, cinv[i][a]));
                    for (size_t c = 0; c < m; c++) {
                        if (c == a) continue;
                        num.push_back(fe_zero());
                        for (size_t d2 = num.size() - 1; d2 > 0; d2--) num[d2] = Fr::sub(num[d2 - 1], Fr::mul(num[d2], pt[s.points[c]]));
                        num[0] = Fr::neg(Fr::mul(num[0], pt[s.points[c]]));
                    }
                    for (size_t d2 = 0; d2 < m; d2++) sp.R[i][d2] = Fr::add(sp.R[i][d2], num[d2]);
                }
            }
            for (uint32_t o = 0; o < nT; o++) {
                F9* cf = &coef[(size_t)b * sh_ncoef + plan->firsts[o]];
                Fe* cr = &corr[((size_t)b * nT + o) * PC_MAX_POINTS];
                size_t at = 0;
                vi = Fr::one();
                for (size_t i = 0; i < ssets.size(); i++, vi = Fr::mul(vi, sp.v)) {
                    const ProofLayout::RotationSet& s = ssets[i];
                    if (!(plan->set_mask[i] >> o & 1u)) continue;
                    size_t a = 0;
                    while (s.points[a] != o) a++;
                    const Fe w = Fr::mul(vi, cinv[i][a]);
                    Fe wy = w;
                    for (size_t j = 0; j < s.coms.size(); j++, wy = Fr::mul(wy, sp.y)) cf[at++] = coef9(wy);
                    for (size_t d2 = 0; d2 < sp.R[i].size(); d2++) cr[d2] = Fr::add(cr[d2], Fr::mul(w, sp.R[i][d2]));
                }
            }
        }
        ZG_TICK("y, v (multi-open)");
        ZG_TRY(shplonk_upload(coef, corr));
        lap(4);
        return ZG_OK;
    }
    // h1 = sum_i v^i N_i / Z_(S_i) as |T| first-order divisions: per point r the combination sum_(i: r in S_i) v^i c_(i,r) N_i
    // (one launch for all of them), the batched Kate division by (X - r), and the sum of the quotients
    int shplonk_h1_queue() {
        const uint32_t np = ntr, nT = npoints;
        ZG_TRY(h2d_list(p, p->sh_lists, plan->lists));
        ZG_TRY(poly_combine_weighted(ctx, polys, np, p->sh_lists, plan->firsts.data(), plan->counts.data(), nT, p->sh_coef, plan->sh_ncoef, p->sh_corr,
                                     PC_MAX_POINTS, (size_t)nT * PC_MAX_POINTS, nullptr, 0, p->wpoly, (size_t)2 * n, wp_bs, n));
        ZG_TRY(poly_kate_division(ctx, p->d_pc, np, plan->slots.data(), nT, p->wpoly, (size_t)2 * n, wp_bs, p->wpoly + n, (size_t)2 * n, wp_bs,
                                  p->ktmp, n));
        ZG_TRY(poly_sum_rows(ctx, np, p->wpoly + n, (size_t)2 * n, wp_bs, nT, p->sh_h1, n, n));
        ctx->msm_dense_hint = true;
        const int st_c = commit(p, phase_msm(dense_g(p), p->sh_h1, n, 1, n, np), W_GWC);
        ctx->msm_dense_hint = false;
        ZG_TRY(st_c);
        ZG_TICK("h1: queued");
        return ZG_OK;
    }
    // h1 -> u; L = sum_i v^i z_i sum_j y^j (P_ij - R_ij(u)) - Z_T(u) h1 with every coefficient already over z_0; h2 = L / (X - u)
    int shplonk_finish() {
        const uint32_t np = ntr, nT = npoints, oL = nT;
        const std::vector<ProofLayout::RotationSet>& ssets = plan->lay.rsets;
        const size_t sh_ncoef = plan->sh_ncoef;
        ZG_TRY(wait_points(p, np, pts, W_GWC));
        ZG_TICK("h1 on the host");
        std::vector<F9> coef((size_t)np * sh_ncoef, F9{});
        std::vector<Fe> corr(np, fe_zero());
        Fe u{};
        for (uint32_t b = 0; b < nb; b++) {
            if (b < np) {
                tr[b].write_point(pts[b]);
                u = tr[b].squeeze();
            }
            p->hpc[b].points[PC_U_SLOT] = u;
        }
        std::vector<Fe> z0inv_all(np);  // every proof's 1 / z_0 under one inversion
        for (uint32_t b = 0; b < np; b++) {
            const Fe* pt = p->hpc[b].points;
            Fe z0 = Fr::one();
            for (uint32_t r = 0; r < nT; r++)
                if (!(plan->set_mask[0] >> r & 1u)) z0 = Fr::mul(z0, Fr::sub(pt[PC_U_SLOT], pt[r]));
            z0inv_all[b] = z0;
        }
        invert_all(z0inv_all);
        for (uint32_t b = 0; b < np; b++) {
            const SProof& sp = sproof[b];
            const Fe* pt = p->hpc[b].points;
            const Fe ub = pt[PC_U_SLOT];
            Fe zT = Fr::one();
            for (uint32_t r = 0; r < nT; r++) zT = Fr::mul(zT, Fr::sub(ub, pt[r]));
            std::vector<Fe> z(ssets.size(), Fr::one());
            for (size_t i = 0; i < ssets.size(); i++)
                for (uint32_t r = 0; r < nT; r++)
                    if (!(plan->set_mask[i] >> r & 1u)) z[i] = Fr::mul(z[i], Fr::sub(ub, pt[r]));
            const Fe z0inv = z0inv_all[b];
            F9* cf = &coef[(size_t)b * sh_ncoef];
            size_t at = 0;
            Fe vi = Fr::one(), rsum = fe_zero();
            for (size_t i = 0; i < ssets.size(); i++, vi = Fr::mul(vi, sp.v)) {
                const Fe w = Fr::mul(Fr::mul(vi, z[i]), z0inv);
                Fe wy = w;
                for (size_t j = 0; j < ssets[i].coms.size(); j++, wy = Fr::mul(wy, sp.y)) cf[at++] = coef9(wy);
                Fe ru = fe_zero();  // R_i(u)
                for (size_t d2 = sp.R[i].size(); d2-- > 0;) ru = Fr::add(Fr::mul(ru, ub), sp.R[i][d2]);
                rsum = Fr::add(rsum, Fr::mul(w, ru));
            }
            cf[at] = coef9(Fr::neg(Fr::mul(zT, z0inv)));
            corr[b] = rsum;
        }
        ZG_TICK("u");
        ZG_TRY(publish());
        ZG_TRY(shplonk_upload(coef, corr));
        const uint32_t firstL = 0;  // (L's coefficients start the table of this half; its list is the last one)
        ZG_TRY(poly_combine_weighted(ctx, polys, np, p->sh_lists + plan->firsts[oL], &firstL, &plan->counts[oL], 1, p->sh_coef, sh_ncoef, p->sh_corr, 1,
                                     1, p->sh_h1, n, p->wpoly, (size_t)2 * n, wp_bs, n));
        const uint32_t uslot = PC_U_SLOT;
        ZG_TRY(poly_kate_division(ctx, p->d_pc, np, &uslot, 1, p->wpoly, (size_t)2 * n, wp_bs, p->wpoly + n, (size_t)2 * n, wp_bs, p->ktmp, n));
        ctx->msm_dense_hint = true;
        const int st_c = commit(p, phase_msm(dense_g(p), p->wpoly + n, (size_t)2 * n, 1, wp_bs, np), W_GWC);
        ctx->msm_dense_hint = false;
        ZG_TRY(st_c);
        ZG_TICK("h2: queued");
        ZG_TRY(wait_points(p, np, pts, W_GWC));
        for (uint32_t b = 0; b < np; b++) tr[b].write_point(pts[b]);
        return ZG_OK;
    }
    int finish() {
        int first_bad = ZG_OK;
        if (gate_failed()) {  // (every gate kernel has ended: the last commitments came from behind them)
            set_error(hold.yielded ? "zg_prover_prove: a phase queued ahead of its challenge had to allocate or synchronise; its gate was let go (ZG_LAT_GATE)"
                                   : "zg_prover_prove: a phase waited more than 4 s for its challenge and ran without it (ZG_LAT_GATE)");
            gate_gave_up = true;  // (nothing is handed out: prove_batch_impl makes the proof again in the plain order)
            p->in_flight = false;
            return ZG_ERR_HIP;
        }
        for (uint32_t b = 0; b < ntr; b++) {
            if (status[b] == ZG_OK && tr[b].failed()) {
                set_error("zg_prover_prove: a commitment of proof %u is the identity point; %s cannot absorb it", b, tr[b].name());
                status[b] = ZG_ERR_INVALID_ARG;
            }
            if (status[b] == ZG_OK && tr[b].stream().size() > proof_cap) {
                set_error("zg_prover_prove: proof buffer too small (%zu > %zu)", tr[b].stream().size(), proof_cap);
                status[b] = ZG_ERR_INVALID_ARG;
            }
            if (status[b] == ZG_OK) {
                memcpy(proofs[b], tr[b].stream().data(), tr[b].stream().size());
                proof_lens[b] = tr[b].stream().size();
            } else {
                proof_lens[b] = 0;
                if (first_bad == ZG_OK) first_bad = status[b];
            }
            if (statuses) statuses[b] = status[b];
        }
        ZG_TICK("proof bytes out");
        lap(5);
        p->phase_ms[6] = std::chrono::duration<double, std::milli>(clk::now() - t_start).count();
        p->in_flight = false;
        p->warm_sig = first_bad == ZG_OK ? form_sig() : 0;
        return first_bad;
    }
};

static int prove_batch_impl(zg_prover* p, size_t count, const zg_fr* const* advice_host, void* const* advice_dev,
                            const zg_fr* const* instance, size_t instance_len, const uint8_t* keys /* [count][32] */,
                            uint8_t* const* proofs, size_t proof_cap, size_t* proof_lens, int* statuses, zg_phase_fn phase_fn = nullptr,
                            void* phase_user = nullptr) {
    ZG_REQUIRE(p && proofs && proof_lens && keys, ZG_ERR_INVALID_ARG, "zg_prover_prove: null argument");
    ZG_TRY(batch_args_ok("zg_prover_prove", "proofs", p, count, instance, instance_len));
    ZG_REQUIRE(phase_fn || p->n_phases == 1, ZG_ERR_INVALID_ARG,
               "zg_prover_prove: the circuit has advice columns in %u phases, whose witness depends on challenges: use zg_prover_prove_phased",
               p->n_phases);
    ZG_REQUIRE(!p->phased() || (p->world <= 1 && !p->rccl_comm), ZG_ERR_UNSUPPORTED,
               "zg_prover_prove: advice phases and challenges are not made on a point-range shard of the SRS");
    ZG_REQUIRE(p->multiopen != ZG_MULTIOPEN_SHPLONK || (p->world <= 1 && !p->rccl_comm), ZG_ERR_UNSUPPORTED,
               "zg_prover_prove: the SHPLONK multi-open is not made on a point-range shard of the SRS");
    ZG_REQUIRE(p->pk->NS == 0 || (p->world <= 1 && !p->rccl_comm), ZG_ERR_UNSUPPORTED,
               "zg_prover_prove: a circuit with shuffles is not proved on a point-range shard of the SRS");
    ZG_REQUIRE(p->world > 1 || p->shard_n == p->pk->n, ZG_ERR_INVALID_ARG,
               "zg_prover_prove: the base sets hold %u of %u points and no shard was declared (zg_prover_set_shard)", p->shard_n, p->pk->n);
    ZG_ENTER(p->ctx);
    {
        ProveBatch job(p, count, advice_host, advice_dev, instance, instance_len, keys, proofs, proof_cap, proof_lens, statuses);
        job.phase_fn = phase_fn;
        job.phase_user = phase_user;
        const int st = job.run();
        if (!job.gate_gave_up) return st;
    }
    // A gate ran into its time limit (the host thread was away for seconds, or a stream that shares a hardware queue with
    // this prover's stood in the way -- LAT_GATE_DEFAULT): the phases behind it ran on the previous challenge.  The inputs
    // are where they were (the blinding rows are a function of the key): the same proof again, every phase after its challenge.
    ProveBatch again(p, count, advice_host, advice_dev, instance, instance_len, keys, proofs, proof_cap, proof_lens, statuses);
    again.no_gate = true;
    return again.run();
}

// create_proof for a `circuits` slice: ONE proof of `circuits` instances of the circuit (ProveBatch::multi).  One circuit is
// the single-proof path, byte for byte.  `who`: zg_prover_prove_multi, which keeps to circuits without challenges, later
// phases and -- for more than one circuit -- shuffles (`general` = false), or zg_prover_prove_circuits*, which takes them
// all; on a circuit that has none of the three the two are one path.
static int prove_multi_impl(const char* who, bool general, zg_prover* p, size_t circuits, const zg_fr* const* advice_host,
                            void* const* advice_dev, const zg_fr* const* instance, size_t instance_len,
                            const uint8_t* keys /* [circuits][32] */, uint8_t* proof, size_t proof_cap, size_t* proof_len,
                            zg_phase_fn phase_fn = nullptr, void* phase_user = nullptr) {
    ZG_REQUIRE(p && proof && proof_len && keys, ZG_ERR_INVALID_ARG, "%s: null argument", who);
    *proof_len = 0;
    ZG_TRY(batch_args_ok(who, "circuits", p, circuits, instance, instance_len));
    ZG_REQUIRE(general || !p->phased(), ZG_ERR_UNSUPPORTED, "%s: not for a circuit with challenges or advice phases (zg_prover_prove_circuits*)", who);
    ZG_REQUIRE(general || circuits == 1 || p->pk->NS == 0, ZG_ERR_UNSUPPORTED,
               "%s: several circuits in one proof, not for a circuit with shuffles (zg_prover_prove_circuits*)", who);
    ZG_REQUIRE(phase_fn || p->n_phases == 1, ZG_ERR_INVALID_ARG,
               "%s: the circuit has advice columns in %u phases, whose witness depends on challenges: use zg_prover_prove_circuits_phased", who,
               p->n_phases);
    uint8_t* out[1] = {proof};
    if (circuits == 1)
        return prove_batch_impl(p, 1, advice_host, advice_dev, instance, instance_len, keys, out, proof_cap, proof_len, nullptr, phase_fn, phase_user);
    ZG_REQUIRE(p->world <= 1 && !p->rccl_comm, ZG_ERR_UNSUPPORTED, "%s: not on a point-range shard of the SRS", who);
    ZG_REQUIRE(circuits <= FOLD_MAX_SLOTS, ZG_ERR_UNSUPPORTED, "%s: %zu circuits in one proof (max %u)", who, circuits, FOLD_MAX_SLOTS);
    ZG_REQUIRE(p->shard_n == p->pk->n, ZG_ERR_INVALID_ARG, "%s: the base sets hold %u of %u points", who, p->shard_n, p->pk->n);
    ZG_ENTER(p->ctx);
    ProveBatch job(p, circuits, advice_host, advice_dev, instance, instance_len, keys, out, proof_cap, proof_len, nullptr, true);
    job.phase_fn = phase_fn;
    job.phase_user = phase_user;
    return job.run();  // (never gated: the gate is a lone proof's)
}

size_t zg_prover_proof_size_multi(const zg_prover* p, size_t circuits) {
    if (!p || !circuits) return 0;
    return proof_size_bound(proof_shape(*p->pk), (uint32_t)circuits, p->multiopen == ZG_MULTIOPEN_SHPLONK, p->transcript == ZG_TRANSCRIPT_BLAKE2B);
}

int zg_prover_prove_multi(zg_prover* p, size_t circuits, const zg_fr* const* advice, const zg_fr* const* instance, size_t instance_len,
                          const uint8_t* rng_keys, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
    return prove_multi_impl("zg_prover_prove_multi", false, p, circuits, advice, nullptr, instance, instance_len, rng_keys, proof, proof_cap,
                            proof_len);
}

int zg_prover_prove_multi_dev(zg_prover* p, size_t circuits, void* const* d_advice, const zg_fr* const* instance, size_t instance_len,
                              const uint8_t* rng_keys, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
    return prove_multi_impl("zg_prover_prove_multi", false, p, circuits, nullptr, d_advice, instance, instance_len, rng_keys, proof, proof_cap,
                            proof_len);
}

// ... for every circuit the library proves: shuffles, challenges and advice phases included
int zg_prover_prove_circuits(zg_prover* p, size_t circuits, const zg_fr* const* advice, const zg_fr* const* instance, size_t instance_len,
                             const uint8_t* rng_keys, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
    return prove_multi_impl("zg_prover_prove_circuits", true, p, circuits, advice, nullptr, instance, instance_len, rng_keys, proof, proof_cap,
                            proof_len);
}

int zg_prover_prove_circuits_dev(zg_prover* p, size_t circuits, void* const* d_advice, const zg_fr* const* instance, size_t instance_len,
                                 const uint8_t* rng_keys, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
    return prove_multi_impl("zg_prover_prove_circuits", true, p, circuits, nullptr, d_advice, instance, instance_len, rng_keys, proof, proof_cap,
                            proof_len);
}

int zg_prover_prove_circuits_phased(zg_prover* p, size_t circuits, zg_phase_fn fn, void* user, const zg_fr* const* instance,
                                    size_t instance_len, const uint8_t* rng_keys, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
    ZG_REQUIRE(p && fn, ZG_ERR_INVALID_ARG, "zg_prover_prove_circuits_phased: null argument");
    // (the slots hold the columns: the callback writes them, phase by phase)
    return prove_multi_impl("zg_prover_prove_circuits_phased", true, p, circuits, nullptr, nullptr, instance, instance_len, rng_keys, proof,
                            proof_cap, proof_len, fn, user);
}

int zg_prover_prove_batch(zg_prover* p, size_t count, const zg_fr* const* advice, const zg_fr* const* instance,
                          size_t instance_len, const uint8_t* rng_keys, uint8_t* const* proofs, size_t proof_cap,
                          size_t* proof_lens, int* statuses) {
    return prove_batch_impl(p, count, advice, nullptr, instance, instance_len, rng_keys, proofs, proof_cap, proof_lens, statuses);
}

int zg_prover_prove_batch_dev(zg_prover* p, size_t count, void* const* d_advice, const zg_fr* const* instance,
                              size_t instance_len, const uint8_t* rng_keys, uint8_t* const* proofs, size_t proof_cap,
                              size_t* proof_lens, int* statuses) {
    return prove_batch_impl(p, count, nullptr, d_advice, instance, instance_len, rng_keys, proofs, proof_cap, proof_lens, statuses);
}

int zg_prover_prove_phased(zg_prover* p, size_t count, zg_phase_fn fn, void* user, const zg_fr* const* instance, size_t instance_len,
                           const uint8_t* rng_keys, uint8_t* const* proofs, size_t* proof_lens) {
    ZG_REQUIRE(p && fn, ZG_ERR_INVALID_ARG, "zg_prover_prove_phased: null argument");
    // (the slots hold the columns: the callback writes them, phase by phase)
    return prove_batch_impl(p, count, nullptr, nullptr, instance, instance_len, rng_keys, proofs, zg_prover_proof_size(p), proof_lens, nullptr, fn,
                            user);
}

int zg_prover_prove_dev(zg_prover* p, void* d_advice, const zg_fr* instance, size_t instance_len, const uint8_t rng_key[32],
                        uint8_t* proof, size_t proof_cap, size_t* proof_len) {
    ZG_REQUIRE(p && proof && proof_len && rng_key && (d_advice || p->pk->A == 0), ZG_ERR_INVALID_ARG, "zg_prover_prove: null argument");
    void* adv[1] = {d_advice};
    const zg_fr* inst[1] = {instance};
    uint8_t* out[1] = {proof};
    return prove_batch_impl(p, 1, nullptr, adv, instance ? inst : nullptr, instance_len, rng_key, out, proof_cap, proof_len, nullptr);
}

int zg_prover_prove(zg_prover* p, const zg_fr* advice, const zg_fr* instance, size_t instance_len, const uint8_t rng_key[32],
                    uint8_t* proof, size_t proof_cap, size_t* proof_len) {
    ZG_REQUIRE(p && proof && proof_len && rng_key && (advice || p->pk->A == 0), ZG_ERR_INVALID_ARG, "zg_prover_prove: null argument");
    const zg_fr* adv[1] = {advice};
    const zg_fr* inst[1] = {instance};
    uint8_t* out[1] = {proof};
    return prove_batch_impl(p, 1, adv, nullptr, instance ? inst : nullptr, instance_len, rng_key, out, proof_cap, proof_len, nullptr);
}

}  // extern "C"
