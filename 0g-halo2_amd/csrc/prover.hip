// The prover object and its proving key: zg_prover_create* (keygen_pk's derived data in HBM, the base tables and the
// extended-domain policy), fork / destroy, the per-proof slots, the latency / throughput forms, the digit tables, fetch,
// the vk commitments and evaluate_h's host side.  create_proof itself is prove_batch.hip.
#include <algorithm>
#include <cstdlib>
#include <memory>

#include "prover.h"
#include "field9.h"

using namespace zg;

namespace {

// A lone proof of a LARGER circuit is bound by work, not by launches: from this size on it takes the quotient from the
// split domain as the throughput form does (39n instead of 68n butterflies per polynomial, 5n instead of 8n evaluate_h
// rows), its coset transforms still phase by phase on the side stream.  gpurun_out/lone_forms3/4.txt -> profiles/r03/
// lone_forms.txt: k = 14 2.96 -> 3.10 ms (the interpolation's extra launches), k = 15 4.24 -> 4.19 (small) and 4.34 ->
// 4.33 (medium), k = 17 11.74 -> 10.39.  (The bit-position tables lose at every size for a lone proof -- k = 17: 11.57 ->
// 11.74 -- and stay a throughput-form choice.)
constexpr int LAT_SPLIT_K_DEFAULT = 15;

template <class T>
int dalloc_into(std::vector<void*>& owned, T** out, size_t count) {
    void* q = nullptr;
    size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        set_error("zg_prover: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return ZG_ERR_OOM;
    }
    owned.push_back(q);
    *out = reinterpret_cast<T*>(q);
    return ZG_OK;
}

// Digit width of the free-position form for the run-form commitments against g_lagrange (the sorted a' / s' columns and
// the products: full-size coefficients wherever a row changes something, but half-empty vectors -- so the width that
// keeps the bucket count of the window form, c + 1: 254 / (c + 2) digits per coefficient instead of 255 / c windows.
// Same-box A/B at k = 14: 0.7122 -> 0.7060 ms/proof at 13; 12: 0.718, 14: 0.722; 15, the random vectors' width: 0.740.)
// ZG_MSM_NAF_GL = width, 0 = the window form; fixed when the prover is created (zg_prover::naf_gl_w).
static uint32_t naf_gl_default(const zg_bases* gl) {
    const int v = knob(K_MSM_NAF_GL);
    if (v >= 0) return v >= 3 && v <= 16 ? (uint32_t)v : 0u;
    const uint32_t w = gl->c + 1;
    return w >= 3 && w <= 16 ? w : 0u;
}

static bool lone_split(const zg_prover* p, bool latency_form) {
    const int sk = knob(K_LAT_SPLIT_K);
    return latency_form && p->pk->k >= (uint32_t)(sk >= 0 ? sk : LAT_SPLIT_K_DEFAULT);
}

}  // namespace

namespace zg {

// the scalars evaluate_h reads, in the form it computes in (theta, beta, gamma already in c)
// terms of evaluate_h after the gates: permutation (l0, llast, one l0 per further set, one lactive per set) and five per
// lookup; 0 when they are too many for ProofConst::eh_ypow (or switched off): the kernel then folds in y term by term
uint32_t evalh_terms(const PkDev& pk) {
    const bool grouped = pk.grouped;
    const uint32_t t = (pk.sets ? 2 + (pk.sets - 1) + pk.sets : 0) + 5 * pk.NL;
    // (at most 40: the sums that multiply l0 / lactive then stay below the operand bound of Fr9::mul2)
    return grouped && pk.hat && t >= 1 && t <= 40 && t + 1 <= EH_MAX_YPOW ? t : 0;
}

// The default (grouped, nine-limb) kernel divides both factors of a permutation column by K = beta delta^col zeta^a:
// (beta sigma + v + gamma) / K = sigma_sc + t and (v + beta delta^col zeta^a w^i + gamma) / K = w^i + t with
// t = (v + gamma) K^-1 -- three products per column instead of four and no delta chain; the set's term gets prod K back
// in its weight.  Needs the sigma_sc slabs of the key and room in ProofConst for the circuit's columns and sets.
bool evalh_perm_scaled(const PkDev& pk) {
    return evalh_terms(pk) != 0 && pk.P >= 1 && pk.P <= EH_MAX_PCOLS && pk.sets <= EH_MAX_PSETS;
}

void evalh_consts(ProofConst& c, const Fe& y, const PkDev& pk) {
    const bool hat = pk.hat;
    const uint32_t n_terms = evalh_terms(pk);
    const Fe zeta = pk.zeta, zeta2 = Fr::sqr(zeta);
    c.eh_y = y; c.eh_beta = c.beta; c.eh_gamma = c.gamma; c.eh_theta = c.theta;
    c.eh_delta_start[0] = Fr::mul(c.beta, zeta);   // beta * coset shift
    c.eh_delta_start[1] = Fr::mul(c.beta, zeta2);
    c.eh_scaled = 0;
    if (pk.NS) {  // (the shuffle pass over h: its three terms per shuffle stand last, everything before them moves up)
        c.sh_y = y;
        c.sh_ypow = Fr::pow_u64(y, 3 * pk.NS);
    }
    if (hat) {
        const Fe c261 = Fr9Params::c261_fe();
        for (Fe* cst : {&c.eh_y, &c.eh_beta, &c.eh_gamma, &c.eh_theta, &c.eh_delta_start[0], &c.eh_delta_start[1]})
            *cst = Fr::mul(*cst, c261);
        Fe ypw[EH_MAX_YPOW];
        Fe pw = Fr::one();
        // (with the terms by degree the gates are weighted from this table too: up to y^(n_terms + gates - 1))
        const uint32_t top = n_terms + (pk.qt.active ? pk.NG : 0u);
        for (uint32_t j = 0; j <= top && j < EH_MAX_YPOW; j++) {
            ypw[j] = pw;
            c.eh_ypow[j] = Fr::mul(pw, c261);
            pw = Fr::mul(pw, y);
        }
        if (evalh_perm_scaled(pk) && !fe_is_zero(c.beta)) {  // (beta = 0 has no inverse: that proof's rows take the unscaled term)
            const Fe shift[2] = {zeta, zeta2}, shift_inv[2] = {zeta2, zeta};  // (zeta^3 = 1)
            const Fe beta_inv = Fr::inv(c.beta), delta = fr_delta();
            Fe dpow = Fr::one(), dipow = Fr::one();
            for (uint32_t s = 0; s < pk.sets; s++) {
                Fe prod[2] = {Fr::one(), Fr::one()};
                for (uint32_t col = s * pk.chunk; col < std::min(pk.P, (s + 1) * pk.chunk); col++) {
                    for (int a = 0; a < 2; a++) {
                        c.eh_pcol[a][col] = Fr::mul(Fr::mul(Fr::mul(beta_inv, dipow), shift_inv[a]), c261);
                        prod[a] = Fr::mul(prod[a], Fr::mul(Fr::mul(c.beta, dpow), shift[a]));
                    }
                    dpow = Fr::mul(dpow, delta);
                    dipow = Fr::mul(dipow, pk.delta_inv);
                }
                // set s's term is the kernel's term number n_terms - sets - 2 - s counted from the last (evaluate_h9_kernel)
                const uint32_t e = n_terms - pk.sets - 2 - s;
                for (int a = 0; a < 2; a++) c.eh_pw[a][s] = Fr::mul(Fr::mul(ypw[e], prod[a]), c261);
            }
            c.eh_scaled = 1;
        }
    }
}

// evaluate_h's arguments for part `di` of the extended domain: the proving key's slabs, the per-proof slabs of this
// prover's slots (proof b at b * cos_bs), scalars from d_pc
EvalHArgs evalh_args(const zg_prover* p, uint32_t di) {
    const PkDev& pk = *p->pk;
    const uint32_t n = pk.n, k = pk.k, bf = pk.bf, A = pk.A, I = pk.I, NL = pk.NL, S = pk.sets;
    const bool hat = pk.hat;
    const PkDev::Dom& d = pk.dom[di];
    const Fe* cos = p->dbuf[di].cos;
    EvalHArgs a;
    memset(&a, 0, sizeof(a));
    a.c = pk.dc;
    a.cols.fixed = d.fixed_cos; a.cols.advice = cos; a.cols.instance = cos + (size_t)A * d.en;
    a.cols.log_size = d.ek; a.cols.rot_scale = (int32_t)(d.en / n);
    a.cols.adv_bs = a.cols.inst_bs = (size_t)p->ncos * d.en;
    a.sigma_cos = d.sigma_cos;
    a.sigma_sc = d.sigma_sc;
    a.pz_cos = cos + (size_t)(A + I) * d.en;
    a.lz_cos = a.pz_cos + (size_t)S * d.en;
    // the a'/s' cosets are interleaved, [2l] = a'_l and [2l+1] = s'_l: two views with a stride of two slabs
    a.pin_cos = a.lz_cos + (size_t)NL * d.en; a.ptab_cos = a.pin_cos + d.en; a.perm_stride = (size_t)2 * d.en;
    a.l0 = d.l0; a.llast = d.llast; a.lactive = d.lactive;
    a.ext_tw = hat ? d.ext_tw + d.en : d.ext_tw;  // (the twiddle table's second half is the 2^261 form)
    a.t_eval = d.t_eval; a.t_mask = (1u << (d.ek - k)) - 1;
    a.last_rot = -(int32_t)(bf + 1);
    a.pc = p->d_pc; a.zpow = (uint32_t)d.zpow;
    a.cos_bs = (size_t)p->ncos * d.en; a.h_bs = d.en;
    a.delta = hat ? Fr::mul(fr_delta(), Fr9Params::c261_fe()) : fr_delta();
    a.hat = hat;
    a.monos_hat = pk.monos_hat;
    a.n_terms = evalh_terms(pk);
    a.gates_hat = pk.gates_hat;
    a.gate_common = pk.gate_common;
    a.gate_uni = pk.gate_uni;
    a.uni_coef = pk.uni_coef;
    a.gate_slab = pk.gate_slab;
    a.gate_slabs = d.gate_slabs;
    a.h = p->dbuf[di].h;
    a.gate_cls = pk.qt.gate_cls; a.tail_lo = pk.qt.tail_lo; a.tail_hi = pk.qt.tail_hi;
    a.set_hi = pk.qt.set_mask; a.lk_hi = pk.qt.lk_mask;
    a.h_hi = di == 1 ? p->h_hi : nullptr;
    return a;
}

}  // namespace zg

namespace {

void free_slots(zg_prover* p) {
    for (void* q : p->slot_owned) (void)hipFree(q);
    p->slot_owned.clear();
    p->sh_h1 = nullptr;  // (SHPLONK's buffers went with the slots)
    if (p->pin.host) (void)hipHostFree(p->pin.host);
    p->pin = PinnedArena{};
    p->gate_seq = 0;  // (the gate word goes with the arena: a new one starts at zero, and a gate opens at its number or later)
    p->cap = 0;
    p->uploaded_lists.clear();
    p->plans.clear();  // (their limits were the slots')
    p->warm_sig = 0;  // (new buffers: the next proof is a first proof again -- ProveBatch::gate_wanted)
}

int alloc_slots_impl(zg_prover* p, uint32_t cap);
// (re)allocates every per-proof buffer for `cap` proofs in flight; on failure the prover is left without slots
// (zg_prover_prove* then refuse with "0 slots") rather than with half of them
int alloc_slots(zg_prover* p, uint32_t cap) {
    const int st = alloc_slots_impl(p, cap);
    if (st != ZG_OK) free_slots(p);
    return st;
}
int alloc_slots_impl(zg_prover* p, uint32_t cap) {
    const PkDev& k = *p->pk;
    ZG_REQUIRE(cap >= 1 && cap <= 1024, ZG_ERR_INVALID_ARG, "zg_prover: batch of %u proofs", cap);
    free_slots(p);
    auto& own = p->slot_owned;
    const uint32_t n = k.n, F = k.F, A = k.A, I = k.I, P = k.P, NL = k.NL, S = k.sets, Q = k.qpd;
    (void)F;
    p->cap = cap;
    const uint32_t NS = k.NS;
    p->ncos = A + I + S + NL + 2 * NL + NS;
    p->npp = p->ncos + 1 + Q + 1;
    p->nsh = k.F + P;
    p->ix_fixed = 0; p->ix_sigma = k.F; p->ix_adv = p->nsh; p->ix_inst = p->ix_adv + A; p->ix_pz = p->ix_inst + I;
    p->ix_lz = p->ix_pz + S; p->ix_perm = p->ix_lz + NL; p->ix_sz = p->ix_perm + 2 * NL; p->ix_random = p->ix_sz + NS;
    p->ix_hpiece = p->ix_random + 1; p->ix_hpoly = p->ix_hpiece + Q;
    const size_t c = cap;
    ZG_TRY(dalloc_into(own, &p->pp, c * p->npp * n));
    for (uint32_t di = 0; di < k.nparts; di++) {
        // (one block per proof, in the order of the coefficient slab: advice, instance, permutation z, lookup z, a'/s'
        //  -- the split form transforms all of them in one batch)
        ZG_TRY(dalloc_into(own, &p->dbuf[di].cos, c * p->ncos * k.dom[di].en));
        ZG_TRY(dalloc_into(own, &p->dbuf[di].h, c * k.dom[di].en));
    }
    if (k.nparts == 3) ZG_TRY(dalloc_into(own, &p->split_tmp, c * 3 * k.dom[2].en));
    p->h_hi = nullptr;
    if (k.qt.active) ZG_TRY(dalloc_into(own, &p->h_hi, c * k.dom[1].en));
    ZG_TRY(dalloc_into(own, &p->adv_val, c * A * n));
    ZG_TRY(dalloc_into(own, &p->inst_val, c * I * n));
    if (I) ZG_HIP(hipMemset(p->inst_val, 0, c * I * n * 32));  // rows past the instance stay zero (prove refills only what it must)
    p->inst_filled.assign(cap, 0);
    ZG_TRY(dalloc_into(own, &p->cin, c * 2 * NL * n));  // compressed inputs, then compressed tables
    p->ctab = p->cin + c * NL * n;
    ZG_TRY(dalloc_into(own, &p->perm, c * (2 * NL + 1) * n));  // + the vanishing argument's random polynomial
    ZG_TRY(dalloc_into(own, &p->zs, c * (S + NL + 1) * n));
    p->sz = p->snum = p->sden = p->stmp = nullptr;
    if (NS) {
        ZG_TRY(dalloc_into(own, &p->sz, c * NS * n));
        ZG_TRY(dalloc_into(own, &p->snum, c * NS * n));
        ZG_TRY(dalloc_into(own, &p->sden, c * NS * n));
        ZG_TRY(dalloc_into(own, &p->stmp, poly_grand_product_tmp_elems(n, cap * NS)));
    }
    const uint32_t mb = S + NL;
    ZG_TRY(dalloc_into(own, &p->num, c * mb * n));
    ZG_TRY(dalloc_into(own, &p->den, c * mb * n));
    ZG_TRY(dalloc_into(own, &p->tmp, poly_grand_product_tmp_elems(n, cap * mb)));
    ZG_TRY(dalloc_into(own, &p->raw, c * 2 * NL * n));
    ZG_TRY(dalloc_into(own, &p->sraw, c * NL * n));
    ZG_TRY(dalloc_into(own, &p->sort_fe, c * NL * n));
    ZG_TRY(dalloc_into(own, &p->sort_u32, c * 2 * NL * n + c * 3 * NL + 2));
    p->max_points = 4 + (uint32_t)(k.advice_queries.size() + k.fixed_queries.size());
    if (p->max_points > PC_MAX_POINTS) p->max_points = PC_MAX_POINTS;
    ZG_TRY(dalloc_into(own, &p->pw, c * p->max_points * n));
    p->max_evals = (uint32_t)(k.advice_queries.size() + k.fixed_queries.size()) + P + 3 * S + 5 * NL + 2 * NS + 4;
    ZG_TRY(dalloc_into(own, &p->wpoly, c * 2 * p->max_points * n));
    p->maxv = std::max<uint32_t>(std::max<uint32_t>(A, 2 * NL + 1), std::max<uint32_t>(S + NL + 1 + NS, std::max<uint32_t>(Q, p->max_points)));
    ZG_TRY(dalloc_into(own, &p->xyzz, c * p->maxv));
    ZG_TRY(dalloc_into(own, &p->d_idx, (size_t)4 * p->max_evals + 64 + (size_t)p->max_points * 512));
    // (per circuit: its advice queries, 3 per permutation set but 2 for the last, 5 per lookup; once: fixed, sigma, h, random)
    p->mlists_cap = c * (k.advice_queries.size() + (S ? 3 * S - 1 : 0) + 5 * NL + 2 * NS) + k.fixed_queries.size() + P + 2;
    ZG_TRY(dalloc_into(own, &p->d_mlists, p->mlists_cap));
    ZG_TRY(dalloc_into(own, &p->ktmp, poly_kate_tmp_elems(n, cap * p->max_points)));
    ZG_TRY(dalloc_into(own, &p->d_pc, c));
    p->d_chal = nullptr;
    if (k.NC) ZG_TRY(dalloc_into(own, &p->d_chal, c * k.NC * 2));
    p->hpc.assign(cap, ProofConst{});
    // SHPLONK's buffers, while the prover is set to it: per slot h1 and PC_MAX_POINTS + 1 rows of low
    // coefficients; the lists and coefficients for the opening queries of `cap` single proofs, or of one proof of `cap`
    // circuits -- the numerators' and L's behind each other
    size_t sh_stage = 0;
    if (p->multiopen == ZG_MULTIOPEN_SHPLONK) {
        p->sh_terms = p->mlists_cap + c * (k.fixed_queries.size() + P + 2);
        const size_t n_coef = p->sh_terms + c + 16, n_corr = c * (PC_MAX_POINTS + 1) * PC_MAX_POINTS;
        ZG_TRY(dalloc_into(own, &p->sh_lists, 2 * p->sh_terms + 16));
        ZG_TRY(dalloc_into(own, &p->sh_coef, n_coef));
        ZG_TRY(dalloc_into(own, &p->sh_corr, n_corr));
        ZG_TRY(dalloc_into(own, &p->sh_h1, c * n));
        // (both halves of a batch stage their two tables and the lists: room for them, so that no upload falls back to a
        //  pageable copy and its synchronise)
        sh_stage = 2 * (n_coef * sizeof(F9) + n_corr * sizeof(Fe) + 256) + (2 * p->sh_terms + 16) * 4;
    }
    // pinned (PinnedArena): commitments D2H (128 B each), evaluations D2H, error flags, then the H2D staging range
    PinnedArena& pin = p->pin;
    pin.evals_at = (c * p->maxv * sizeof(XYZZ) + 4095) & ~size_t(4095);
    pin.errors_at = pin.evals_at + c * p->max_evals * sizeof(Fe);
    pin.stage_begin = pin.evals_at + ((c * p->max_evals * sizeof(Fe) + c * NL * 4 + 4095) & ~size_t(4095));
    pin.cap = pin.stage_begin + (1u << 20) + c * 16 * sizeof(ProofConst) + c * (size_t)k.I * 4096 + sh_stage;
    // Kernels store results here that the host reads right after an event.  COHERENT (fine-grained), said explicitly:
    // with any flag but the default the runtime takes the coherence of host memory from HIP_HOST_COHERENT, and an event's
    // default release is device scope, which promises nothing about non-coherent host memory (the non-coherent form with a
    // hipEventReleaseToSystem event measured the same: 2.17 against 2.18 ms for a lone k = 14 proof).
    ZG_HIP(hipHostMalloc((void**)&pin.host, pin.cap, hipHostMallocMapped | hipHostMallocCoherent));
    ZG_HIP(hipHostGetDevicePointer((void**)&pin.dev, pin.host, 0));
    memset(pin.host + pin.stage_end(), 0, PinnedArena::MARGIN);  // (the margin behind the staging range: the gate words)
    return ZG_OK;
}

// ---- evaluate_h's view of one gate: gate = U(cell f) * inner, f a query index present in every monomial.
// U(x) = x when f occurs exactly once per monomial (uc empty); otherwise the monomials are grouped by the
// power of f and, when every group is a scalar multiple of the lowest one, U(x) = sum_k uc[k-1] x^k --
// the shape halo2's selector compression leaves behind (selector -> q * prod_{u != t} (u - q)).  Failing
// that, one occurrence of f is split off and the rest stays expanded.  Coefficients are in the 2^261 form.
// What the nine-limb evaluation does with a coefficient given in the 2^261 form (DMono::coeff_is_one): 1 / 2 for +1 / -1,
// 3 for any other integer c with |c| <= F9_SMALL_MAX, negative ones stored as r - |c| (DMono::small = c), 0 otherwise.
void classify_coeff9(DMono& d) {
    const Fe raw_one{{1, 0, 0, 0, 0, 0, 0, 0}};
    const Fe unhat = Fr::inv(Fr::from_u64(32));  // x * 2^261 -> the library form x * 2^256
    auto small_int = [&](const Fe& hat, int32_t* out) {  // the plain integer, if it is at most F9_SMALL_MAX
        const Fe v = Fr::mul(Fr::mul(hat, unhat), raw_one);
        for (int i = 1; i < 8; i++)
            if (v.l[i]) return false;
        *out = (int32_t)v.l[0];
        return v.l[0] <= (uint32_t)F9_SMALL_MAX;
    };
    int32_t c = 0;
    d.small = 0;
    if (small_int(d.coeff, &c)) {
        d.coeff_is_one = c == 1 ? 1 : 3;
        d.small = c;
    } else if (small_int(Fr::neg(d.coeff), &c)) {
        d.coeff_is_one = c == 1 ? 2 : 3;
        d.small = -c;
    } else {
        d.coeff_is_one = 0;
    }
}

struct GateFactor {
    std::vector<DMono> inner;
    std::vector<Fe> uc;
    uint32_t cost = 0;  // field products per row
};

GateFactor factor_gate(const std::vector<DMono>& monos, zg_poly g, uint32_t f, const Fe& c261, bool tabulated) {
    auto strip = [&](const DMono& src, bool all) {  // src without one / every occurrence of f
        DMono d = src;
        uint32_t w = 0;
        bool dropped = false;
        for (uint32_t b = 0; b < src.n_factors; b++) {
            if (src.factors[b] == f && (all || !dropped)) { dropped = true; continue; }
            d.factors[w++] = src.factors[b];
        }
        for (uint32_t b = w; b < ZG_MAX_FACTORS; b++) d.factors[b] = 0;
        d.n_factors = w;
        return d;
    };
    auto power = [&](const DMono& d) { return (uint32_t)std::count(d.factors, d.factors + d.n_factors, f); };
    auto same_cells = [](const DMono& x, const DMono& y) {
        return x.n_factors == y.n_factors && std::equal(x.factors, x.factors + x.n_factors, y.factors);
    };
    auto cell_order = [](const DMono& x, const DMono& y) {
        return std::lexicographical_compare(x.factors, x.factors + x.n_factors, y.factors, y.factors + y.n_factors);
    };
    uint32_t pmin = ZG_MAX_FACTORS + 1, pmax = 0;
    for (uint32_t m = g.first; m < g.first + g.count; m++) {
        pmin = std::min(pmin, power(monos[m]));
        pmax = std::max(pmax, power(monos[m]));
    }
    GateFactor out;
    bool univariate = pmax > 1;
    if (univariate) {
        std::vector<std::vector<DMono>> by_power(pmax + 1);
        for (uint32_t m = g.first; m < g.first + g.count; m++) by_power[power(monos[m])].push_back(strip(monos[m], true));
        for (auto& grp : by_power) std::sort(grp.begin(), grp.end(), cell_order);
        std::vector<DMono>& base = by_power[pmin];
        const Fe b0_inv = Fr::inv(base[0].coeff);
        out.uc.assign(pmax, Fe{});
        out.uc[pmin - 1] = Fr::mul(Fr::one(), c261);
        for (uint32_t k = pmin + 1; k <= pmax && univariate; k++) {
            const auto& grp = by_power[k];
            if (grp.empty()) continue;
            univariate = grp.size() == base.size();
            for (size_t i = 0; i < grp.size() && univariate; i++)  // grp = ratio * base, term by term
                univariate = same_cells(grp[i], base[i]) &&
                             fe_eq(Fr::mul(grp[i].coeff, base[0].coeff), Fr::mul(grp[0].coeff, base[i].coeff));
            if (univariate) out.uc[k - 1] = Fr::mul(Fr::mul(grp[0].coeff, b0_inv), c261);
        }
        if (univariate) {
            // U * B = (d U) * (B / d) with d the most frequent coefficient of B: those monomials become
            // coefficient-free products again, as they were before the selector was substituted
            // (up to sign: a coefficient -1 costs the kernel a subtraction, like +1 an addition)
            size_t best = 0, best_n = 0;
            for (size_t i = 0; i < base.size(); i++) {
                size_t cnt = 0;
                const Fe neg_i = Fr::neg(base[i].coeff);
                for (const DMono& o : base) cnt += fe_eq(o.coeff, base[i].coeff) || fe_eq(o.coeff, neg_i);
                if (cnt > best_n) best = i, best_n = cnt;
            }
            const Fe d = base[best].coeff, d_inv = Fr::inv(d);
            for (DMono& o : base) {
                o.coeff = Fr::mul(Fr::mul(o.coeff, d_inv), c261);  // (o / d) back in the 2^261 form
                classify_coeff9(o);
            }
            for (Fe& u : out.uc) u = Fr::mul(u, Fr::mul(d, Fr::inv(c261)));  // (d carries the 2^261 factor already)
            out.inner = std::move(base);
        }
    }
    if (!univariate) {
        out.uc.clear();
        for (uint32_t m = g.first; m < g.first + g.count; m++) out.inner.push_back(strip(monos[m], false));
    }
    for (const DMono& d : out.inner) {
        const uint32_t operands = d.n_factors + (d.coeff_is_one && d.n_factors ? 0u : 1u);  // (a small integer is no operand)
        out.cost += operands ? operands - 1 : 0;
    }
    if (!out.uc.empty() && !tabulated) out.cost += (uint32_t)out.uc.size();  // Horner in the kernel
    return out;
}

// ------------------------------------------------------------------ zg_prover_create, step by step
template <class T>
int key_alloc(PkDev* pk, T** out, size_t count) { return dalloc_into(pk->owned, out, count); }

int prover_events(zg_prover* p) {
    ZG_HIP(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    ZG_HIP(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
    ZG_HIP(hipEventCreateWithFlags(&p->ev_err, hipEventDisableTiming));
    for (hipEvent_t& e : p->evs) ZG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return ZG_OK;
}

// the key's shape: the circuit's sizes, the domain's constants, the forms evaluate_h's data is kept in
int key_shape(PkDev* pk, const zg_ctx* ctx, const zg_circuit* cs, const zg_fr* vk_repr) {
    pk->device = ctx->device;
    pk->k = cs->k;
    pk->n = 1u << cs->k;
    pk->cs_degree = cs->cs_degree;
    pk->bf = cs->blinding_factors;
    pk->qpd = cs->cs_degree - 1;
    pk->ext_k = cs->k;
    while ((1ull << pk->ext_k) < (uint64_t)pk->n * pk->qpd) pk->ext_k++;
    ZG_REQUIRE(pk->ext_k <= 22, ZG_ERR_UNSUPPORTED, "zg_prover_create: extended domain 2^%u not built", pk->ext_k);
    pk->en = 1u << pk->ext_k;
    ZG_REQUIRE(pk->n > pk->bf + 2, ZG_ERR_INVALID_ARG, "zg_prover_create: too few rows");
    pk->usable = pk->n - (pk->bf + 1);
    pk->F = cs->n_fixed; pk->A = cs->n_advice; pk->I = cs->n_instance; pk->P = cs->n_perm_columns; pk->NL = cs->n_lookups;
    pk->chunk = cs->cs_degree - 2;
    pk->sets = pk->P ? (pk->P + pk->chunk - 1) / pk->chunk : 0;
    pk->advice_queries.assign(cs->advice_queries, cs->advice_queries + cs->n_advice_queries);
    pk->fixed_queries.assign(cs->fixed_queries, cs->fixed_queries + cs->n_fixed_queries);
    pk->vk_repr = to_fe(vk_repr);
    pk->omega = host_domain_omega(pk->k);
    pk->omega_inv = Fr::inv(pk->omega);
    pk->ifft_div = Fr::inv(Fr::from_u64(pk->n));
    pk->hat = knob(K_EVALH9) != 0;
    pk->grouped = knob(K_EVALH_GROUPED) != 0;
    pk->delta_inv = Fr::inv(fr_delta());
    pk->zeta = ctx->coset_gen;
    return ZG_OK;
}

// Challenges become columns: every ZG_CHALLENGE query is rewritten to the instance-like column IU + its index (`queries`
// keeps the rewritten list alive, *out is the circuit with that list and I = IU + NC instance columns), and the key learns
// how many there are.  A circuit without challenges comes back as it is.
int challenge_columns(PkDev* pk, const zg_circuit* cs, std::vector<zg_query>& queries, zg_circuit* out) {
    *out = *cs;
    pk->IU = cs->n_instance;
    pk->NC = 0;
    pk->q_chal.assign(cs->n_queries, 0);
    for (uint32_t q = 0; q < cs->n_queries; q++) {
        if (cs->queries[q].kind != ZG_CHALLENGE) continue;
        ZG_REQUIRE(cs->queries[q].column < ZG_MAX_CHALLENGES, ZG_ERR_INVALID_ARG, "zg_prover_create: query %u names challenge %u (max %u)", q,
                   cs->queries[q].column, (uint32_t)ZG_MAX_CHALLENGES);
        pk->q_chal[q] = 1;
        pk->NC = std::max(pk->NC, cs->queries[q].column + 1);
    }
    for (uint32_t c = 0; c < cs->n_perm_columns; c++)
        ZG_REQUIRE(cs->perm_columns[c].kind != ZG_CHALLENGE, ZG_ERR_INVALID_ARG, "zg_prover_create: permutation column %u is a challenge", c);
    if (!pk->NC) return ZG_OK;
    queries.assign(cs->queries, cs->queries + cs->n_queries);
    for (uint32_t q = 0; q < cs->n_queries; q++)
        if (pk->q_chal[q]) queries[q].kind = ZG_INSTANCE, queries[q].column += pk->IU;
    out->queries = queries.data();
    out->n_instance = pk->I = pk->IU + pk->NC;
    return ZG_OK;
}

// the circuit image, validated; its monomials and lookups in the layout the kernels read
int validate_circuit(const PkDev* pk, const zg_circuit* cs, std::vector<DMono>& monos, std::vector<DLookup>& lks) {
    for (uint32_t q = 0; q < cs->n_queries; q++) {
        const zg_query& qq = cs->queries[q];
        uint32_t lim = qq.kind == ZG_FIXED ? pk->F : qq.kind == ZG_ADVICE ? pk->A : qq.kind == ZG_INSTANCE ? pk->I : 0;
        ZG_REQUIRE(qq.column < lim, ZG_ERR_INVALID_ARG, "zg_prover_create: query %u names column %u of kind %u", q,
                   qq.column, qq.kind);
        // (a ZG_CHALLENGE query arrives here as its pseudo-column, rewritten by challenge_columns: a rotation would leave
        //  the constant polynomial what it is, but upstream has none)
        ZG_REQUIRE(!(q < pk->q_chal.size() && pk->q_chal[q]) || qq.rotation == 0, ZG_ERR_INVALID_ARG,
                   "zg_prover_create: query %u rotates a challenge", q);
    }
    monos.assign(cs->n_monomials, DMono{});
    Fe one = Fr::one();
    for (uint32_t m = 0; m < cs->n_monomials; m++) {
        const zg_monomial& s = cs->monomials[m];
        ZG_REQUIRE(s.n_factors <= ZG_MAX_FACTORS, ZG_ERR_INVALID_ARG, "zg_prover_create: monomial %u has %u factors", m, s.n_factors);
        DMono d;
        memset(&d, 0, sizeof(d));
        memcpy(&d.coeff, &s.coeff, 32);
        d.n_factors = s.n_factors;
        d.coeff_is_one = fe_eq(d.coeff, one) ? 1 : fe_eq(d.coeff, Fr::neg(one)) ? 2 : 0;
        for (uint32_t f = 0; f < s.n_factors; f++) {
            ZG_REQUIRE(s.factors[f] < cs->n_queries, ZG_ERR_INVALID_ARG, "zg_prover_create: monomial %u factor out of range", m);
            d.factors[f] = s.factors[f];
        }
        monos[m] = d;
    }
    auto poly_ok = [&](const zg_poly& q) { return (uint64_t)q.first + q.count <= cs->n_monomials; };
    lks.assign(cs->n_lookups, DLookup{});
    for (uint32_t l = 0; l < cs->n_lookups; l++) {
        const zg_lookup& s = cs->lookups[l];
        ZG_REQUIRE(s.width >= 1 && s.width <= ZG_MAX_LOOKUP_WIDTH, ZG_ERR_INVALID_ARG, "zg_prover_create: lookup %u width %u", l, s.width);
        lks[l].width = s.width;
        for (uint32_t e = 0; e < s.width; e++) {
            ZG_REQUIRE(poly_ok(s.inputs[e]) && poly_ok(s.tables[e]), ZG_ERR_INVALID_ARG, "zg_prover_create: lookup %u polynomial out of range", l);
            lks[l].inputs[e] = s.inputs[e];
            lks[l].tables[e] = s.tables[e];
        }
    }
    for (uint32_t gi = 0; gi < cs->n_gates; gi++)
        ZG_REQUIRE(poly_ok(cs->gates[gi]), ZG_ERR_INVALID_ARG, "zg_prover_create: gate %u out of range", gi);
    for (uint32_t c = 0; c < cs->n_perm_columns; c++) {
        const zg_query& qq = cs->perm_columns[c];
        uint32_t lim = qq.kind == ZG_FIXED ? pk->F : qq.kind == ZG_ADVICE ? pk->A : qq.kind == ZG_INSTANCE ? pk->I : 0;
        ZG_REQUIRE(qq.column < lim, ZG_ERR_INVALID_ARG, "zg_prover_create: permutation column %u out of range", c);
    }
    ZG_REQUIRE(cs->n_lookups <= 60, ZG_ERR_UNSUPPORTED, "zg_prover_create: %u lookups", cs->n_lookups);
    return ZG_OK;
}

// the witness check's host view: which lookup tables are the key's alone, which depend on the witness
void check_info(PkDev* pk, const zg_circuit* cs, const std::vector<DMono>& monos, const std::vector<DLookup>& lks) {
    pk->NG = cs->n_gates;
    pk->ck.perm_cols.assign(cs->perm_columns, cs->perm_columns + cs->n_perm_columns);
    for (uint32_t l = 0; l < cs->n_lookups; l++) {
        bool var = false;
        for (uint32_t e = 0; e < lks[l].width; e++)
            for (uint32_t m = lks[l].tables[e].first; m < lks[l].tables[e].first + lks[l].tables[e].count; m++)
                for (uint32_t f = 0; f < monos[m].n_factors; f++) var |= cs->queries[monos[m].factors[f]].kind != ZG_FIXED;
        pk->ck.lookup_width.push_back(lks[l].width);
        pk->ck.table_var.push_back(var ? 1 : 0);
    }
}

// the circuit's tables to the device (DevCircuit)
int upload_circuit(PkDev* pk, const zg_circuit* cs, const std::vector<DMono>& monos, const std::vector<DLookup>& lks, hipStream_t st) {
    zg_query* d_q; DMono* d_m; zg_poly* d_g; DLookup* d_l; zg_query* d_pc;
    ZG_TRY(key_alloc(pk, &d_q, cs->n_queries));
    ZG_TRY(key_alloc(pk, &d_m, cs->n_monomials));
    ZG_TRY(key_alloc(pk, &d_g, cs->n_gates));
    ZG_TRY(key_alloc(pk, &d_l, cs->n_lookups));
    ZG_TRY(key_alloc(pk, &d_pc, cs->n_perm_columns));
    if (cs->n_queries) ZG_HIP(hipMemcpyAsync(d_q, cs->queries, cs->n_queries * sizeof(zg_query), hipMemcpyHostToDevice, st));
    if (cs->n_monomials) ZG_HIP(hipMemcpyAsync(d_m, monos.data(), monos.size() * sizeof(DMono), hipMemcpyHostToDevice, st));
    if (cs->n_gates) ZG_HIP(hipMemcpyAsync(d_g, cs->gates, cs->n_gates * sizeof(zg_poly), hipMemcpyHostToDevice, st));
    if (cs->n_lookups) ZG_HIP(hipMemcpyAsync(d_l, lks.data(), lks.size() * sizeof(DLookup), hipMemcpyHostToDevice, st));
    if (cs->n_perm_columns) ZG_HIP(hipMemcpyAsync(d_pc, cs->perm_columns, cs->n_perm_columns * sizeof(zg_query), hipMemcpyHostToDevice, st));
    ZG_HIP(hipStreamSynchronize(st));  // (the caller's host vectors may change from here on)
    pk->dc.queries = d_q; pk->dc.monos = d_m; pk->dc.gates = d_g; pk->dc.lookups = d_l; pk->dc.perm_cols = d_pc;
    pk->dc.n_gates = cs->n_gates; pk->dc.n_lookups = cs->n_lookups; pk->dc.n_perm = pk->P; pk->dc.chunk = pk->chunk;
    pk->dc.n_sets = pk->sets;
    return ZG_OK;
}

// Every query index present in all monomials of the gate is a candidate factor (q * (b^2 - b) has two); the cheapest
// evaluation wins (*f: its query index, 0xffffffff when the gate has none).  zero_g's gates are selector * (...), and a
// selector halo2 merged with others is a polynomial in its column: that one is tabulated with the proving key.
GateFactor cheapest_factor(const std::vector<DMono>& monos, const zg_circuit* cs, zg_poly g, const Fe& c261, uint32_t* f) {
    GateFactor best;
    *f = 0xffffffffu;
    const DMono& first = monos[g.first];
    for (uint32_t a = 0; a < first.n_factors; a++) {
        const uint32_t cand = first.factors[a];
        if (a && cand == first.factors[a - 1]) continue;
        bool all = true;
        for (uint32_t m = g.first; m < g.first + g.count && all; m++)
            all = std::find(monos[m].factors, monos[m].factors + monos[m].n_factors, cand) != monos[m].factors + monos[m].n_factors;
        if (!all) continue;
        GateFactor opt = factor_gate(monos, g, cand, c261, cs->queries[cand].kind == ZG_FIXED);
        if (*f == 0xffffffffu || opt.cost < best.cost) best = std::move(opt), *f = cand;
    }
    return best;
}

// evaluate_h's view of the circuit (hat): coefficients in the 2^261 form, gates factored by their common cell
int factored_view(PkDev* pk, const zg_circuit* cs, std::vector<DMono>& monos) {
    // Invariant (a fault in round 1, gdb: evaluate_h9_kernel reading monos_hat[m].n_factors through a null table):
    // hat implies that monos_hat, gates_hat, gate_common, gate_uni, uni_coef and gate_slab are ALL allocated here,
    // whatever the circuit holds (no gates, no lookups); poly_evaluate_h refuses a launch without them.
    const Fe c261 = Fr9Params::c261_fe();
    for (auto& d : monos) {
        d.coeff = Fr::mul(d.coeff, c261);
        classify_coeff9(d);
    }
    std::vector<zg_poly> gates_hat(cs->n_gates);
    std::vector<uint32_t> common(cs->n_gates, 0xffffffffu);
    std::vector<zg_poly> gate_uni(cs->n_gates, zg_poly{0, 0});  // count 0: the factor is the cell itself
    std::vector<Fe> uni_coef;
    for (uint32_t gi = 0; gi < cs->n_gates; gi++) {
        const zg_poly g = cs->gates[gi];
        gates_hat[gi] = g;
        if (g.count < 2) continue;
        uint32_t f;
        const GateFactor best = cheapest_factor(monos, cs, g, c261, &f);
        if (f == 0xffffffffu) continue;
        gates_hat[gi].first = (uint32_t)monos.size();
        gates_hat[gi].count = (uint32_t)best.inner.size();
        monos.insert(monos.end(), best.inner.begin(), best.inner.end());
        if (!best.uc.empty()) {
            gate_uni[gi].first = (uint32_t)uni_coef.size();
            gate_uni[gi].count = (uint32_t)best.uc.size();
            if (cs->queries[f].kind == ZG_FIXED) pk->slab_jobs.push_back({gi, f, gate_uni[gi].first, gate_uni[gi].count});
            uni_coef.insert(uni_coef.end(), best.uc.begin(), best.uc.end());
        }
        common[gi] = f;
    }
#ifdef ZG_TICKS
    {   // per row of evaluate_h: the coefficient products of the factored tables, as eval_poly9 will see them
        uint32_t full = 0, small = 0, cells = 0;
        auto tally = [&](zg_poly q) {
            for (uint32_t m = q.first; m < q.first + q.count; m++) {
                const DMono& d = monos[m];
                if (!d.n_factors) continue;
                full += d.coeff_is_one == 0;
                small += d.coeff_is_one == 3;
                cells += d.n_factors - 1;
            }
        };
        for (uint32_t gi = 0; gi < cs->n_gates; gi++) tally(gates_hat[gi]);
        for (uint32_t l = 0; l < cs->n_lookups; l++)
            for (uint32_t e = 0; e < cs->lookups[l].width; e++) tally(cs->lookups[l].inputs[e]), tally(cs->lookups[l].tables[e]);
        fprintf(stderr, "evaluate_h tables: per row %u products by a full coefficient, %u by a small integer, %u between cells\n",
                full, small, cells);
    }
#endif
    ZG_TRY(key_alloc(pk, &pk->gate_uni, cs->n_gates ? cs->n_gates : 1));
    ZG_TRY(key_alloc(pk, &pk->uni_coef, uni_coef.size() ? uni_coef.size() : 1));
    if (cs->n_gates) ZG_HIP(hipMemcpy(pk->gate_uni, gate_uni.data(), cs->n_gates * sizeof(zg_poly), hipMemcpyHostToDevice));
    if (!uni_coef.empty()) ZG_HIP(hipMemcpy(pk->uni_coef, uni_coef.data(), uni_coef.size() * sizeof(Fe), hipMemcpyHostToDevice));
    ZG_TRY(key_alloc(pk, &pk->monos_hat, monos.size() ? monos.size() : 1));
    ZG_TRY(key_alloc(pk, &pk->gates_hat, cs->n_gates ? cs->n_gates : 1));
    ZG_TRY(key_alloc(pk, &pk->gate_common, cs->n_gates ? cs->n_gates : 1));
    if (!monos.empty()) ZG_HIP(hipMemcpy(pk->monos_hat, monos.data(), monos.size() * sizeof(DMono), hipMemcpyHostToDevice));
    if (cs->n_gates) {
        ZG_HIP(hipMemcpy(pk->gates_hat, gates_hat.data(), cs->n_gates * sizeof(zg_poly), hipMemcpyHostToDevice));
        ZG_HIP(hipMemcpy(pk->gate_common, common.data(), cs->n_gates * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return ZG_OK;
}

// SRS: upload + window tables, or tables shared with other provers on this device (read-only)
int attach_bases(zg_prover* p, const zg_g1_affine* g, const zg_g1_affine* g_lagrange, const zg_bases* shared_g, const zg_bases* shared_gl) {
    zg_ctx* ctx = p->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t n = p->pk->n;
    if (shared_g) {
        ZG_REQUIRE(shared_g->device == ctx->device && shared_gl->device == ctx->device, ZG_ERR_INVALID_ARG,
                   "zg_prover_create_shared: bases live on another device");
        ZG_REQUIRE(shared_g->n == shared_gl->n && shared_g->n <= n && shared_g->n >= 1 && shared_g->c == shared_gl->c, ZG_ERR_INVALID_ARG,
                   "zg_prover_create_shared: bases do not match 2^k = %u points", n);
        p->g = const_cast<zg_bases*>(shared_g);
        p->gl = const_cast<zg_bases*>(shared_gl);
    } else {
        p->owned_bases = std::make_shared<zg_prover::OwnedBases>();
        WsScope ws(ctx);
        Affine* d = ws.get<Affine>(n);
        if (!d) return ZG_ERR_OOM;
        ZG_HIP(hipMemcpyAsync(d, g, (size_t)n * sizeof(Affine), hipMemcpyHostToDevice, st));
        ZG_TRY(bases_register_dev(ctx, d, n, 0, &p->owned_bases->g));
        ZG_HIP(hipMemcpyAsync(d, g_lagrange, (size_t)n * sizeof(Affine), hipMemcpyHostToDevice, st));
        ZG_TRY(bases_register_dev(ctx, d, n, 0, &p->owned_bases->gl));
        p->g = p->owned_bases->g;
        p->gl = p->owned_bases->gl;
    }
    // (fewer points than 2^k: a point-range shard of the SRS; zg_prover_set_shard names the range before the first proof)
    p->shard_lo = 0;
    p->shard_n = (uint32_t)p->g->n;
    return ZG_OK;
}

// ... and the tables the commitments are multiplied against (ZG_MSM_RUNS, ZG_MSM_NAF_GL, ZG_MSM_NAF)
int enable_tables(zg_prover* p) {
    zg_ctx* ctx = p->ctx;
    const PkDev* pk = p->pk.get();
    const bool run_form = knob(K_MSM_RUNS) != 0;
    if (run_form && pk->sets + pk->NL > 0) ZG_TRY(bases_enable_runs(ctx, p->gl));
    p->naf_gl_w = naf_gl_default(p->gl);
    // The quotient pieces and the opening quotients are vectors of random scalars, which fill every window.  With
    // 288 GB of HBM the base set gets a table with one row per BIT position (bases_enable_naf; 255 rows: 0.27 GB at
    // k = 14, 2.1 GB at k = 17) and a scalar is recoded into odd signed digits at FREE positions: 254 / (w + 1)
    // additions per scalar and only odd buckets -- 15.9 at w = 15 where 12-bit windows spend 22.  Same-box A/B at
    // k = 14: 0.7447 -> 0.7319 ms/proof against a larger-window table (w = 15; 14: 0.7355, 13: 0.744, 16: 0.753);
    // k = 17, w = 16: 5.97 -> 5.895.  ZG_MSM_NAF = digit width, 0 = the window table only.
    const int naf_env = knob(K_MSM_NAF);
    uint32_t lg = 0;
    while ((2u << lg) <= p->g->n) lg++;
    uint32_t nw = lg >= 16 ? 16u : lg >= 14 ? 15u : lg + 1 < 3 ? 3u : lg + 1;
    if (naf_env >= 0) nw = (uint32_t)naf_env;
    if (nw >= 3 && nw <= 16) {
        ZG_TRY(bases_enable_naf(ctx, p->g, nw));
        const zg_bases* gd = bases_dense(p->g);
        if (p->naf_gl_w && p->gl->run_table && gd && gd->naf_w) {
            // the same for g_lagrange and its running sums: the sorted columns and the products are committed in the
            // run form, whose coefficients s_i - s_{i+1} are full-size scalars wherever a row changes something
            ZG_TRY(bases_enable_naf(ctx, p->gl, gd->naf_w));
            if (zg_bases* gld = bases_dense(p->gl)) ZG_TRY(bases_enable_runs(ctx, gld));
        }
    }
    return ZG_OK;
}

// parts of the extended domain
void choose_domain_parts(PkDev* pk) {
    const uint32_t n = pk->n, en = pk->en, Q = pk->qpd;
    const bool split_env = knob(K_SPLIT_DOMAIN) != 0;
    uint32_t m1 = 1;
    while (m1 * 2 <= Q) m1 *= 2;
    const uint32_t m2 = Q - m1;
    const bool split = split_env && pk->hat && m2 != 0 && (m2 & (m2 - 1)) == 0 && (m1 + m2) * n < en;
    auto log2u = [](uint32_t v) { uint32_t l = 0; while ((1u << l) < v) l++; return l; };
    // The single coset serves the latency configuration (a lone proof pays for the extra launches of the split
    // form in its h phase: 0.72 -> 0.93 ms), the split one the throughput configuration (-5 % ms/proof); both sets
    // of proving-key cosets are kept (+60 % of 0.2 GB per key) and zg_prover_set_overlap picks.
    pk->nparts = 1;
    pk->dom[0].ek = pk->ext_k; pk->dom[0].en = en; pk->dom[0].zpow = 1;
    if (split) {
        pk->nparts = 3;
        pk->dom[1].ek = pk->k + log2u(m1); pk->dom[1].en = n * m1; pk->dom[1].zpow = 1;
        pk->dom[2].ek = pk->k + log2u(m2); pk->dom[2].en = n * m2; pk->dom[2].zpow = 2;
    }
}

// The quotient's terms by degree (PkDev::QTerms), degrees as ConstraintSystem::degree counts them: a gate's polynomial
// degree, selector included; c + 2 for the product term of a permutation set of c columns; max(4, 2 + input degree + table
// degree) for a lookup's product term; 2 or 3 for every other term (l0 / l_last / chaining terms of the permutation and
// the lookups' other four), which are therefore always low: m1 >= 2 wherever the domain is split.  A witness polynomial is
// needed on the second part when a high term queries it at any rotation.
int classify_terms(PkDev* pk, const zg_circuit* cs) {
    PkDev::QTerms& qt = pk->qt;
    const uint32_t NG = cs->n_gates, S = pk->sets, NL = pk->NL, A = pk->A, I = pk->I;
    uint32_t m1 = 1;
    while (m1 * 2 <= pk->qpd) m1 *= 2;  // (choose_domain_parts' first part)
    const uint32_t low_max = m1 + 1;
    auto degree = [&](const zg_poly& q) {
        uint32_t d = 0;
        for (uint32_t m = q.first; m < q.first + q.count; m++) {
            uint32_t f = 0;  // (a challenge has degree 0, as ConstraintSystem::degree counts it)
            for (uint32_t i = 0; i < cs->monomials[m].n_factors; i++) f += pk->q_chal[cs->monomials[m].factors[i]] ? 0u : 1u;
            d = std::max(d, f);
        }
        return d;
    };
    qt.gate_hi.assign(NG, 0);
    qt.set_hi.assign(S, 0);
    qt.lk_hi.assign(NL, 0);
    qt.part2.assign((size_t)A + I + S + 3 * NL + pk->NS, 0);
    auto mark_cell = [&](const zg_query& q) {
        if (q.kind == ZG_ADVICE) qt.part2[q.column] = 1;
        else if (q.kind == ZG_INSTANCE) qt.part2[A + q.column] = 1;
    };
    auto mark = [&](const zg_poly& q) {
        for (uint32_t m = q.first; m < q.first + q.count; m++)
            for (uint32_t f = 0; f < cs->monomials[m].n_factors; f++) mark_cell(cs->queries[cs->monomials[m].factors[f]]);
    };
    bool any_low = S + NL > 0;
    std::vector<uint32_t> cls(NG ? NG : 1, 0);
    uint32_t last[2] = {0xffffffffu, 0xffffffffu};
    for (uint32_t g = 0; g < NG; g++) {
        const uint32_t hi = degree(cs->gates[g]) > low_max ? 1u : 0u;
        qt.gate_hi[g] = (uint8_t)hi;
        any_low |= !hi;
        if (hi) mark(cs->gates[g]);
        cls[g] = hi | (last[hi] == 0xffffffffu ? 1u : g - last[hi]) << 1;
        last[hi] = g;
    }
    const uint32_t T = evalh_terms(*pk);
    qt.tail_lo = last[0] == 0xffffffffu ? 0u : T + NG - 1 - last[0];
    qt.tail_hi = last[1] == 0xffffffffu ? 0u : T + NG - 1 - last[1];
    qt.set_mask = 0;
    qt.lk_mask = 0;
    for (uint32_t s = 0; s < S; s++) {
        const uint32_t c0 = s * pk->chunk, c1 = std::min(pk->P, c0 + pk->chunk);
        if (c1 - c0 + 2 <= low_max) continue;
        qt.set_hi[s] = 1;
        if (s < 32) qt.set_mask |= 1u << s;
        qt.part2[A + I + s] = 1;
        for (uint32_t col = c0; col < c1; col++) mark_cell(cs->perm_columns[col]);
    }
    for (uint32_t l = 0; l < NL; l++) {
        const zg_lookup& lk = cs->lookups[l];
        uint32_t din = 1, dtab = 1;  // (at least 1, as upstream counts them)
        for (uint32_t e = 0; e < lk.width; e++) {
            din = std::max(din, degree(lk.inputs[e]));
            dtab = std::max(dtab, degree(lk.tables[e]));
        }
        if (std::max(4u, 2 + din + dtab) <= low_max) continue;
        qt.lk_hi[l] = 1;
        qt.lk_mask |= 1ull << l;
        qt.part2[A + I + S + l] = 1;
        qt.part2[A + I + S + NL + 2 * l] = qt.part2[A + I + S + NL + 2 * l + 1] = 1;
        for (uint32_t e = 0; e < lk.width; e++) mark(lk.inputs[e]), mark(lk.tables[e]);
    }
    // (the shuffles' terms are computed on every part: their products and every cell they read are needed on the second)
    for (uint32_t j = 0; j < pk->NS; j++) {
        qt.part2[A + I + S + 3 * NL + j] = 1;
        for (uint32_t e = 0; e < pk->shuffles[j].width; e++) mark(pk->shuffles[j].inputs[e]), mark(pk->shuffles[j].tables[e]);
    }
    // (without low terms, without the split domain or its grouped nine-limb kernel, or with more terms than eh_ypow has
    //  powers for, every term stays on both parts)
    qt.active = pk->nparts == 3 && any_low && m1 >= 2 && T != 0 && T + NG < EH_MAX_YPOW && S <= 32 && NL < 64;
    ZG_TRY(key_alloc(pk, &qt.gate_cls, cls.size()));
    ZG_HIP(hipMemcpy(qt.gate_cls, cls.data(), cls.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return ZG_OK;
}

int alloc_key_slabs(PkDev* pk) {
    const uint32_t n = pk->n, F = pk->F, P = pk->P;
    ZG_TRY(key_alloc(pk, &pk->sh_polys, (size_t)(F + P) * n));
    ZG_TRY(key_alloc(pk, &pk->fixed_val, (size_t)F * n));
    ZG_TRY(key_alloc(pk, &pk->sigma_val, (size_t)P * n));
    for (uint32_t di = 0; di < pk->nparts; di++) {
        PkDev::Dom& d = pk->dom[di];
        ZG_TRY(key_alloc(pk, &d.fixed_cos, (size_t)F * d.en));
        ZG_TRY(key_alloc(pk, &d.sigma_cos, (size_t)P * d.en));
        if (evalh_perm_scaled(*pk)) ZG_TRY(key_alloc(pk, &d.sigma_sc, (size_t)P * d.en));
        ZG_TRY(key_alloc(pk, &d.l0, (size_t)d.en));
        ZG_TRY(key_alloc(pk, &d.llast, (size_t)d.en));
        ZG_TRY(key_alloc(pk, &d.lactive, (size_t)d.en));
    }
    return ZG_OK;
}

// keygen_pk's derived data of `count` key columns (fixed / sigma): values -> HBM, coefficient forms, cosets on every part
int key_columns(zg_ctx* ctx, PkDev* pk, const zg_fr* values, uint32_t count, Fe* val, Fe* polys, Fe* PkDev::Dom::*cos) {
    const uint32_t n = pk->n;
    if (!count) return ZG_OK;
    ZG_HIP(hipMemcpyAsync(val, values, (size_t)count * n * 32, hipMemcpyHostToDevice, ctx->stream));
    ZG_TRY(ntt_batch_to_dev(ctx, val, polys, n, count, pk->k, pk->omega_inv, &pk->ifft_div));
    for (uint32_t di = 0; di < pk->nparts; di++) {
        PkDev::Dom& d = pk->dom[di];
        ZG_TRY(coeff_to_coset_dev(ctx, polys, n, n, d.*cos, d.en, count, d.ek, pk->hat, pk->shift(d.zpow)));
    }
    return ZG_OK;
}

// evaluate_h's scaled permutation term: sigma_sc[col] = sigma_cos[col] * (delta^col zeta^zpow)^-1 on every part
int key_sigma_scaled(zg_ctx* ctx, PkDev* pk) {
    if (!evalh_perm_scaled(*pk)) return ZG_OK;
    for (uint32_t di = 0; di < pk->nparts; di++) {
        PkDev::Dom& d = pk->dom[di];
        Fe f = pk->shift(3 - d.zpow);  // zeta^-zpow (zeta^3 = 1)
        for (uint32_t col = 0; col < pk->P; col++) {
            ZG_TRY(poly_scale(ctx, d.sigma_cos + (size_t)col * d.en, d.sigma_sc + (size_t)col * d.en, d.en, f));
            f = Fr::mul(f, pk->delta_inv);
        }
    }
    return ZG_OK;
}

// a gate factor that is a polynomial in a FIXED cell (a merged selector) does not depend on the
// witness: its coset is part of the proving key here, as the unmerged selector's would have been
int key_gate_slabs(zg_ctx* ctx, PkDev* pk, const zg_circuit* cs) {
    const uint32_t n = pk->n;
    hipStream_t st = ctx->stream;
    std::vector<uint32_t> slab_of(cs->n_gates ? cs->n_gates : 1, 0xffffffffu);
    ZG_TRY(key_alloc(pk, &pk->gate_slab, slab_of.size()));
    for (uint32_t di = 0; di < pk->nparts; di++) {
        PkDev::Dom& d = pk->dom[di];
        ZG_TRY(key_alloc(pk, &d.gate_slabs, std::max<size_t>(1, pk->slab_jobs.size() * (size_t)d.en)));
        for (size_t j = 0; j < pk->slab_jobs.size(); j++) {
            const auto& job = pk->slab_jobs[j];
            const zg_query q = cs->queries[job.query];
            ZG_TRY(poly_gate_factor(ctx, d.fixed_cos + (size_t)q.column * d.en, (uint32_t)(q.rotation * (int32_t)(d.en / n)),
                                    d.en, pk->uni_coef + job.first, job.count, d.gate_slabs + j * (size_t)d.en));
            slab_of[job.gate] = (uint32_t)j;
        }
    }
    ZG_HIP(hipMemcpyAsync(pk->gate_slab, slab_of.data(), slab_of.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ZG_HIP(hipStreamSynchronize(st));
    return ZG_OK;
}

// l_0 / l_last / l_active_row on every part of the domain
int key_l_polynomials(zg_ctx* ctx, PkDev* pk) {
    const uint32_t n = pk->n, en = pk->en;
    WsScope ws(ctx);
    Fe* t3 = ws.get<Fe>((size_t)3 * n);
    Fe* lblind = ws.get<Fe>(en);
    if (ws.failed) return ZG_ERR_OOM;
    ZG_TRY(poly_l_cosets_init(ctx, t3, t3 + n, t3 + 2 * n, n, pk->bf));
    ZG_TRY(ntt_batch_dev(ctx, t3, n, 3, pk->k, pk->omega_inv, &pk->ifft_div));
    for (uint32_t di = 0; di < pk->nparts; di++) {
        PkDev::Dom& d = pk->dom[di];
        ZG_TRY(coeff_to_coset_dev(ctx, t3, n, n, d.l0, d.en, 1, d.ek, pk->hat, pk->shift(d.zpow)));
        ZG_TRY(coeff_to_coset_dev(ctx, t3 + n, n, n, d.llast, d.en, 1, d.ek, pk->hat, pk->shift(d.zpow)));
        ZG_TRY(coeff_to_coset_dev(ctx, t3 + 2 * n, n, n, lblind, d.en, 1, d.ek, pk->hat, pk->shift(d.zpow)));
        ZG_TRY(poly_lactive(ctx, d.lactive, d.llast, lblind, d.en, pk->hat));
    }
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    return ZG_OK;
}

// t_evaluations of EvaluationDomain: ((shift * ext_omega^i)^n - 1)^-1, one period, per part of the domain; the twiddles
int key_t_evals(zg_ctx* ctx, PkDev* pk) {
    const uint32_t n = pk->n;
    ZG_TRY(get_twiddles(ctx, pk->k, pk->omega, &pk->omega_tw));
    for (uint32_t di = 0; di < pk->nparts; di++) {
        PkDev::Dom& d = pk->dom[di];
        uint32_t t_len = 1u << (d.ek - pk->k);
        std::vector<Fe> te(t_len);
        Fe ext_omega = host_domain_omega(d.ek);
        const Fe shift = pk->shift(d.zpow);
        Fe cur = Fr::pow_u64(shift, n), step = Fr::pow_u64(ext_omega, n);
        for (uint32_t i = 0; i < t_len; i++) {
            te[i] = Fr::inv(Fr::sub(cur, Fr::one()));
            if (pk->hat) te[i] = Fr::mul(te[i], Fr9Params::c261_fe());
            cur = Fr::mul(cur, step);
        }
        ZG_TRY(key_alloc(pk, &d.t_eval, t_len));
        ZG_HIP(hipMemcpy(d.t_eval, te.data(), t_len * sizeof(Fe), hipMemcpyHostToDevice));
        ZG_TRY(get_twiddles(ctx, d.ek, ext_omega, &d.ext_tw));
    }
    return ZG_OK;
}

}  // namespace

namespace zg {

int prover_drain(zg_prover* p) {
    ZG_ENTER(p->ctx);
    ZG_HIP(hipStreamSynchronize(p->ctx->stream));
    if (p->ctx->side) ZG_HIP(hipStreamSynchronize(p->ctx->side->stream));
    return ZG_OK;
}

int batch_args_ok(const char* who, const char* what, const zg_prover* p, size_t count, const zg_fr* const* instance, size_t instance_len) {
    const PkDev& pk = *p->pk;
    ZG_REQUIRE(count >= 1 && count <= p->cap, ZG_ERR_INVALID_ARG, "%s: %zu %s for %u slots (zg_prover_set_batch)", who, count, what, p->cap);
    ZG_REQUIRE(pk.IU == 0 || instance || instance_len == 0, ZG_ERR_INVALID_ARG, "%s: instance is null", who);
    ZG_REQUIRE(instance_len <= pk.usable, ZG_ERR_INVALID_ARG, "%s: instance too large (Error::InstanceTooLarge)", who);
    return ZG_OK;
}

int advice_into_slots(zg_prover* p, uint32_t nb, const zg_fr* const* advice_host, void* const* advice_dev) {
    const size_t adv_bs = (size_t)p->pk->A * p->pk->n;
    hipStream_t st = p->ctx->stream;
    for (uint32_t b = 0; b < nb && adv_bs; b++) {
        Fe* slot = p->adv_val + b * adv_bs;
        if (advice_host && advice_host[b]) {
            ZG_HIP(hipMemcpyAsync(slot, advice_host[b], adv_bs * 32, hipMemcpyHostToDevice, st));
        } else if (advice_dev && advice_dev[b] && advice_dev[b] != (void*)slot) {
            ZG_HIP(hipMemcpyAsync(slot, advice_dev[b], adv_bs * 32, hipMemcpyDeviceToDevice, st));
        }
    }
    return ZG_OK;
}

}  // namespace zg

extern "C" {

int zg_prover_set_multiopen(zg_prover* p, int scheme) {
    ZG_REQUIRE(p, ZG_ERR_INVALID_ARG, "zg_prover_set_multiopen: null prover");
    ZG_REQUIRE(scheme == ZG_MULTIOPEN_GWC || scheme == ZG_MULTIOPEN_SHPLONK, ZG_ERR_INVALID_ARG, "zg_prover_set_multiopen: scheme %d", scheme);
    ZG_ENTER(p->ctx);
    if (scheme == p->multiopen) return ZG_OK;
    ZG_TRY(prover_drain(p));
    const int before = p->multiopen;
    p->multiopen = scheme;
    p->warm_sig = 0;
    // SHPLONK's buffers and its share of the staging range come with the slots: allocate them anew (a prover that goes
    // back to GWC keeps what it has).  A failure leaves the prover without slots, as a failed zg_prover_set_batch does.
    if (scheme == ZG_MULTIOPEN_SHPLONK && p->cap && !p->sh_h1) {
        p->have_last = false;
        const int st = alloc_slots(p, p->cap);
        if (st != ZG_OK) p->multiopen = before;
        return st;
    }
    return ZG_OK;
}

int zg_prover_multiopen(const zg_prover* p) { return p ? p->multiopen : ZG_MULTIOPEN_GWC; }

int zg_prover_set_transcript(zg_prover* p, int transcript) {
    ZG_REQUIRE(p, ZG_ERR_INVALID_ARG, "zg_prover_set_transcript: null prover");
    ZG_REQUIRE(transcript == ZG_TRANSCRIPT_EVM || transcript == ZG_TRANSCRIPT_BLAKE2B, ZG_ERR_INVALID_ARG,
               "zg_prover_set_transcript: transcript %d", transcript);
    ZG_ENTER(p->ctx);
    p->transcript = transcript;  // (host state only: read when a batch of proofs starts)
    return ZG_OK;
}

int zg_prover_transcript(const zg_prover* p) { return p ? p->transcript : ZG_TRANSCRIPT_EVM; }

int zg_prover_set_phases(zg_prover* p, const uint8_t* advice_phase, uint32_t n_challenges, const uint8_t* challenge_phase) {
    ZG_REQUIRE(p, ZG_ERR_INVALID_ARG, "zg_prover_set_phases: null prover");
    const PkDev& pk = *p->pk;
    const char* why = phases_error(pk.A, advice_phase, pk.NC, n_challenges, challenge_phase, ZG_MAX_PHASES, ZG_MAX_CHALLENGES);
    ZG_REQUIRE(!why, ZG_ERR_INVALID_ARG, "zg_prover_set_phases: %s", why);
    ZG_ENTER(p->ctx);
    ZG_TRY(prover_drain(p));
    p->advice_phase.assign(advice_phase, advice_phase + pk.A);
    p->challenge_phase.assign(challenge_phase, challenge_phase + n_challenges);
    p->n_phases = 1;
    for (uint8_t ph : p->advice_phase) p->n_phases = std::max<uint32_t>(p->n_phases, ph + 1u);
    p->plans.clear();  // (the layouts they hold state the phases)
    p->warm_sig = 0;
    return ZG_OK;
}

int zg_prover_phases(const zg_prover* p, uint8_t* advice_phase, uint32_t* n_challenges, uint8_t* challenge_phase) {
    if (!p) return 0;
    for (uint32_t c = 0; advice_phase && c < p->pk->A; c++) advice_phase[c] = c < p->advice_phase.size() ? p->advice_phase[c] : 0;
    if (n_challenges) *n_challenges = (uint32_t)p->challenge_phase.size();
    for (size_t j = 0; challenge_phase && j < p->challenge_phase.size(); j++) challenge_phase[j] = p->challenge_phase[j];
    return (int)p->n_phases;
}

size_t zg_prover_proof_size(const zg_prover* p) { return zg_prover_proof_size_multi(p, 1); }

void zg_prover_destroy(zg_prover* p) {
    if (!p) return;
    {
        std::lock_guard<std::recursive_mutex> lock(p->ctx->mu);
        (void)hipSetDevice(p->ctx->device);
        (void)prover_drain(p);
        free_slots(p);
        if (p->gathered) (void)hipFree(p->gathered);
        p->owned_bases.reset();  // (the tables go with the last prover that uses them)
        if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
        if (p->ev_join) (void)hipEventDestroy(p->ev_join);
        if (p->ev_err) (void)hipEventDestroy(p->ev_err);
        for (hipEvent_t e : p->evs)
            if (e) (void)hipEventDestroy(e);
        p->pk.reset();  // (the key's HBM goes with its last prover)
    }
    delete p;
}

}  // extern "C"
// (poly.h)
int zg::shuffles_ok(const char* who, const zg_circuit* cs, const zg_shuffle* shuffles, uint32_t n_shuffles) {
    ZG_REQUIRE(shuffles || n_shuffles == 0, ZG_ERR_INVALID_ARG, "%s: %u shuffles and a null array", who, n_shuffles);
    ZG_REQUIRE(n_shuffles <= ZG_MAX_SHUFFLES, ZG_ERR_UNSUPPORTED, "%s: %u shuffles (max %u)", who, n_shuffles, (uint32_t)ZG_MAX_SHUFFLES);
    ZG_REQUIRE(n_shuffles == 0 || ((cs->monomials || !cs->n_monomials) && (cs->queries || !cs->n_queries)), ZG_ERR_INVALID_ARG,
               "%s: null circuit arrays", who);
    auto poly_ok = [&](const zg_poly& q) { return (uint64_t)q.first + q.count <= cs->n_monomials; };
    // ConstraintSystem::degree's count of an expression: a challenge has degree 0, an expression at least 1
    auto degree = [&](const zg_poly& q) {
        uint32_t d = 1;
        for (uint32_t m = q.first; m < q.first + q.count; m++) {
            uint32_t f = 0;
            for (uint32_t i = 0; i < cs->monomials[m].n_factors && i < ZG_MAX_FACTORS; i++) {
                const uint32_t qi = cs->monomials[m].factors[i];
                f += qi < cs->n_queries && cs->queries[qi].kind == ZG_CHALLENGE ? 0u : 1u;
            }
            d = std::max(d, f);
        }
        return d;
    };
    for (uint32_t j = 0; j < n_shuffles; j++) {
        const zg_shuffle& sf = shuffles[j];
        ZG_REQUIRE(sf.width >= 1 && sf.width <= ZG_MAX_LOOKUP_WIDTH, ZG_ERR_INVALID_ARG, "%s: shuffle %u width %u", who, j, sf.width);
        for (uint32_t e = 0; e < sf.width; e++) {
            ZG_REQUIRE(poly_ok(sf.inputs[e]) && poly_ok(sf.shuffles[e]), ZG_ERR_INVALID_ARG, "%s: shuffle %u polynomial out of range", who, j);
            const uint32_t need = 2 + std::max(degree(sf.inputs[e]), degree(sf.shuffles[e]));
            ZG_REQUIRE(cs->cs_degree >= need, ZG_ERR_INVALID_ARG, "%s: shuffle %u needs cs_degree %u, the circuit says %u", who, j, need,
                       cs->cs_degree);
        }
    }
    return ZG_OK;
}
extern "C" {

static int prover_create_impl(zg_ctx* ctx, const zg_circuit* cs, const zg_shuffle* shuffles, uint32_t n_shuffles, const zg_fr* fixed_values,
                              const zg_fr* sigma_values, const zg_g1_affine* g, const zg_g1_affine* g_lagrange, const zg_bases* shared_g,
                              const zg_bases* shared_gl, const zg_fr* vk_repr, zg_prover** out) {
    ZG_REQUIRE(ctx && cs && vk_repr && out, ZG_ERR_INVALID_ARG, "zg_prover_create: null argument");
    ZG_TRY(shuffles_ok("zg_prover_create", cs, shuffles, n_shuffles));
    ZG_REQUIRE(cs->n_fixed == 0 || fixed_values, ZG_ERR_INVALID_ARG, "zg_prover_create: fixed_values is null");
    ZG_REQUIRE(cs->n_perm_columns == 0 || sigma_values, ZG_ERR_INVALID_ARG, "zg_prover_create: sigma_values is null");
    ZG_REQUIRE(cs->cs_degree >= 3 && cs->cs_degree <= 9, ZG_ERR_UNSUPPORTED, "zg_prover_create: cs_degree %u", cs->cs_degree);
    ZG_REQUIRE(cs->k >= 4, ZG_ERR_UNSUPPORTED, "zg_prover_create: k=%u < 4", cs->k);
    ZG_ENTER(ctx);
    std::unique_ptr<zg_prover, void (*)(zg_prover*)> guard(new zg_prover(), zg_prover_destroy);
    zg_prover* p = guard.get();
    p->ctx = ctx;
    p->pk = std::make_shared<PkDev>();
    PkDev* pk = p->pk.get();
    // (the steps above, in the order they run: every HIP call of a step is on ctx->stream or synchronous)
    ZG_TRY(key_shape(pk, ctx, cs, vk_repr));
    ZG_TRY(prover_events(p));
    if (p->use_side && !ctx->side) ZG_TRY(zg_ctx_create(ctx->device, &ctx->side));
    std::vector<DMono> monos;
    std::vector<DLookup> lks;
    std::vector<zg_query> rewritten;
    zg_circuit with_columns;
    ZG_TRY(challenge_columns(pk, cs, rewritten, &with_columns));
    cs = &with_columns;  // (from here on a challenge is a column)
    p->challenge_phase.assign(pk->NC, 0);  // (the default: every challenge behind phase 0's commitments)
    ZG_TRY(validate_circuit(pk, cs, monos, lks));
    check_info(pk, cs, monos, lks);
    ZG_TRY(upload_circuit(pk, cs, monos, lks, ctx->stream));
    pk->NS = n_shuffles;
    for (uint32_t j = 0; j < n_shuffles; j++) {
        DLookup d{};
        d.width = shuffles[j].width;
        for (uint32_t e = 0; e < d.width; e++) d.inputs[e] = shuffles[j].inputs[e], d.tables[e] = shuffles[j].shuffles[e];
        pk->shuffles.push_back(d);
    }
    if (n_shuffles) {
        DLookup* d_sf = nullptr;
        ZG_TRY(key_alloc(pk, &d_sf, n_shuffles));
        ZG_HIP(hipMemcpy(d_sf, pk->shuffles.data(), n_shuffles * sizeof(DLookup), hipMemcpyHostToDevice));
        pk->d_shuffles = d_sf;
    }
    if (pk->hat) ZG_TRY(factored_view(pk, cs, monos));
    ZG_TRY(attach_bases(p, g, g_lagrange, shared_g, shared_gl));
    ZG_TRY(enable_tables(p));
    choose_domain_parts(pk);
    ZG_TRY(classify_terms(pk, cs));
    ZG_TRY(alloc_key_slabs(pk));
    // keygen_pk's derived data: fixed / sigma polys + cosets, the gate slabs, l_0 / l_last / l_active_row, t_evaluations
    ZG_TRY(key_columns(ctx, pk, fixed_values, pk->F, pk->fixed_val, pk->sh_polys, &PkDev::Dom::fixed_cos));
    if (pk->hat) ZG_TRY(key_gate_slabs(ctx, pk, cs));
    ZG_TRY(key_columns(ctx, pk, sigma_values, pk->P, pk->sigma_val, pk->sh_polys + (size_t)pk->F * pk->n, &PkDev::Dom::sigma_cos));
    ZG_TRY(key_sigma_scaled(ctx, pk));
    ZG_TRY(key_l_polynomials(ctx, pk));
    ZG_TRY(key_t_evals(ctx, pk));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    p->lat_split = lone_split(p, p->use_side);  // (a prover starts in the latency form)
    ZG_TRY(alloc_slots(p, 1));
    *out = guard.release();
    return ZG_OK;
}

int zg_prover_create(zg_ctx* ctx, const zg_circuit* cs, const zg_fr* fixed_values, const zg_fr* sigma_values,
                     const zg_g1_affine* g, const zg_g1_affine* g_lagrange, const zg_fr* vk_repr, zg_prover** out) {
    return zg_prover_create_shuffles(ctx, cs, nullptr, 0, fixed_values, sigma_values, g, g_lagrange, vk_repr, out);
}

int zg_prover_create_shuffles(zg_ctx* ctx, const zg_circuit* cs, const zg_shuffle* shuffles, uint32_t n_shuffles, const zg_fr* fixed_values,
                              const zg_fr* sigma_values, const zg_g1_affine* g, const zg_g1_affine* g_lagrange, const zg_fr* vk_repr,
                              zg_prover** out) {
    ZG_REQUIRE(g && g_lagrange, ZG_ERR_INVALID_ARG, "zg_prover_create: null SRS");
    return prover_create_impl(ctx, cs, shuffles, n_shuffles, fixed_values, sigma_values, g, g_lagrange, nullptr, nullptr, vk_repr, out);
}

int zg_prover_create_shared(zg_ctx* ctx, const zg_circuit* cs, const zg_fr* fixed_values, const zg_fr* sigma_values,
                            const zg_bases* g, const zg_bases* g_lagrange, const zg_fr* vk_repr, zg_prover** out) {
    return zg_prover_create_shared_shuffles(ctx, cs, nullptr, 0, fixed_values, sigma_values, g, g_lagrange, vk_repr, out);
}

int zg_prover_create_shared_shuffles(zg_ctx* ctx, const zg_circuit* cs, const zg_shuffle* shuffles, uint32_t n_shuffles,
                                     const zg_fr* fixed_values, const zg_fr* sigma_values, const zg_bases* g, const zg_bases* g_lagrange,
                                     const zg_fr* vk_repr, zg_prover** out) {
    ZG_REQUIRE(g && g_lagrange, ZG_ERR_INVALID_ARG, "zg_prover_create_shared: null bases");
    return prover_create_impl(ctx, cs, shuffles, n_shuffles, fixed_values, sigma_values, nullptr, nullptr, g, g_lagrange, vk_repr, out);
}

uint32_t zg_prover_shuffles(const zg_prover* p) { return p ? p->pk->NS : 0; }

int zg_prover_set_batch(zg_prover* p, size_t max_batch) {
    ZG_REQUIRE(p, ZG_ERR_INVALID_ARG, "zg_prover_set_batch: null prover");
    ZG_ENTER(p->ctx);
    ZG_TRY(prover_drain(p));
    if (max_batch == p->cap) return ZG_OK;
    ZG_REQUIRE(max_batch >= 1 && max_batch <= 1024, ZG_ERR_INVALID_ARG, "zg_prover_set_batch: %zu proofs", max_batch);
    p->have_last = false;
    ZG_TRY(alloc_slots(p, (uint32_t)max_batch));
    if (p->rccl_comm && p->gathered_cap < p->cap) {  // the gather buffer follows the slot count
        if (p->gathered) (void)hipFree(p->gathered);
        p->gathered = nullptr;
        ZG_HIP(hipMalloc((void**)&p->gathered, (size_t)p->world * p->maxv * p->cap * sizeof(XYZZ)));
        p->gathered_cap = p->cap;
    }
    return ZG_OK;
}

size_t zg_prover_batch(const zg_prover* p) { return p ? p->cap : 0; }

void* zg_prover_advice_slot(zg_prover* p, size_t slot) {
    if (!p || slot >= p->cap) return nullptr;
    return p->adv_val + slot * (size_t)p->pk->A * p->pk->n;
}

int zg_prover_fork(const zg_prover* parent, zg_ctx* ctx, zg_prover** out) {
    ZG_REQUIRE(parent && ctx && out, ZG_ERR_INVALID_ARG, "zg_prover_fork: null argument");
    ZG_REQUIRE(ctx->device == parent->pk->device, ZG_ERR_INVALID_ARG, "zg_prover_fork: the context is on another device");
    ZG_ENTER(ctx);
    std::unique_ptr<zg_prover, void (*)(zg_prover*)> guard(new zg_prover(), zg_prover_destroy);
    zg_prover* p = guard.get();
    p->ctx = ctx;
    p->pk = parent->pk;
    p->g = parent->g;
    p->gl = parent->gl;
    p->owned_bases = parent->owned_bases;  // (joint ownership; null when the caller registered the tables)
    p->use_side = parent->use_side;
    p->lat_split = parent->lat_split;
    p->naf_gl_w = parent->naf_gl_w;
    p->qterms = parent->qterms;
    p->multiopen = parent->multiopen;
    p->transcript = parent->transcript;
    p->advice_phase = parent->advice_phase; p->challenge_phase = parent->challenge_phase; p->n_phases = parent->n_phases;
    p->shard_lo = parent->shard_lo; p->shard_n = parent->shard_n; p->world = parent->world; p->rank = parent->rank;
    p->exchange = parent->exchange; p->exchange_user = parent->exchange_user;
    // (a communicator serialises its collectives on ONE stream: a fork does not inherit it)
    ZG_TRY(prover_events(p));
    if (p->use_side && !ctx->side) ZG_TRY(zg_ctx_create(ctx->device, &ctx->side));
    ZG_TRY(alloc_slots(p, parent->cap ? parent->cap : 1));
    *out = guard.release();
    return ZG_OK;
}

int zg_prover_set_overlap(zg_prover* p, int enable) {
    ZG_REQUIRE(p, ZG_ERR_INVALID_ARG, "zg_prover_set_overlap: null prover");
    ZG_ENTER(p->ctx);
    if (enable && !p->ctx->side) {
        ZG_TRY(zg_ctx_create(p->ctx->device, &p->ctx->side));
        p->ctx->side->profiling = p->ctx->profiling;
        p->ctx->side->prof_filter = p->ctx->prof_filter;
    }
    p->use_side = enable != 0;
    p->ctx->msm_pair = enable != 0;  // latency configuration: two lanes per addition in the MSM reduction
    p->lat_split = lone_split(p, enable != 0);
    return ZG_OK;
}

// The latency form's digit tables (msm.hip: every multiple of every window -- no buckets) of this prover's base sets:
// g, g_lagrange and the running sums of g_lagrange.  EXPLICIT since round 4: tens of GB and seconds of build
// time are the caller's decision, never a side effect of the first proof.
int zg_prover_enable_digit_tables(zg_prover* p, uint64_t max_bytes, uint64_t* bytes_built) {
    ZG_REQUIRE(p, ZG_ERR_INVALID_ARG, "zg_prover_enable_digit_tables: null prover");
    zg_ctx* ctx = p->ctx;
    ZG_ENTER(ctx);
    if (bytes_built) *bytes_built = 0;
    ZG_REQUIRE(p->g->n == p->gl->n, ZG_ERR_INVALID_ARG, "zg_prover_enable_digit_tables: the base sets differ in length");
    uint32_t c = p->g->full_c ? p->g->full_c : p->gl->full_c;
    if (!c) {
        size_t free_b = 0, total_b = 0;
        ZG_HIP(hipMemGetInfo(&free_b, &total_b));
        // the library's own cap: a third of the card (90 GB of the MI355X's 288), and never more than what is free now
        // minus a reserve of 8 GiB per table build
        double budget = max_bytes ? (double)max_bytes : (double)total_b / 3.0;
        if (budget > 90e9 && !max_bytes) budget = 90e9;
        if (budget + 3.0 * 8.0 * 1073741824.0 > (double)free_b) budget = (double)free_b - 3.0 * 8.0 * 1073741824.0;
        c = budget > 0 ? default_full_bits(p->g->n, budget) : 0;
    }
    if (!c) return ZG_OK;  // (n too large, the knob says none, or no room inside the budget: the bucket form stays)
    ZG_TRY(bases_enable_full(ctx, p->g, c, false));
    ZG_TRY(bases_enable_full(ctx, p->gl, c, true));
    if (bytes_built) {
        const uint64_t one = (uint64_t)((255 + c - 1) / c) * (1ull << (c - 1)) * p->g->n * sizeof(Affine);
        *bytes_built = (p->g->full_table.load() ? one : 0) + (p->gl->full_table.load() ? one : 0) + (p->gl->full_run_table.load() ? one : 0);
    }
    return ZG_OK;
}

int zg_prover_phase_ms(const zg_prover* p, double* out, size_t cap) {
    ZG_REQUIRE(p && out, ZG_ERR_INVALID_ARG, "zg_prover_phase_ms: null argument");
    for (size_t i = 0; i < cap && i < 8; i++) out[i] = p->phase_ms[i];
    return ZG_OK;
}

int zg_prover_gate_stats(const zg_prover* p, uint64_t* out, size_t cap) {
    ZG_REQUIRE(p && out, ZG_ERR_INVALID_ARG, "zg_prover_gate_stats: null argument");
    for (size_t i = 0; i < cap && i < 4; i++) out[i] = p->gate_stats[i];
    return ZG_OK;
}

int zg_prover_set_quotient_terms(zg_prover* p, int enable) {
    ZG_REQUIRE(p, ZG_ERR_INVALID_ARG, "zg_prover_set_quotient_terms: null prover");
    ZG_ENTER(p->ctx);
    ZG_TRY(prover_drain(p));
    p->qterms = enable != 0;
    p->warm_sig = 0;  // (another launch sequence: the next proof is a first proof)
    return ZG_OK;
}

int zg_prover_quotient_terms(const zg_prover* p, uint32_t* out, size_t cap, size_t* count) {
    ZG_REQUIRE(p && count, ZG_ERR_INVALID_ARG, "zg_prover_quotient_terms: null argument");
    const PkDev::QTerms& qt = p->pk->qt;
    std::vector<uint32_t> v = {qt.active ? 1u : 0u, (uint32_t)qt.gate_hi.size(), (uint32_t)qt.set_hi.size(), (uint32_t)qt.lk_hi.size(),
                               (uint32_t)qt.part2.size()};
    for (const std::vector<uint8_t>* part : {&qt.gate_hi, &qt.set_hi, &qt.lk_hi, &qt.part2}) v.insert(v.end(), part->begin(), part->end());
    *count = v.size();
    if (!out) return ZG_OK;
    ZG_REQUIRE(cap >= v.size(), ZG_ERR_INVALID_ARG, "zg_prover_quotient_terms: need %zu words", v.size());
    memcpy(out, v.data(), v.size() * sizeof(uint32_t));
    return ZG_OK;
}

int zg_prover_fetch_slot(zg_prover* p, size_t slot, uint32_t what, uint32_t index, zg_fr* out, size_t cap_elems) {
    ZG_REQUIRE(p && out, ZG_ERR_INVALID_ARG, "zg_prover_fetch: null argument");
    ZG_ENTER(p->ctx);
    ZG_REQUIRE(p->have_last, ZG_ERR_INVALID_ARG, "zg_prover_fetch: no proof has been produced yet");
    ZG_REQUIRE(slot < p->last_nb, ZG_ERR_INVALID_ARG, "zg_prover_fetch: slot %zu of a batch of %u", slot, p->last_nb);
    const PkDev& pk = *p->pk;
    const Fe* src = nullptr;
    size_t count = 0;
    const size_t n = pk.n;
    const Fe* zs = p->zs + slot * (size_t)(pk.sets + pk.NL + 1) * n;
    const Fe* perm = p->perm + slot * (size_t)(2 * pk.NL + 1) * n;
    const Fe* hp = p->pp + slot * (size_t)p->npp * n + (size_t)(p->ix_hpiece - p->nsh) * n;
    switch (what) {
        case 0: src = p->dbuf[0].h + slot * (size_t)pk.en; count = pk.en; break;
        case 1: ZG_REQUIRE(index < pk.sets, ZG_ERR_INVALID_ARG, "zg_prover_fetch: set %u", index);
                src = zs + (size_t)index * n; count = n; break;
        case 2: ZG_REQUIRE(index < pk.NL, ZG_ERR_INVALID_ARG, "zg_prover_fetch: lookup %u", index);
                src = zs + (size_t)(pk.sets + index) * n; count = n; break;
        case 3: ZG_REQUIRE(index < pk.NL, ZG_ERR_INVALID_ARG, "zg_prover_fetch: lookup %u", index);
                src = perm + (size_t)(2 * index) * n; count = n; break;
        case 4: ZG_REQUIRE(index < pk.NL, ZG_ERR_INVALID_ARG, "zg_prover_fetch: lookup %u", index);
                src = perm + (size_t)(2 * index + 1) * n; count = n; break;
        case 5: src = hp; count = (size_t)pk.qpd * n; break;
        case 6: case 7: case 8: case 9: case 10: {  // challenge `index` as a column: value row, coefficient row, slabs
            ZG_REQUIRE(index < pk.NC, ZG_ERR_INVALID_ARG, "zg_prover_fetch: challenge %u of %u", index, pk.NC);
            const uint32_t di = what - 8;
            ZG_REQUIRE(what < 8 || (di < pk.nparts && (di == 0) == !p->last_split), ZG_ERR_INVALID_ARG,
                       "zg_prover_fetch: the last proof did not use that part of the extended domain");
            if (what == 6) src = p->inst_val + (slot * pk.I + pk.IU + index) * n, count = n;
            else if (what == 7) src = p->pp + slot * (size_t)p->npp * n + (size_t)(p->ix_inst + pk.IU + index - p->nsh) * n, count = n;
            else src = p->dbuf[di].cos + (slot * p->ncos + pk.A + pk.IU + index) * (size_t)pk.dom[di].en, count = pk.dom[di].en;
            break;
        }
        case 11: ZG_REQUIRE(index < pk.NS, ZG_ERR_INVALID_ARG, "zg_prover_fetch: shuffle %u", index);
                 src = p->sz + (slot * pk.NS + index) * n; count = n; break;
        case 12: case 13: {  // h as the last proof left it on a part of the split domain
            const uint32_t di = what - 11;
            ZG_REQUIRE(p->last_split && di < pk.nparts, ZG_ERR_INVALID_ARG, "zg_prover_fetch: the last proof did not use the split domain");
            ZG_REQUIRE(!p->last_by_degree, ZG_ERR_INVALID_ARG,
                       "zg_prover_fetch: the last proof took the quotient's terms by degree, which reuses the parts' h (zg_prover_set_quotient_terms(0))");
            src = p->dbuf[di].h + slot * (size_t)pk.dom[di].en; count = pk.dom[di].en;
            break;
        }
        default: ZG_REQUIRE(false, ZG_ERR_INVALID_ARG, "zg_prover_fetch: unknown item %u", what);
    }
    ZG_REQUIRE(cap_elems >= count, ZG_ERR_INVALID_ARG, "zg_prover_fetch: need %zu elements", count);
    if (what == 0 && p->last_split) {  // split domain: h on EvaluationDomain's coset, from its coefficients
        WsScope ws(p->ctx);
        Fe* tmp = ws.get<Fe>(count);
        if (!tmp) return ZG_ERR_OOM;
        ZG_TRY(coeff_to_coset_dev(p->ctx, hp, (size_t)pk.qpd * n, (uint32_t)(pk.qpd * n), tmp, count, 1, pk.ext_k, false, pk.zeta));
        ZG_HIP(hipStreamSynchronize(p->ctx->stream));
        ZG_HIP(hipMemcpy(out, tmp, count * 32, hipMemcpyDeviceToHost));
        return ZG_OK;
    }
    if ((what == 0 || (what >= 8 && what != 11)) && pk.hat) {  // h and the slabs on a coset are kept as x * 2^261: hand back the library form
        WsScope ws(p->ctx);
        Fe* tmp = ws.get<Fe>(count);
        if (!tmp) return ZG_ERR_OOM;
        ZG_TRY(poly_scale(p->ctx, src, tmp, count, Fr::inv(Fr::from_u64(32))));
        ZG_HIP(hipStreamSynchronize(p->ctx->stream));
        ZG_HIP(hipMemcpy(out, tmp, count * 32, hipMemcpyDeviceToHost));
        return ZG_OK;
    }
    ZG_HIP(hipStreamSynchronize(p->ctx->stream));
    ZG_HIP(hipMemcpy(out, src, count * 32, hipMemcpyDeviceToHost));
    return ZG_OK;
}

int zg_prover_coset_generator(const zg_prover* p, zg_fr* out) {
    ZG_REQUIRE(p && out, ZG_ERR_INVALID_ARG, "zg_prover_coset_generator: null argument");
    memcpy(out, &p->pk->zeta, 32);
    return ZG_OK;
}

// What keygen_pk derived, as halo2's ProvingKey holds it: the coefficient forms as they stand, the extended families from
// the single-coset slabs (dom[0]: kept beside the split parts, and beside sigma_sc) with the nine-limb form's 2^5 taken off.
int zg_prover_export_key(zg_prover* p, uint32_t family, uint32_t index, zg_fr* out, size_t cap_elems) {
    ZG_REQUIRE(p && out, ZG_ERR_INVALID_ARG, "zg_prover_export_key: null argument");
    zg_ctx* ctx = p->ctx;
    ZG_ENTER(ctx);
    const PkDev& pk = *p->pk;
    const PkDev::Dom& d = pk.dom[0];
    const Fe* src = nullptr;
    uint32_t limit = 1;
    bool extended = true;
    switch (family) {
        case ZG_KEY_FIXED_POLY: src = pk.sh_polys; limit = pk.F; extended = false; break;
        case ZG_KEY_SIGMA_POLY: src = pk.sh_polys + (size_t)pk.F * pk.n; limit = pk.P; extended = false; break;
        case ZG_KEY_FIXED_COSET: src = d.fixed_cos; limit = pk.F; break;
        case ZG_KEY_SIGMA_COSET: src = d.sigma_cos; limit = pk.P; break;
        case ZG_KEY_L0: src = d.l0; break;
        case ZG_KEY_L_LAST: src = d.llast; break;
        case ZG_KEY_L_ACTIVE_ROW: src = d.lactive; break;
        default: ZG_REQUIRE(false, ZG_ERR_INVALID_ARG, "zg_prover_export_key: unknown family %u", family);
    }
    ZG_REQUIRE(index < limit, ZG_ERR_INVALID_ARG, "zg_prover_export_key: index %u of a family of %u", index, limit);
    const size_t count = extended ? d.en : pk.n;
    ZG_REQUIRE(cap_elems >= count, ZG_ERR_INVALID_ARG, "zg_prover_export_key: need %zu elements", count);
    src += (size_t)index * count;
    hipStream_t st = ctx->stream;
    if (extended && pk.hat) {
        WsScope ws(ctx);
        Fe* tmp = ws.get<Fe>(count);
        if (!tmp) return ZG_ERR_OOM;
        ZG_TRY(poly_scale(ctx, src, tmp, count, Fr::inv(Fr::from_u64(32))));
        ZG_HIP(hipMemcpyAsync(out, tmp, count * 32, hipMemcpyDeviceToHost, st));
        ZG_HIP(hipStreamSynchronize(st));
        return ZG_OK;
    }
    ZG_HIP(hipMemcpyAsync(out, src, count * 32, hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    return ZG_OK;
}

int zg_prover_fetch(zg_prover* p, uint32_t what, uint32_t index, zg_fr* out, size_t cap_elems) {
    return zg_prover_fetch_slot(p, 0, what, index, out, cap_elems);
}

// ---- stand-alone building blocks ----
// Evaluator::evaluate_h (+ vanishing::Argument::construct's division by X^n - 1) for ONE circuit instance over this
// prover's resident proving key: from the coefficient forms of the witness-side polynomials and the four challenges
// to h on EvaluationDomain's extended coset (2^ext_k values, library form).  Host pointers: this is the
// arithmetic-level entry; inside create_proof the same kernel runs on slabs that never leave HBM.
// (from_device: the families and h_out are device pointers -- zg_prover_evaluate_h_dev; the copies into slot 0 are then
//  device-to-device, h is scaled straight into h_out and the call returns with the work queued)
static int evaluate_h_impl(zg_prover* p, const void* advice_polys, const void* instance_polys, const void* perm_z_polys,
                           const void* lookup_z_polys, const void* permuted_polys, const zg_fr* theta, const zg_fr* beta,
                           const zg_fr* gamma, const zg_fr* y, void* h_out, bool from_device) {
    ZG_REQUIRE(p && theta && beta && gamma && y && h_out, ZG_ERR_INVALID_ARG, "zg_prover_evaluate_h: null argument");
    const PkDev& pk = *p->pk;
    ZG_REQUIRE((advice_polys || !pk.A) && (instance_polys || !pk.I) && (perm_z_polys || !pk.sets) &&
                   (lookup_z_polys || !pk.NL) && (permuted_polys || !pk.NL),
               ZG_ERR_INVALID_ARG, "zg_prover_evaluate_h: a polynomial family is missing");
    ZG_REQUIRE(pk.NS == 0, ZG_ERR_UNSUPPORTED, "zg_prover_evaluate_h: not for a circuit with shuffles (their products are no argument of this entry)");
    ZG_REQUIRE(p->cap >= 1, ZG_ERR_INVALID_ARG, "zg_prover_evaluate_h: the prover has no slot");
    zg_ctx* ctx = p->ctx;
    ZG_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const uint32_t n = pk.n;
    p->have_last = false;
    // slot 0's coefficient slab, in its order: advice, instance, permutation z, lookup z, a'/s'
    struct Fam { const void* src; uint32_t ix, count; };
    const hipMemcpyKind kind = from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const Fam fams[] = {{advice_polys, p->ix_adv, pk.A}, {instance_polys, p->ix_inst, pk.I}, {perm_z_polys, p->ix_pz, pk.sets},
                        {lookup_z_polys, p->ix_lz, pk.NL}, {permuted_polys, p->ix_perm, 2 * pk.NL}};
    for (const Fam& f : fams)
        if (f.count)
            ZG_HIP(hipMemcpyAsync(p->pp + (size_t)(f.ix - p->nsh) * n, f.src, (size_t)f.count * n * 32, kind, st));
    ProofConst& c = p->hpc[0];
    memset(&c, 0, sizeof(c));
    c.theta = to_fe(theta); c.beta = to_fe(beta); c.gamma = to_fe(gamma);
    evalh_consts(c, to_fe(y), pk);
    p->pin.stage_reset();
    ZG_TRY(upload_consts(p, 1));
    // (the scalars leave through the pinned staging range, which the next call on this prover rewinds: the device form
    //  returns with work queued, so it waits here until they -- and the copies above -- have arrived)
    if (from_device) ZG_HIP(hipStreamSynchronize(st));
    const PkDev::Dom& d = pk.dom[0];
    ZG_TRY(coeff_to_coset_dev(ctx, p->pp + (size_t)(p->ix_adv - p->nsh) * n, n, n, p->dbuf[0].cos, d.en, p->ncos, d.ek, pk.hat, pk.shift(d.zpow)));
    const EvalHArgs a = evalh_args(p, 0);
    ZG_TRY(poly_evaluate_h(ctx, a, d.en, 1, pk.A + pk.I + pk.F, (double)d.en));
    // (the nine-limb kernel leaves h as x * 2^261: hand back the library form)
    const Fe unhat = pk.hat ? Fr::inv(Fr::from_u64(32)) : Fr::one();
    if (from_device) return poly_scale(ctx, p->dbuf[0].h, (Fe*)h_out, d.en, unhat);
    WsScope ws(ctx);
    Fe* tmp = ws.get<Fe>(d.en);
    if (!tmp) return ZG_ERR_OOM;
    ZG_TRY(poly_scale(ctx, p->dbuf[0].h, tmp, d.en, unhat));
    ZG_HIP(hipMemcpyAsync(h_out, tmp, (size_t)d.en * 32, hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    return ZG_OK;
}

int zg_prover_evaluate_h(zg_prover* p, const zg_fr* advice_polys, const zg_fr* instance_polys, const zg_fr* perm_z_polys,
                         const zg_fr* lookup_z_polys, const zg_fr* permuted_polys, const zg_fr* theta, const zg_fr* beta,
                         const zg_fr* gamma, const zg_fr* y, zg_fr* h_out) {
    return evaluate_h_impl(p, advice_polys, instance_polys, perm_z_polys, lookup_z_polys, permuted_polys, theta, beta, gamma, y,
                           h_out, false);
}

int zg_prover_evaluate_h_dev(zg_prover* p, const void* d_advice_polys, const void* d_instance_polys, const void* d_perm_z_polys,
                             const void* d_lookup_z_polys, const void* d_permuted_polys, const zg_fr* theta, const zg_fr* beta,
                             const zg_fr* gamma, const zg_fr* y, void* d_h_out) {
    return evaluate_h_impl(p, d_advice_polys, d_instance_polys, d_perm_z_polys, d_lookup_z_polys, d_permuted_polys, theta, beta,
                           gamma, y, d_h_out, true);
}

// ---- the arithmetic level on device pointers: the prover's launch helpers over the CALLER's Lagrange columns and the
// resident key (fixed columns, sigma values, the circuit image)
static Cols caller_cols(const PkDev& pk, const void* d_advice, const void* d_instance) {
    Cols c;
    c.fixed = pk.fixed_val; c.advice = (const Fe*)d_advice; c.instance = (const Fe*)d_instance;
    c.log_size = pk.k; c.rot_scale = 1;
    c.adv_bs = 0; c.inst_bs = 0;
    return c;
}

int zg_prover_lookup_compress_dev(zg_prover* p, uint32_t lookup, const void* d_advice, const void* d_instance, const zg_fr* theta,
                                  void* d_input, void* d_table) {
    ZG_REQUIRE(p && theta && d_input && d_table, ZG_ERR_INVALID_ARG, "zg_prover_lookup_compress_dev: null argument");
    const PkDev& pk = *p->pk;
    ZG_REQUIRE(lookup < pk.NL, ZG_ERR_INVALID_ARG, "zg_prover_lookup_compress_dev: lookup %u of %u", lookup, pk.NL);
    ZG_REQUIRE((d_advice || !pk.A) && (d_instance || !pk.I), ZG_ERR_INVALID_ARG, "zg_prover_lookup_compress_dev: a column family is missing");
    zg_ctx* ctx = p->ctx;
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    ProofConst hc;
    memset(&hc, 0, sizeof(hc));
    hc.theta = to_fe(theta);
    ProofConst* dpc = nullptr;
    ZG_TRY(poly_one_const(ctx, ws, hc, &dpc));
    DevCircuit one = pk.dc;  // a circuit of ONE lookup: the kernel's lookup 0, written at column 0 of the outputs
    one.lookups = pk.dc.lookups + lookup;
    one.n_lookups = 1;
    return poly_lookup_compress(ctx, one, caller_cols(pk, d_advice, d_instance), dpc, 1, (Fe*)d_input, (Fe*)d_table, pk.n);
}

uint32_t zg_prover_permutation_sets(const zg_prover* p) { return p ? p->pk->sets : 0; }

int zg_prover_permutation_terms_dev(zg_prover* p, uint32_t set, const void* d_advice, const void* d_instance, const zg_fr* beta,
                                    const zg_fr* gamma, void* d_num, void* d_den) {
    ZG_REQUIRE(p && beta && gamma && d_num && d_den, ZG_ERR_INVALID_ARG, "zg_prover_permutation_terms_dev: null argument");
    const PkDev& pk = *p->pk;
    ZG_REQUIRE(set < pk.sets, ZG_ERR_INVALID_ARG, "zg_prover_permutation_terms_dev: set %u of %u", set, pk.sets);
    ZG_REQUIRE((d_advice || !pk.A) && (d_instance || !pk.I), ZG_ERR_INVALID_ARG, "zg_prover_permutation_terms_dev: a column family is missing");
    zg_ctx* ctx = p->ctx;
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    ProofConst hc;
    memset(&hc, 0, sizeof(hc));
    hc.beta = to_fe(beta);
    hc.gamma = to_fe(gamma);
    ProofConst* dpc = nullptr;
    ZG_TRY(poly_one_const(ctx, ws, hc, &dpc));
    return poly_perm_terms(ctx, pk.dc, caller_cols(pk, d_advice, d_instance), dpc, 1, pk.sigma_val, pk.omega_tw, (Fe*)d_num,
                           (Fe*)d_den, 1, pk.n, (int)set);
}

// keygen_vk's commit_lagrange of every fixed column and permutation polynomial, with the MSM the prover commits with
int zg_prover_vk_commitments(const zg_prover* p, zg_g1_affine* fixed_out, zg_g1_affine* sigma_out) {
    ZG_REQUIRE(p && (fixed_out || p->pk->F == 0) && (sigma_out || p->pk->P == 0), ZG_ERR_INVALID_ARG,
               "zg_prover_vk_commitments: null argument");
    ZG_REQUIRE(p->world == 1 && p->gl->n >= p->pk->n, ZG_ERR_UNSUPPORTED,
               "zg_prover_vk_commitments: a point-range shard holds only part of g_lagrange");
    zg_ctx* ctx = p->ctx;
    ZG_ENTER(ctx);
    const PkDev& pk = *p->pk;
    const uint32_t cnt[2] = {pk.F, pk.P};
    const Fe* vals[2] = {pk.fixed_val, pk.sigma_val};
    zg_g1_affine* outs[2] = {fixed_out, sigma_out};
    const uint32_t most = std::max(pk.F, pk.P);
    if (most == 0) return ZG_OK;
    void* d_xyzz = nullptr;
    ZG_HIP(hipMalloc(&d_xyzz, (size_t)most * sizeof(XYZZ)));
    std::vector<zg_g1> jac(most);
    int st = ZG_OK;
    for (int w = 0; w < 2 && st == ZG_OK; w++) {
        if (!cnt[w]) continue;
        st = zg_msm_batch_dev(ctx, p->gl, vals[w], pk.n, cnt[w], pk.n, d_xyzz);
        if (st == ZG_OK) st = zg_msm_finish(ctx, d_xyzz, cnt[w], jac.data());
        for (uint32_t c = 0; c < cnt[w] && st == ZG_OK; c++) {  // normalised: z = 1, or (0, 1, 0) for the identity
            const bool inf = fe_is_zero(*reinterpret_cast<const Fe*>(&jac[c].z));
            outs[w][c].x = inf ? zg_fq{} : jac[c].x;
            outs[w][c].y = inf ? zg_fq{} : jac[c].y;
        }
    }
    (void)hipFree(d_xyzz);
    return st;
}

}  // extern "C"
