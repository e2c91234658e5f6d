// The order of a proof's items, stated once: what create_proof writes and opens for N instances of one circuit under a
// multi-open argument (halo2_proofs v2023_04_20 src/plonk/prover.rs, src/poly/kzg/multiopen/{gwc,shplonk}), as the prover
// (prove_batch.hip), the batch verifier (verify.hip) and the proof-size functions all take it from here.  Host only, no
// HIP types: families and points are abstract, each side maps them to its own handles (polynomial indices and
// ProofConst slots; term indices and point sets).  The layout depends on the circuit, the scheme and N alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace zg {

struct ProofShape {
    uint32_t A = 0, F = 0, P = 0, NL = 0, sets = 0;  // advice, fixed, permutation columns; lookups; permutation z polynomials
    uint32_t NS = 0;                                 // shuffle arguments (one product polynomial each)
    uint32_t qpd = 0, bf = 0, log_n = 0;             // h pieces, blinding factors
    std::vector<std::pair<uint32_t, int32_t>> advice_queries, fixed_queries;  // (column, rotation)
    // create_proof's phases (ConstraintSystem::advice_column_phase / challenge_phase): the phase each advice column is
    // committed in (empty: all in the first) and the phase after whose commitments each challenge is squeezed
    std::vector<uint8_t> advice_phase, challenge_phase;
};

// A proof's commitments by family, in transcript order; behind them what an opening query may also name: the key's fixed
// and sigma commitments and h = sum_i xn^i (h piece i).  A circuit's share of ADVICE .. LOOKUP_Z follows the circuit
// before it; PERMUTED holds (input, table) per lookup: 2l, 2l + 1.
//
// The shuffle products (SHUFFLE_Z, one per shuffle and circuit) stand between LOOKUP_Z and RANDOM in the transcript; the
// enumerator follows H, and the family's range is kept beside pt[] (ProofLayout::shuffle_pt), so that every family
// before it keeps its number.  Without shuffles the range is empty and the layout is what it was.
enum Family : uint32_t { ADVICE, PERMUTED, PERM_Z, LOOKUP_Z, RANDOM, H_PIECE, OPENING, N_POINT_FAMILIES, FIXED = N_POINT_FAMILIES, SIGMA, H, SHUFFLE_Z };
// A proof's evaluations by family, in transcript order: every circuit's advice | fixed, random, sigma once | every
// circuit's permutation evaluations (set s: z, z(wx), z(w^last x) at 3s .., the last set without the third) | every
// circuit's lookup evaluations (z, z(wx), a', a'(w^-1 x), s') | every circuit's shuffle evaluations (z, z(wx):
// ProofLayout::shuffle_ev, beside ev[] as shuffle_pt is beside pt[]) | the expected h(x), which no proof holds.
//
// With advice phases the ADVICE family alone changes its order, for any N: phase-major, within a phase circuit-major,
// within a circuit ascending column -- create_proof commits every circuit's columns of a phase, then squeezes that
// phase's challenges (ascending index), then goes on to the next phase.  Evaluations and opening queries keep
// cs.advice_queries' order; point_index() is where a column's commitment stands.
enum EvalFamily : uint32_t { EV_ADVICE, EV_FIXED, EV_RANDOM, EV_SIGMA, EV_PERM, EV_LOOKUP, EV_H, N_EVAL_FAMILIES };

struct ProofLayout {
    struct Range { uint32_t first = 0, count = 0; };  // (count: of the whole proof, every circuit's share)
    static constexpr uint32_t NONE = ~0u;
    // (com, SHPLONK: the query's commitment in `coms`, NONE for a (commitment, point) pair that an earlier query opened)
    struct Query { Family fam; uint32_t circuit, index, point, eval, com = NONE; };
    // SHPLONK's construct_intermediate_sets: a commitment with the queries that open it, one per point of its set in the
    // set's order; a rotation set with its points (ascending) and commitments (first appearance)
    struct Com { Family fam; uint32_t circuit, index, set, place; std::vector<uint32_t> queries; };
    struct RotationSet { std::vector<uint32_t> points, coms; };

    // a phase of the advice commitments: where its points end among the proof's (every circuit's share), its columns in
    // ascending order and the challenges squeezed behind its last point, in squeeze order
    struct Phase { uint32_t end = 0; std::vector<uint32_t> columns, challenges; };

    uint32_t N = 1;
    bool shplonk = false;
    std::vector<Phase> phases;  // at least one; theta follows the last
    // more than one phase: per advice column where its phase starts among the ADVICE points, the columns of that phase
    // and the column's place among them (empty: the one phase holds the columns in their order)
    std::vector<uint32_t> adv_first, adv_per, adv_place;
    Range pt[N_POINT_FAMILIES], ev[N_EVAL_FAMILIES];
    Range shuffle_pt, shuffle_ev;           // SHUFFLE_Z's points (before pt[RANDOM]) and evaluations (before ev[EV_H])
    std::vector<Query> queries;             // create_proof's order
    std::vector<Query> evals;               // the same queries by evaluation index: transcript order, the expected h(x) last
    std::vector<int64_t> rotations;         // the distinct opening points x omega^r by first appearance (r as first met)
    std::vector<std::vector<uint32_t>> at;  // GWC: per point its queries in order -- one point set, one W, per point
    std::vector<Com> coms;                  // SHPLONK: by first appearance, a repeated (commitment, point) pair counted once
    std::vector<RotationSet> rsets;         // SHPLONK: by equal point sets, in the order of their first commitment
    // (SHPLONK's T, the distinct points over all sets, is every point: 0 .. rotations.size())

    uint32_t n_points() const { return pt[OPENING].first + pt[OPENING].count; }
    uint32_t n_scalars() const { return ev[EV_H].first; }
    size_t bytes(bool blake2b) const { return (size_t)(blake2b ? 32 : 64) * n_points() + (size_t)32 * n_scalars(); }
    // where commitment (fam, circuit, index) stands among the proof's points
    uint32_t point_index(Family fam, uint32_t circuit, uint32_t index) const {
        if (fam == ADVICE && !adv_first.empty()) return pt[ADVICE].first + adv_first[index] + circuit * adv_per[index] + adv_place[index];
        if (fam == SHUFFLE_Z) return shuffle_pt.first + circuit * (shuffle_pt.count / N) + index;
        return pt[fam].first + circuit * (pt[fam].count / N) + index;
    }
    // Blake2b transcript, a fixed layout of 32-byte items: the evaluations stand between the h pieces and the argument's points
    uint32_t item_of_point(uint32_t point) const { return point + (point >= pt[OPENING].first ? n_scalars() : 0); }
    size_t n_shplonk_pairs() const {
        size_t m = 0;
        for (const RotationSet& s : rsets) m += s.points.size();
        return m;
    }
};

namespace layout_detail {
inline void families(const ProofShape& s, uint32_t N, uint32_t n_open, ProofLayout& l) {
    ProofLayout::Range *pt = l.pt, *ev = l.ev;
    const uint32_t npz = s.sets ? 3 * s.sets - 1 : 0;
    const uint32_t pc[N_POINT_FAMILIES] = {N * s.A, N * 2 * s.NL, N * s.sets, N * s.NL, 1, s.qpd, n_open};
    const uint32_t ec[N_EVAL_FAMILIES] = {N * (uint32_t)s.advice_queries.size(), (uint32_t)s.fixed_queries.size(), 1, s.P, N * npz, N * 5 * s.NL, 1};
    // (the shuffle products: N * NS points in front of RANDOM, 2 N * NS evaluations in front of EV_H)
    for (uint32_t f = 0, at = 0; f < N_POINT_FAMILIES; at += pc[f++]) {
        if (f == RANDOM) l.shuffle_pt = {at, N * s.NS}, at += N * s.NS;
        pt[f] = {at, pc[f]};
    }
    for (uint32_t f = 0, at = 0; f < N_EVAL_FAMILIES; at += ec[f++]) {
        if (f == EV_H) l.shuffle_ev = {at, 2 * N * s.NS}, at += 2 * N * s.NS;
        ev[f] = {at, ec[f]};
    }
}
// the phases of the ADVICE family (ProofLayout::phases, adv_*)
inline void phases(const ProofShape& s, ProofLayout& l) {
    uint32_t last = 0;
    for (uint32_t c = 0; c < s.A && c < s.advice_phase.size(); c++) last = s.advice_phase[c] > last ? s.advice_phase[c] : last;
    l.phases.assign(last + 1, ProofLayout::Phase{});
    for (uint32_t c = 0; c < s.A; c++) l.phases[c < s.advice_phase.size() ? s.advice_phase[c] : 0].columns.push_back(c);
    for (uint32_t j = 0; j < s.challenge_phase.size(); j++) l.phases[s.challenge_phase[j] <= last ? s.challenge_phase[j] : last].challenges.push_back(j);
    uint32_t at = l.pt[ADVICE].first;
    for (ProofLayout::Phase& ph : l.phases) ph.end = at += l.N * (uint32_t)ph.columns.size();
    if (last == 0) return;
    l.adv_first.assign(s.A, 0); l.adv_per.assign(s.A, 0); l.adv_place.assign(s.A, 0);
    uint32_t first = 0;
    for (const ProofLayout::Phase& ph : l.phases) {
        for (uint32_t i = 0; i < ph.columns.size(); i++) {
            l.adv_first[ph.columns[i]] = first;
            l.adv_per[ph.columns[i]] = (uint32_t)ph.columns.size();
            l.adv_place[ph.columns[i]] = i;
        }
        first += l.N * (uint32_t)ph.columns.size();
    }
}
}  // namespace layout_detail

// What zg_prover_set_phases / zg_verifier_set_phases ask of a setting (upstream: advice_column_in and
// challenge_usable_after assert that the phase before has a column): nullptr when it is legal, else what is wrong.
// `used`: the challenges the circuit's expressions name.
inline const char* phases_error(uint32_t A, const uint8_t* advice_phase, uint32_t used, uint32_t n_challenges, const uint8_t* challenge_phase,
                                uint32_t max_phases, uint32_t max_challenges) {
    if ((A && !advice_phase) || (n_challenges && !challenge_phase)) return "a phase array is null";
    uint32_t last = 0, seen = 1;  // (phase 0 always exists)
    for (uint32_t c = 0; c < A; c++) {
        if (advice_phase[c] >= max_phases) return "an advice column's phase is out of range";
        last = advice_phase[c] > last ? advice_phase[c] : last;
        seen |= 1u << advice_phase[c];
    }
    if (seen != (2u << last) - 1u) return "a phase has no advice column (phases are contiguous from 0)";
    if (n_challenges < used) return "fewer challenges than the circuit uses";
    if (n_challenges > max_challenges) return "too many challenges";
    for (uint32_t j = 0; j < n_challenges; j++) {
        if (challenge_phase[j] >= max_phases) return "a challenge's phase is out of range";
        if (challenge_phase[j] > last) return "a challenge is squeezed after a phase that has no advice column";
    }
    return nullptr;
}

// The bound zg_prover_proof_size{,_multi} return: the proof's length with as many W as GWC could need, one per
// possible opening point (2 + every advice and fixed query), or SHPLONK's 2.
inline size_t proof_size_bound(const ProofShape& s, uint32_t N, bool shplonk, bool blake2b) {
    ProofLayout l;
    layout_detail::families(s, N, shplonk ? 2 : 2 + (uint32_t)(s.advice_queries.size() + s.fixed_queries.size()), l);
    return l.bytes(blake2b);
}

inline ProofLayout build_layout(const ProofShape& s, uint32_t N, bool shplonk) {
    ProofLayout l;
    l.N = N;
    l.shplonk = shplonk;
    layout_detail::families(s, N, 0, l);
    layout_detail::phases(s, l);
    // ---- the opening queries; points by first appearance, rotations compared mod n as upstream compares field points
    const int64_t n = (int64_t)1 << s.log_n, last = -(int64_t)(s.bf + 1);
    std::vector<int64_t> keys;
    auto add = [&](int64_t rot, Family fam, uint32_t circuit, uint32_t index, uint32_t eval) {
        const int64_t key = ((rot % n) + n) % n;
        uint32_t j = 0;
        while (j < keys.size() && keys[j] != key) j++;
        if (j == keys.size()) {
            keys.push_back(key);
            l.rotations.push_back(rot);
            l.at.emplace_back();
        }
        l.at[j].push_back((uint32_t)l.queries.size());
        l.queries.push_back({fam, circuit, index, j, eval});
    };
    const uint32_t AQ = (uint32_t)s.advice_queries.size(), npz = l.ev[EV_PERM].count / N;
    for (uint32_t c = 0; c < N; c++) {
        const uint32_t ev_adv = l.ev[EV_ADVICE].first + c * AQ, ev_pz = l.ev[EV_PERM].first + c * npz, ev_lk = l.ev[EV_LOOKUP].first + c * 5 * s.NL;
        for (uint32_t i = 0; i < AQ; i++) add(s.advice_queries[i].second, ADVICE, c, s.advice_queries[i].first, ev_adv + i);
        for (uint32_t z = 0; z < s.sets; z++) {
            add(0, PERM_Z, c, z, ev_pz + 3 * z);
            add(1, PERM_Z, c, z, ev_pz + 3 * z + 1);
        }
        for (uint32_t z = s.sets; z-- > 0;)
            if (z + 1 != s.sets) add(last, PERM_Z, c, z, ev_pz + 3 * z + 2);
        for (uint32_t k = 0; k < s.NL; k++) {
            add(0, LOOKUP_Z, c, k, ev_lk + 5 * k);
            add(0, PERMUTED, c, 2 * k, ev_lk + 5 * k + 2);
            add(0, PERMUTED, c, 2 * k + 1, ev_lk + 5 * k + 4);
            add(-1, PERMUTED, c, 2 * k, ev_lk + 5 * k + 3);
            add(1, LOOKUP_Z, c, k, ev_lk + 5 * k + 1);
        }
        for (uint32_t j = 0; j < s.NS; j++) {
            const uint32_t ev_sh = l.shuffle_ev.first + 2 * (c * s.NS + j);
            add(0, SHUFFLE_Z, c, j, ev_sh);
            add(1, SHUFFLE_Z, c, j, ev_sh + 1);
        }
    }
    for (uint32_t i = 0; i < s.fixed_queries.size(); i++) add(s.fixed_queries[i].second, FIXED, 0, s.fixed_queries[i].first, l.ev[EV_FIXED].first + i);
    for (uint32_t c = 0; c < s.P; c++) add(0, SIGMA, 0, c, l.ev[EV_SIGMA].first + c);
    add(0, H, 0, 0, l.ev[EV_H].first);
    add(0, RANDOM, 0, 0, l.ev[EV_RANDOM].first);
    l.evals.resize(l.queries.size());
    for (const ProofLayout::Query& q : l.queries) l.evals[q.eval] = q;
    l.pt[OPENING].count = shplonk ? 2 : (uint32_t)l.rotations.size();
    if (!shplonk) return l;
    // ---- construct_intermediate_sets over the same queries
    std::vector<std::vector<char>> opened;  // per commitment and point: is it opened there
    for (uint32_t qi = 0; qi < l.queries.size(); qi++) {
        const ProofLayout::Query q = l.queries[qi];
        size_t c = 0;
        while (c < l.coms.size() && !(l.coms[c].fam == q.fam && l.coms[c].circuit == q.circuit && l.coms[c].index == q.index)) c++;
        if (c == l.coms.size()) {
            l.coms.push_back({q.fam, q.circuit, q.index, 0, 0, {}});
            opened.emplace_back(l.rotations.size(), 0);
        }
        if (opened[c][q.point]) continue;
        opened[c][q.point] = 1;
        l.coms[c].queries.push_back(qi);
        l.queries[qi].com = (uint32_t)c;
    }
    std::vector<std::vector<char>> set_key;
    for (size_t c = 0; c < l.coms.size(); c++) {
        ProofLayout::Com& com = l.coms[c];
        size_t i = 0;
        while (i < set_key.size() && set_key[i] != opened[c]) i++;
        if (i == set_key.size()) {
            set_key.push_back(opened[c]);
            l.rsets.emplace_back();
            for (uint32_t p = 0; p < l.rotations.size(); p++)
                if (opened[c][p]) l.rsets[i].points.push_back(p);
        }
        com.set = (uint32_t)i;
        com.place = (uint32_t)l.rsets[i].coms.size();
        l.rsets[i].coms.push_back((uint32_t)c);
        std::vector<uint32_t> by_point;
        for (uint32_t p : l.rsets[i].points)
            for (uint32_t qi : com.queries)
                if (l.queries[qi].point == p) by_point.push_back(qi);
        com.queries.swap(by_point);
    }
    return l;
}

}  // namespace zg
