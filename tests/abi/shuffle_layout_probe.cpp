// Host program for the shuffle arguments of csrc/proof_layout.h (tests/test_shuffle_host.py): no device code, no HIP header.
// usage: shuffle_layout_probe <script>.  Every line of the script is one case,
//     A F P NL sets qpd bf log_n N NS  nAQ (column rotation)*nAQ  nFQ (column rotation)*nFQ
// and is answered by the lines below, "end" last.  A commitment or a query's polynomial is family:circuit:index, a shuffle
// product's family "sz".  With NS = 0 the answer is proof_layout_probe's for the same shape, line for line; with shuffles
// a line "<scheme> shuffles pt:first:count ev:first:count" follows the evals line: the family's points and evaluations.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../0g-halo2_amd/csrc/proof_layout.h"

using namespace zg;

static const char* const FAM[] = {"adv", "perm", "pz", "lz", "rand", "hp", "open", "fix", "sig", "h", "sz"};
static const char* const EVFAM[] = {"adv", "fix", "rand", "sig", "pz", "lk", "h"};

static void print_scheme(const ProofShape& s, uint32_t N, bool shplonk) {
    const ProofLayout l = build_layout(s, N, shplonk);
    const char* name = shplonk ? "shplonk" : "gwc";
    std::printf("%s sizes points %u scalars %u evm %zu blake2b %zu bound_evm %zu bound_blake2b %zu\n", name, l.n_points(), l.n_scalars(),
                l.bytes(false), l.bytes(true), proof_size_bound(s, N, shplonk, false), proof_size_bound(s, N, shplonk, true));
    std::printf("%s points", name);
    for (uint32_t f = 0; f < N_POINT_FAMILIES; f++) std::printf(" %s:%u:%u", FAM[f], l.pt[f].first, l.pt[f].count);
    std::printf("\n%s evals", name);
    for (uint32_t f = 0; f < N_EVAL_FAMILIES; f++) std::printf(" %s:%u:%u", EVFAM[f], l.ev[f].first, l.ev[f].count);
    if (s.NS) std::printf("\n%s shuffles pt:%u:%u ev:%u:%u", name, l.shuffle_pt.first, l.shuffle_pt.count, l.shuffle_ev.first, l.shuffle_ev.count);
    std::printf("\n%s items", name);  // the Blake2b verifier's: the item of every point
    for (uint32_t p = 0; p < l.n_points(); p++) std::printf(" %u", l.item_of_point(p));
    std::printf("\n%s rotations", name);
    for (int64_t r : l.rotations) std::printf(" %lld", (long long)r);
    std::printf("\n%s queries", name);  // polynomial@point=evaluation
    for (const ProofLayout::Query& q : l.queries) std::printf(" %s:%u:%u@%u=%u", FAM[q.fam], q.circuit, q.index, q.point, q.eval);
    std::printf("\n%s transcript", name);  // the evaluations in transcript order, as polynomial@point
    for (const ProofLayout::Query& q : l.evals) std::printf(" %s:%u:%u@%u", FAM[q.fam], q.circuit, q.index, q.point);
    std::printf("\n");
    if (!shplonk) {
        std::printf("gwc sets");  // per point the indices of its queries
        for (const std::vector<uint32_t>& set : l.at) {
            std::printf(" ");
            for (size_t k = 0; k < set.size(); k++) std::printf("%s%u", k ? "," : "", set[k]);
        }
        std::printf("\n");
        return;
    }
    std::printf("shplonk coms");  // commitment/set/place/queries, one per set point
    for (const ProofLayout::Com& c : l.coms) {
        std::printf(" %s:%u:%u/%u/%u/", FAM[c.fam], c.circuit, c.index, c.set, c.place);
        for (size_t k = 0; k < c.queries.size(); k++) std::printf("%s%u", k ? "," : "", c.queries[k]);
    }
    std::printf("\nshplonk sets");  // points/commitments
    for (const ProofLayout::RotationSet& rs : l.rsets) {
        std::printf(" ");
        for (size_t k = 0; k < rs.points.size(); k++) std::printf("%s%u", k ? "," : "", rs.points[k]);
        std::printf("/");
        for (size_t k = 0; k < rs.coms.size(); k++) std::printf("%s%u", k ? "," : "", rs.coms[k]);
    }
    std::printf("\nshplonk T %zu pairs %zu\n", l.rotations.size(), l.n_shplonk_pairs());
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <script>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        ProofShape s;
        uint32_t N = 0;
        ss >> s.A >> s.F >> s.P >> s.NL >> s.sets >> s.qpd >> s.bf >> s.log_n >> N >> s.NS;
        for (auto* list : {&s.advice_queries, &s.fixed_queries}) {
            size_t count = 0;
            ss >> count;
            for (size_t i = 0; i < count && ss; i++) {
                uint32_t column = 0;
                int32_t rotation = 0;
                ss >> column >> rotation;
                list->push_back({column, rotation});
            }
        }
        if (!ss || N == 0 || N > 1024 || s.NS > 1024 || s.log_n == 0 || s.log_n > 28) {
            std::fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        std::printf("case N %u\n", N);
        print_scheme(s, N, false);
        print_scheme(s, N, true);
        std::printf("end\n");
    }
    return 0;
}
