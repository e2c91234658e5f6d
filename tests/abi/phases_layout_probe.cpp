// Host program for the advice phases of csrc/proof_layout.h (tests/test_phases_host.py): no device code, no HIP header.
// usage: phases_layout_probe <script>.  Every line of the script is one case,
//     A F P NL sets qpd bf log_n N  nAQ (column rotation)*nAQ  nFQ (column rotation)*nFQ  nAP (phase)*nAP  nCH (phase)*nCH
// (nAP = 0: the empty phase vector) and is answered by the lines below, "end" last.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../0g-halo2_amd/csrc/proof_layout.h"

using namespace zg;

static void print_scheme(const ProofShape& s, uint32_t N, bool shplonk) {
    const ProofLayout l = build_layout(s, N, shplonk);
    const char* name = shplonk ? "shplonk" : "gwc";
    std::printf("%s sizes points %u scalars %u evm %zu blake2b %zu\n", name, l.n_points(), l.n_scalars(), l.bytes(false), l.bytes(true));
    std::printf("%s families", name);
    for (uint32_t f = 0; f < N_POINT_FAMILIES; f++) std::printf(" %u:%u", l.pt[f].first, l.pt[f].count);
    for (uint32_t f = 0; f < N_EVAL_FAMILIES; f++) std::printf(" %u:%u", l.ev[f].first, l.ev[f].count);
    std::printf("\n%s phases", name);  // end/columns/challenges
    for (const ProofLayout::Phase& ph : l.phases) {
        std::printf(" %u/", ph.end);
        for (size_t i = 0; i < ph.columns.size(); i++) std::printf("%s%u", i ? "," : "", ph.columns[i]);
        std::printf("/");
        for (size_t i = 0; i < ph.challenges.size(); i++) std::printf("%s%u", i ? "," : "", ph.challenges[i]);
    }
    std::printf("\n%s advice", name);  // point_index of circuit:column, circuit-major
    for (uint32_t c = 0; c < N; c++)
        for (uint32_t i = 0; i < s.A; i++) std::printf(" %u:%u=%u", c, i, l.point_index(ADVICE, c, i));
    std::printf("\n%s others", name);  // the other families' point_index: untouched by the phases
    for (uint32_t c = 0; c < N; c++) {
        for (uint32_t i = 0; i < 2 * s.NL; i++) std::printf(" %u", l.point_index(PERMUTED, c, i));
        for (uint32_t i = 0; i < s.sets; i++) std::printf(" %u", l.point_index(PERM_Z, c, i));
        for (uint32_t i = 0; i < s.NL; i++) std::printf(" %u", l.point_index(LOOKUP_Z, c, i));
    }
    std::printf(" %u", l.point_index(RANDOM, 0, 0));
    std::printf("\n%s queries", name);
    for (const ProofLayout::Query& q : l.queries) std::printf(" %u:%u:%u@%u=%u/%u", (uint32_t)q.fam, q.circuit, q.index, q.point, q.eval, q.com);
    std::printf("\n%s adv_tables %zu %zu %zu\n", name, l.adv_first.size(), l.adv_per.size(), l.adv_place.size());
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
        ss >> s.A >> s.F >> s.P >> s.NL >> s.sets >> s.qpd >> s.bf >> s.log_n >> N;
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
        for (auto* list : {&s.advice_phase, &s.challenge_phase}) {
            size_t count = 0;
            ss >> count;
            for (size_t i = 0; i < count && ss; i++) {
                uint32_t phase = 0;
                ss >> phase;
                list->push_back((uint8_t)phase);
            }
        }
        if (!ss || N == 0 || N > 1024 || s.log_n == 0 || s.log_n > 28 || (!s.advice_phase.empty() && s.advice_phase.size() != s.A)) {
            std::fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        const char* why = s.advice_phase.empty() ? nullptr
                                                 : phases_error(s.A, s.advice_phase.data(), 0, (uint32_t)s.challenge_phase.size(),
                                                                s.challenge_phase.data(), 3, 16);
        std::printf("case N %u\n", N);
        std::printf("legal %s\n", why ? why : "yes");
        if (!why) {
            print_scheme(s, N, false);
            print_scheme(s, N, true);
        }
        std::printf("end\n");
    }
    return 0;
}
