// Host program for tests/test_transcript_host.py: csrc/blake2b.h, the Blake2bTranscript of csrc/transcript.h and the host
// path of csrc/g1_compress.h, driven by a script of one command per line; one line of output per command.  No device code
// runs.  Every integer is 32 bytes of little-endian hex, the canonical value.
//   hash <hex | ->            BLAKE2b-512, personalisation "Halo2-Transcript", of the bytes  -> 128 hex digits
//   raw <tokens>              the streaming state: `a<hex>` absorbs bytes, `q` prints the digest of a clone (clone-and-finalise)
//   wide <128 hex>            challenge_from_wide of a 64-byte digest                        -> the challenge
//   tr <tokens>               a Blake2bTranscript: `c<int>` common_scalar, `s<int>` write_scalar, `p<x>,<y>` write_point,
//                             `q` squeeze (prints the challenge); ends with `stream=<hex>` and `failed=<0|1>`
//   dec <64 hex>              g1_decompress_one -> valid x y
//   cmp <x> <y>               g1_compress_one of the point -> 64 hex digits
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../0g-halo2_amd/csrc/transcript.h"

using namespace zg;

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
    return out;
}
static std::string hex(const uint8_t* b, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) {
        s.push_back(d[b[i] >> 4]);
        s.push_back(d[b[i] & 15]);
    }
    return s;
}
static Fe raw_of(const std::string& h) {
    const std::vector<uint8_t> b = unhex(h);
    Fe v = fe_zero();
    for (size_t i = 0; i < b.size() && i < 32; i++) v.l[i >> 2] |= (uint32_t)b[i] << (8 * (i & 3));
    return v;
}
static std::string hex_of_raw(const Fe& raw) {
    uint8_t b[32];
    fe_to_le_bytes_raw(raw, b);
    return hex(b, 32);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: transcript_probe <script>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd, tok;
        ss >> cmd;
        if (cmd == "hash") {
            ss >> tok;
            const std::vector<uint8_t> data = unhex(tok);
            Blake2b s;
            b2_init_halo2(s);
            b2_update(s, data.data(), data.size());
            uint8_t d[64];
            b2_digest(s, d);
            std::cout << hex(d, 64) << "\n";
        } else if (cmd == "raw") {
            Blake2b s;
            b2_init_halo2(s);
            std::string out;
            while (ss >> tok) {
                if (tok[0] == 'a') {
                    const std::vector<uint8_t> data = unhex(tok.substr(1));
                    b2_update(s, data.data(), data.size());
                } else {
                    uint8_t d[64];
                    b2_digest(s, d);
                    out += hex(d, 64) + " ";
                }
            }
            std::cout << out << "\n";
        } else if (cmd == "wide") {
            ss >> tok;
            const std::vector<uint8_t> d = unhex(tok);
            std::cout << hex_of_raw(Fr::to_raw(challenge_from_wide(d.data()))) << "\n";
        } else if (cmd == "tr") {
            Blake2bTranscript t;
            std::string out;
            while (ss >> tok) {
                if (tok[0] == 'c') {
                    t.common_scalar(Fr::from_raw(raw_of(tok.substr(1))));
                } else if (tok[0] == 's') {
                    t.write_scalar(Fr::from_raw(raw_of(tok.substr(1))));
                } else if (tok[0] == 'p') {
                    const size_t comma = tok.find(',');
                    Jac p;
                    p.x = Fq::from_raw(raw_of(tok.substr(1, comma - 1)));
                    p.y = Fq::from_raw(raw_of(tok.substr(comma + 1)));
                    p.z = fe_is_zero(p.x) && fe_is_zero(p.y) ? fe_zero() : Fq::one();
                    t.write_point(p);
                } else {
                    out += hex_of_raw(Fr::to_raw(t.squeeze())) + " ";
                }
            }
            std::cout << out << "stream=" << (t.stream.empty() ? "-" : hex(t.stream.data(), t.stream.size())) << " failed=" << (t.failed ? 1 : 0)
                      << "\n";
        } else if (cmd == "dec") {
            ss >> tok;
            const std::vector<uint8_t> b = unhex(tok);
            Affine p;
            const bool ok = g1_decompress_one(b.data(), p);
            std::cout << (ok ? 1 : 0) << " " << hex_of_raw(Fq::to_raw(p.x)) << " " << hex_of_raw(Fq::to_raw(p.y)) << "\n";
        } else if (cmd == "cmp") {
            std::string xs, ys;
            ss >> xs >> ys;
            Affine p;
            p.x = Fq::from_raw(raw_of(xs));
            p.y = Fq::from_raw(raw_of(ys));
            uint8_t b[32];
            g1_compress_one(p, b);
            std::cout << hex(b, 32) << "\n";
        } else if (!cmd.empty()) {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
