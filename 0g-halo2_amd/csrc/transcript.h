// Host side of the Fiat-Shamir transcript: Keccak-256 and snark-verifier's EvmTranscript
// (system/halo2/transcript/evm.rs at v2023_04_20; used by the reference at
// /root/reference/src/wnn.rs:21,241,249,260).  Points are absorbed / written as x || y, 32-byte
// big-endian canonical coordinates; scalars as 32-byte big-endian; a challenge is
// keccak256(buffer ++ [1 if the buffer is exactly the previous 32-byte state]) reduced mod r.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "blake2b.h"
#include "curve.h"
#include "g1_compress.h"
#include "keccak.h"

namespace zg {

inline void fe_to_be_bytes_fr(const Fe& a, uint8_t out[32]) {
    Fe r = Fr::to_raw(a);
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) out[31 - (4 * i + j)] = (uint8_t)(r.l[i] >> (8 * j));
}
inline void fe_to_be_bytes_fq(const Fe& a, uint8_t out[32]) {
    Fe r = Fq::to_raw(a);
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) out[31 - (4 * i + j)] = (uint8_t)(r.l[i] >> (8 * j));
}

class EvmTranscript {
   public:
    std::vector<uint8_t> buf;     // pending hash input
    std::vector<uint8_t> stream;  // proof bytes
    bool failed = false;          // an identity point was offered (EvmTranscript refuses those)

    void common_scalar(const Fe& s) {
        uint8_t b[32];
        fe_to_be_bytes_fr(s, b);
        buf.insert(buf.end(), b, b + 32);
    }
    void write_scalar(const Fe& s) {
        uint8_t b[32];
        fe_to_be_bytes_fr(s, b);
        buf.insert(buf.end(), b, b + 32);
        stream.insert(stream.end(), b, b + 32);
    }
    // p: normalised Jacobian as the MSM returns it (z = 1, or z = 0 for the identity)
    void write_point(const Jac& p) {
        if (fe_is_zero(p.z)) {
            failed = true;
            return;
        }
        uint8_t b[64];
        fe_to_be_bytes_fq(p.x, b);
        fe_to_be_bytes_fq(p.y, b + 32);
        buf.insert(buf.end(), b, b + 64);
        stream.insert(stream.end(), b, b + 64);
    }
    Fe squeeze() {
        if (squeeze_appends_one(buf.size())) buf.push_back(1);
        uint8_t h[32];
        keccak256(buf.data(), buf.size(), h);
        buf.assign(h, h + 32);
        return challenge_from_hash(h);
    }
};

// halo2's own transcript, writer side: Blake2bWrite<_, G1Affine, Challenge255> (halo2_proofs v2023_04_20
// src/transcript/blake2b.rs; blake2b.h).  A scalar is absorbed as 0x02 || to_repr() (32 little-endian bytes), a point as
// 0x01 || x.to_repr() || y.to_repr() -- the uncompressed pair -- while the PROOF gets the 32-byte GroupEncoding:
// x.to_repr() with the low bit of y in bit 7 of the last byte (halo2curves 0.3.3 G1Affine::to_bytes).
class Blake2bTranscript {
   public:
    Blake2b st;
    std::vector<uint8_t> stream;  // proof bytes
    bool failed = false;          // an identity point was offered (common_point refuses those)

    Blake2bTranscript() { b2_init_halo2(st); }
    void common_scalar(const Fe& s) {
        b2_byte(st, 2);
        b2_int(st, Fr::to_raw(s));
    }
    void write_scalar(const Fe& s) {
        const Fe raw = Fr::to_raw(s);
        uint8_t b[32];
        fe_to_le_bytes_raw(raw, b);
        b2_byte(st, 2);
        b2_update(st, b, 32);
        stream.insert(stream.end(), b, b + 32);
    }
    void write_point(const Jac& p) {
        if (fe_is_zero(p.z)) {
            failed = true;
            return;
        }
        const Fe x = Fq::to_raw(p.x), y = Fq::to_raw(p.y);
        b2_byte(st, 1);
        b2_int(st, x);
        b2_int(st, y);
        uint8_t b[32];
        fe_to_le_bytes_raw(x, b);
        b[31] |= (uint8_t)((y.l[0] & 1u) << 7);  // (g1_compress_one's bytes, from the integers at hand)
        stream.insert(stream.end(), b, b + 32);
    }
    Fe squeeze() { return b2_squeeze(st); }
};

// The transcript a proof is written into: one or the other (zg_prover_set_transcript), behind EvmTranscript's interface
class Transcript {
   public:
    bool blake2b = false;
    EvmTranscript evm;
    Blake2bTranscript b2;

    void common_scalar(const Fe& s) { blake2b ? b2.common_scalar(s) : evm.common_scalar(s); }
    void write_scalar(const Fe& s) { blake2b ? b2.write_scalar(s) : evm.write_scalar(s); }
    void write_point(const Jac& p) { blake2b ? b2.write_point(p) : evm.write_point(p); }
    Fe squeeze() { return blake2b ? b2.squeeze() : evm.squeeze(); }
    bool failed() const { return blake2b ? b2.failed : evm.failed; }
    const std::vector<uint8_t>& stream() const { return blake2b ? b2.stream : evm.stream; }
    const char* name() const { return blake2b ? "Blake2bWrite" : "EvmTranscript"; }
};

}  // namespace zg
