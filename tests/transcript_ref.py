"""The two transcripts of the proof tests, writer and reader each, restated on Python integers -- nothing of the library
under test.  Written from the published sources (include/zg_halo2.h states the rules; DESIGN.md section 17 lists what
remains to be verified against the crates).

  EVM       snark-verifier's EvmTranscript (oracle/prover.c tr_*): Keccak-256 over the pending input, big-endian scalars,
            points as 64 bytes x || y
  BLAKE2B   halo2_proofs v2023_04_20 src/transcript/blake2b.rs (Blake2bWrite / Blake2bRead with Challenge255) over hashlib,
            little-endian scalars, points in halo2curves 0.3.3's 32-byte GroupEncoding (compress / decompress)

A transcript is chosen by argument: WRITER[t] / READER[t] with t = EVM or BLAKE2B, the library's own codes.  A point's
width in the stream is the transcript's (point_bytes).  A writer absorbs and appends to `out`; a reader absorbs what it
reads from the proof and remembers the first failure (`bad`: the stream ran out, a scalar not below r, a point that is no
canonical encoding of a curve point other than the identity); reader.writer(keccak) is a writer that goes on where the
reader stands.  Points are affine integer pairs (x, y)."""
import hashlib

import orc
from circuit import R

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
EVM, BLAKE2B = 0, 1
PERSONAL = b"Halo2-Transcript"


def hasher():
    return hashlib.blake2b(digest_size=64, person=PERSONAL)


def le32(v: int) -> bytes:
    return v.to_bytes(32, "little")


def challenge(digest: bytes) -> int:
    """Challenge255::new: the 64-byte digest as a little-endian integer mod r"""
    return int.from_bytes(digest, "little") % R


def fq_sqrt(t: int):
    """a root of t in Fq, or None (q = 3 mod 4)"""
    y = pow(t, (Q + 1) // 4, Q)
    return y if y * y % Q == t % Q else None


def compress(x: int, y: int) -> bytes:
    """G1Affine::to_bytes; (0, 0) is the identity"""
    if (x, y) == (0, 0):
        return bytes(32)
    b = bytearray(le32(x))
    b[31] |= (y & 1) << 7
    return bytes(b)


def decompress(b: bytes):
    """G1Affine::from_bytes -> (x, y), (0, 0) for the identity, None for an invalid encoding"""
    b = bytearray(b)
    sign = b[31] >> 7
    b[31] &= 0x7F
    x = int.from_bytes(b, "little")
    if x >= Q:
        return None
    if x == 0 and sign == 0:
        return (0, 0)
    y = fq_sqrt((x * x * x + 3) % Q)
    if y is None:
        return None
    return (x, Q - y if (y & 1) != sign else y)


# ---------------------------------------------------------------------------------------------------- what each absorbs
class _Evm:
    point_bytes, byteorder = 64, "big"

    def __init__(self, keccak):
        self.keccak, self.buf = keccak, b""

    def adopt(self, other):
        self.buf = other.buf

    def common_scalar(self, v: int):
        self.buf += (v % R).to_bytes(32, "big")

    def common_point(self, pt):
        self.buf += self.encode(pt)

    def squeeze(self) -> int:
        h = self.keccak(self.buf + (b"\x01" if len(self.buf) == 32 else b""))
        self.buf = h
        return int.from_bytes(h, "big") % R

    @staticmethod
    def encode(pt) -> bytes:
        return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")

    @staticmethod
    def decode(b: bytes):
        x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
        if x >= Q or y >= Q or (y * y - x * x * x - 3) % Q != 0:  # canonical coordinates, on the curve ((0, 0) is not)
            return None
        return (x, y)


class _Blake2b:
    point_bytes, byteorder = 32, "little"

    def __init__(self, keccak=None):  # (the backend's Keccak, as the walkers pass it: not used)
        self.h = hasher()

    def adopt(self, other):
        self.h = other.h.copy()

    def common_scalar(self, v: int):
        self.h.update(b"\x02" + le32(v % R))

    def common_point(self, pt):
        self.h.update(b"\x01" + le32(pt[0]) + le32(pt[1]))

    def squeeze(self) -> int:
        self.h.update(b"\x00")
        return challenge(self.h.copy().digest())

    @staticmethod
    def encode(pt) -> bytes:
        return compress(*pt)

    @staticmethod
    def decode(b: bytes):
        xy = decompress(b)
        return None if xy == (0, 0) else xy  # the identity, which common_point refuses


# ---------------------------------------------------------------------------------------------------- writing and reading
class _Writer:
    def __init__(self, keccak=None):
        super().__init__(keccak)
        self.out = bytearray()

    def write_scalar(self, v: int):
        self.common_scalar(v)
        self.out += (v % R).to_bytes(32, self.byteorder)

    def write_point(self, pt):
        assert tuple(pt) != (0, 0), "the transcript cannot absorb the identity"
        self.common_point(pt)
        self.out += self.encode(pt)


class _Reader:
    def __init__(self, proof: bytes, keccak=orc.keccak256):
        super().__init__(keccak)
        self.data, self.pos, self.bad = bytes(proof), 0, False

    def _take(self, count: int):
        if self.pos + count > len(self.data):
            self.bad = True
            return None
        self.pos += count
        return self.data[self.pos - count:self.pos]

    def scalar(self) -> int:
        b = self._take(32)
        if b is None or int.from_bytes(b, self.byteorder) >= R:
            self.bad = True
            return 0
        v = int.from_bytes(b, self.byteorder)
        self.common_scalar(v)
        return v

    def point(self):
        b = self._take(self.point_bytes)
        pt = None if b is None else self.decode(b)
        if pt is None:
            self.bad = True
            return None
        self.common_point(pt)
        return pt

    def writer(self, keccak=None):
        """a writer in this reader's state, its output what has been read"""
        w = self.Writer(keccak or getattr(self, "keccak", None))
        w.adopt(self)
        w.out = bytearray(self.data[:self.pos])
        return w


class EvmWriter(_Writer, _Evm):
    pass


class Blake2bWriter(_Writer, _Blake2b):
    pass


class EvmReader(_Reader, _Evm):
    Writer = EvmWriter


class Blake2bReader(_Reader, _Blake2b):
    Writer = Blake2bWriter


WRITER = {EVM: EvmWriter, BLAKE2B: Blake2bWriter}
READER = {EVM: EvmReader, BLAKE2B: Blake2bReader}
