"""The comparator of the Blake2b-transcript tests: halo2's own transcript (halo2_proofs v2023_04_20 src/transcript/blake2b.rs:
Blake2bWrite / Blake2bRead with Challenge255) and halo2curves 0.3.3's 32-byte GroupEncoding of G1, restated on Python
integers and hashlib -- nothing of the library under test.  Written from the published sources (include/zg_halo2.h states
the rules; DESIGN.md section 17 lists what remains to be verified against the crates).

  Transcript / _Reader   writer and reader with the method names of arith_level.Transcript and multi_ref._Reader: the
                         walkers of tests/arith_level.py, tests/multi_ref.py and tests/shplonk_ref.py look their transcript
                         class up as a module attribute, so `use(monkeypatch)` swaps these in without editing those files
  compress / decompress  GroupEncoding on integers
  proof_len              32 bytes per item
  shplonk_create_proof   shplonk_ref.create_proof restated for this transcript: that walker cuts the GWC tail off by its
                         64-byte points and hands the Keccak buffer over, which a class swap cannot reach
"""
import hashlib

import numpy as np

import arith_level
import multi_ref
import orc
import shplonk_ref
from circuit import R

Q = multi_ref.Q
GWC, SHPLONK = 0, 1
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


class Transcript:
    """Blake2bWrite.  The constructor takes and ignores the backend's Keccak, as arith_level.create_proof passes it."""

    def __init__(self, keccak=None):
        self.h, self.out = hasher(), bytearray()

    def common_scalar(self, v: int):
        self.h.update(b"\x02" + le32(v % R))

    def write_scalar(self, v: int):
        self.common_scalar(v)
        self.out += le32(v % R)

    def write_point(self, pt):
        x, y = pt
        assert (x, y) != (0, 0), "the transcript cannot absorb the identity"
        self.h.update(b"\x01" + le32(x) + le32(y))
        self.out += compress(x, y)

    def squeeze(self) -> int:
        self.h.update(b"\x00")
        return challenge(self.h.copy().digest())


class _Reader:
    """Blake2bRead: the running hash, the proof stream, the first failure."""

    def __init__(self, proof: bytes):
        self.h, self.data, self.pos, self.bad = hasher(), bytes(proof), 0, False

    def common_scalar(self, v: int):
        self.h.update(b"\x02" + le32(v % R))

    def point(self):
        if self.pos + 32 > len(self.data):
            self.bad = True
            return None
        xy = decompress(self.data[self.pos:self.pos + 32])
        self.pos += 32
        if xy is None or xy == (0, 0):  # an invalid encoding; the identity, which common_point refuses
            self.bad = True
            return None
        self.h.update(b"\x01" + le32(xy[0]) + le32(xy[1]))
        return multi_ref._point(*xy)

    def scalar(self):
        if self.pos + 32 > len(self.data):
            self.bad = True
            return 0
        v = int.from_bytes(self.data[self.pos:self.pos + 32], "little")
        self.pos += 32
        if v >= R:
            self.bad = True
            return 0
        self.h.update(b"\x02" + le32(v))
        return v

    def squeeze(self) -> int:
        self.h.update(b"\x00")
        return challenge(self.h.copy().digest())


def use(monkeypatch):
    """the walkers of arith_level, multi_ref and shplonk_ref on this transcript, for the rest of the test"""
    monkeypatch.setattr(arith_level, "Transcript", Transcript)
    monkeypatch.setattr(multi_ref, "_Reader", _Reader)
    monkeypatch.setattr(shplonk_ref, "_Reader", _Reader)


def counts(cs, N: int, scheme: int):
    """(points, scalars) of a proof of N circuits"""
    A, NL, S, P, d = cs.n_advice, len(cs.lookups), multi_ref.n_sets(cs), len(cs.perm_columns), cs.degree()
    AQ, FQ = len(cs.advice_queries), len(cs.fixed_queries)
    tail = 2 if scheme == SHPLONK else multi_ref.n_point_sets(cs)
    return (N * (A + 3 * NL + S) + 1 + (d - 1) + tail, N * (AQ + (3 * S - 1 if S else 0) + 5 * NL) + FQ + 1 + P)


def proof_len(cs, N: int = 1, scheme: int = GWC) -> int:
    points, scalars = counts(cs, N, scheme)
    return 32 * (points + scalars)


def verify(vk, instances, proof: bytes, scheme: int = GWC) -> int:
    """the reference verifier of the scheme (its transcript classes swapped by `use`)"""
    assert multi_ref._Reader is _Reader and shplonk_ref._Reader is _Reader, "call blake2b_ref.use(monkeypatch) first"
    if scheme == SHPLONK:
        return shplonk_ref.verify(vk, instances, proof, circuits=len(instances))
    return multi_ref.verify(vk, instances, proof)


def create_proof(be, vk, advice, instance, scheme: int = GWC) -> bytes:
    """the caller-walked prover of the scheme over a backend of tests/arith_level.py, one circuit"""
    assert issubclass(arith_level.Transcript, Transcript), "call blake2b_ref.use(monkeypatch) first"
    if scheme == SHPLONK:
        return shplonk_create_proof(be, vk, advice, instance)
    cs = vk.cs
    if not cs.n_instance:
        return arith_level.create_proof(be, shplonk_ref._OneEmptyInstanceColumn(cs), orc.fr_from_int(vk.vk_repr), advice,
                                        np.zeros((1, 0, 4), np.uint64))
    return arith_level.create_proof(be, cs, orc.fr_from_int(vk.vk_repr), advice, instance)


def shplonk_create_proof(be, vk, advice, instance) -> bytes:
    """shplonk_ref.create_proof, its steps and helpers, with 32-byte points in the GWC tail that is cut off and the running
    hash of the reader handed to the writer."""
    sr = shplonk_ref
    cs = vk.cs
    rec = sr._Recorder(be)
    gwc = create_proof(rec, vk, advice, instance, GWC)
    prefix = gwc[:len(gwc) - 32 * multi_ref.n_point_sets(cs)]
    t, x, qs = sr._replay(vk, [instance], prefix)
    assert t is not None and t.pos == len(prefix)
    adv_p, _, pz_p, lz_p, perm_p = rec.coeff
    poly = {("h",): rec.h_poly, ("random",): rec.random_poly}
    for key in {q[1] for q in qs}:
        if key[0] == 0:
            fam, idx = key[1], key[2]
            poly[key] = {"adv": adv_p, "pz": pz_p, "lz": lz_p}[fam][idx] if fam in ("adv", "pz", "lz") else \
                perm_p[2 * idx + (fam == "ptab")]
        elif key[0] == "fixed":
            poly[key] = be.fixed_polys[key[1]]
        elif key[0] == "sigma":
            poly[key] = be.sigma_polys[key[1]]
    tr = Transcript()
    tr.h, tr.out = t.h.copy(), bytearray(prefix)

    y, v = tr.squeeze(), tr.squeeze()
    sets, T = sr.intermediate_sets([(q[0], q[1]) for q in qs])
    evals = {(q[1], q[0]): q[3] for q in qs}
    quotients = be.zeros(len(sets))
    work = be.zeros(2)
    for i, (points, keys) in enumerate(sets):
        ypow = [pow(y, j, R) for j in range(len(keys))]
        be.lincomb([poly[key] for key in keys], ypow, None, work[0])
        low = [0] * len(points)
        for yj, key in zip(ypow, keys):
            rij = sr._interpolate(points, [evals[key, p] for p in points])
            low = [(a + yj * c) % R for a, c in zip(low, rij)]
        be.put(work[0], 0, sr._one_column(be, [(be.get1(work[0], d) - low[d]) % R for d in range(len(points))]), 0, len(points))
        src, dst = work[0], work[1]
        for r in points:
            be.kate(src, r, dst)
            src, dst = dst, src
        be.lincomb([src], [1], None, quotients[i])
    h1 = be.zeros(1)[0]
    be.lincomb([quotients[i] for i in range(len(sets))], [pow(v, i, R) for i in range(len(sets))], None, h1)
    tr.write_point(be.commit(h1[None], False)[0])
    u = tr.squeeze()

    def z_of(points):
        acc = 1
        for r in T:
            if r not in points:
                acc = acc * (u - r) % R
        return acc

    zT = z_of([])
    terms, coeffs, const = [], [], 0
    for i, (points, keys) in enumerate(sets):
        wi = pow(v, i, R) * z_of(points) % R
        for j, key in enumerate(keys):
            c = wi * pow(y, j, R) % R
            terms.append(poly[key])
            coeffs.append(c)
            const = (const + c * sr._lagrange_at(points, [evals[key, p] for p in points], u)) % R
    be.lincomb(terms + [h1], coeffs + [(-zT) % R], const, work[0])
    be.kate(work[0], u, work[1])
    h2 = be.zeros(1)[0]
    be.lincomb([work[1]], [sr._inv(z_of(sets[0][0]))], None, h2)
    tr.write_point(be.commit(h2[None], False)[0])
    return bytes(tr.out)
