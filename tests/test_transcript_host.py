"""The host side of halo2's Blake2b transcript with compressed points, on a machine without a GPU:
csrc/blake2b.h, the Blake2bTranscript of csrc/transcript.h and the host path of csrc/g1_compress.h through the stand-alone
program tests/abi/transcript_probe.hip, against hashlib and Python integers (tests/transcript_ref.py); and the golden Blake2b
proof of two circuits, made on the GPU, against the reference verifier."""
import hashlib
import json
import os
import subprocess

import field9_ref as ref
import proof_ref
import transcript_cases as tc
import transcript_ref as b2
from circuit import R
from test_gpu_multi import toy_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "abi", "transcript_probe")
Q = b2.Q


def run(exe, tmp_path, lines):
    script = tmp_path / "script.txt"
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


def pattern(n: int) -> bytes:
    return bytes((11 * i + n) & 0xFF for i in range(n))


def le(v: int) -> str:
    return b2.le32(v).hex()


# ---- the cases: (script line, expected output line)
def blake2b_cases():
    cases = []
    for n in (0, 1, 127, 128, 129, 255, 256, 257, 1152):
        h = b2.hasher()
        h.update(pattern(n))
        cases.append(("hash " + hx(pattern(n)), h.hexdigest()))
    # the streaming state: a digest exactly at the end of a block, one byte later, and after two more blocks and a half
    h, want = b2.hasher(), []
    parts = [pattern(128), b"\x00", pattern(320)]
    for p in parts:
        h.update(p)
        want.append(h.copy().hexdigest())
    cases.append(("raw " + " ".join("a%s q" % p.hex() for p in parts), " ".join(want) + " "))
    # the reduction of the largest digest
    cases.append(("wide " + "ff" * 64, le(((1 << 512) - 1) % R)))
    cases.append(("wide " + (b2.le32(R) + b2.le32(0)).hex(), le(0)))
    cases.append(("wide " + (b2.le32(R - 1) + b2.le32(R - 1)).hex(), le((R - 1 + ((R - 1) << 256)) % R)))
    return cases


def transcript_cases():
    """squeeze - absorb - squeeze: 31 scalars are 1023 bytes, so the first squeeze's 0x00 ends the eighth block exactly and
    the second squeeze finalises one byte later; then points and scalars into the proof, and the identity refused"""
    rng_vals = [(0x1234567 * (i + 1) ** 3) % R for i in range(31)]
    P, S = ref.ec_mul(7, ref.G), ref.ec_mul(11, ref.G)
    t = b2.Blake2bWriter()
    toks, outs = [], []
    for v in rng_vals:
        t.common_scalar(v)
        toks.append("c" + le(v))
    totals = [33 * 31 + 1, 33 * 31 + 2]
    assert totals[0] % 128 == 0 and totals[1] % 128 == 1
    for _ in range(2):
        outs.append(le(t.squeeze()))
        toks.append("q")
    t.write_point(P)
    toks.append("p%s,%s" % (le(P[0]), le(P[1])))
    t.write_scalar(R - 1)
    toks.append("s" + le(R - 1))
    outs.append(le(t.squeeze()))
    toks.append("q")
    t.write_point(ref.ec_neg(S))
    toks.append("p%s,%s" % (le(S[0]), le(Q - S[1])))
    outs.append(le(t.squeeze()))
    toks.append("q")
    first = ("tr " + " ".join(toks), " ".join(outs) + " stream=%s failed=0" % bytes(t.out).hex())
    ident = ("tr p%s,%s q" % (le(0), le(0)), "%s stream=- failed=1" % le(b2.Blake2bWriter().squeeze()))
    return [first, ident]


def point_cases():
    cases = []
    valid = 0
    for name, enc in tc.edge_encodings().items():
        xy = b2.decompress(enc)
        want = "0 %s %s" % (le(0), le(0)) if xy is None else "1 %s %s" % (le(xy[0]), le(xy[1]))
        cases.append(("dec " + enc.hex(), want))
        if xy is not None:
            valid += 1
            assert ref.on_curve(None if xy == (0, 0) else xy)
            cases.append(("cmp %s %s" % (le(xy[0]), le(xy[1])), enc.hex()))  # compress(decompress(e)) == e
    assert valid >= 6
    return cases


def all_cases():
    return blake2b_cases() + transcript_cases() + point_cases()


def check(exe, tmp_path):
    cases = all_cases()
    got = run(exe, tmp_path, [c[0] for c in cases])
    bad = [(c[0][:60], g[:140], c[1][:140]) for c, g in zip(cases, got) if g != c[1]]
    assert not bad, "%d of %d lines differ, the first: %s" % (len(bad), len(cases), bad[0])


def test_the_reference_is_hashlibs_blake2b_and_the_edge_cases_are_what_they_say():
    assert b2.hasher().digest() == hashlib.blake2b(b"", digest_size=64, person=b"Halo2-Transcript").digest()
    assert b2.hasher().digest() != hashlib.blake2b(b"", digest_size=64).digest()
    assert Q % 4 == 3 and pow(3, (Q - 1) // 2, Q) == Q - 1  # the root is t^((q+1)/4); 3 is a non-residue
    e = tc.edge_encodings()
    P = ref.ec_mul(5, ref.G)
    assert b2.decompress(e["a point"]) == P and b2.decompress(e["its negative"]) == ref.ec_neg(P)
    assert b2.decompress(e["bit 6 set"]) is None and b2.decompress(e["x = q, sign 0"]) is None
    assert b2.decompress(e["x = 0, sign 0 (the identity)"]) == (0, 0) and b2.decompress(e["x = 0, sign 1"]) is None
    assert b2.decompress(e["the smallest x >= 1 without a point, sign 1"]) is None
    x = tc.smallest_x(True)
    lo, hi = (b2.decompress(e["the smallest x with a point, sign %d" % s]) for s in (0, 1))
    assert lo[0] == hi[0] == x and lo[1] & 1 == 0 and hi[1] == Q - lo[1]


def test_host_build_meets_hashlib_and_the_integers(tmp_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    check(EXE, tmp_path)


def test_host_build_under_the_sanitizers(tmp_path):
    """a second, stand-alone build of the probe with the host code under UBSan and ASan (nothing preloaded, nothing loaded
    into Python); the first finding ends it"""
    exe = str(tmp_path / "transcript_probe_san")
    subprocess.run(["hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
                    "-fno-sanitize-recover=all", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi", "transcript_probe.hip"), "-o", exe], check=True)
    check(exe, tmp_path)


def test_golden_proof_of_two_circuits(orc):
    """the device prover's Blake2b proof of two toy circuits (k = 5, GWC; tests/test_gpu_transcript.py holds the prover to
    these bytes): the reference verifier accepts it, and rejects it with the instances swapped"""
    rec = json.load(open(tc.GOLDEN_B2_N2))
    family = toy_family(2)
    cs, asg, ilen = family[0]
    params = orc.params_new(cs.k, rec["params_seed"])
    vk = proof_ref.Vk(cs, params, asg.fixed_values(), asg.sigma_values(), orc.fr_from_int(rec["vk_repr"]))
    inst = [a.instance_values(ilen) for _, a, _ in family]
    proof = bytes.fromhex(rec["proof"])

    def verdict(instances, p) -> int:
        return proof_ref.verify(vk, instances, p, transcript=b2.BLAKE2B).verdict

    assert len(proof) == proof_ref.proof_len(cs, N=2, transcript=b2.BLAKE2B) < proof_ref.proof_len(cs, N=2)
    assert verdict(inst, proof) == 1
    assert verdict([inst[1], inst[0]], proof) == 0
    assert verdict(inst, proof + b"\x00") == 0
    assert verdict(inst, proof[:-1]) == -1
    flipped = bytearray(proof)
    flipped[31] ^= 0x80  # the first commitment's sign: its negative
    assert verdict(inst, bytes(flipped)) == 0
