"""Inputs shared by tests/test_transcript_host.py and tests/test_gpu_transcript.py: the edge encodings of G1 points
(halo2curves' 32-byte GroupEncoding) and the record of the golden Blake2b proof."""
import os

import field9_ref as ref
import transcript_ref as b2

Q = b2.Q
GOLDEN_B2_N2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blake2b_n2.json")


def has_point(x: int) -> bool:
    return b2.fq_sqrt((x * x * x + 3) % Q) is not None


def smallest_x(with_point: bool) -> int:
    x = 1
    while has_point(x) != with_point:
        x += 1
    return x


def signed(x: int, sign: int) -> bytes:
    b = bytearray(b2.le32(x))
    b[31] |= sign << 7
    return bytes(b)


def edge_encodings() -> dict:
    """name -> 32 bytes; what each decodes to is for transcript_ref.decompress to say"""
    P = ref.ec_mul(5, ref.G)
    bit6 = bytearray(b2.compress(*P))
    bit6[31] |= 0x40
    out = {
        "a point": b2.compress(*P),
        "its negative": b2.compress(*ref.ec_neg(P)),
        "bit 6 set": bytes(bit6),
        "x = 0, sign 0 (the identity)": bytes(32),
        "x = 0, sign 1": signed(0, 1),
    }
    for sign in (0, 1):
        out["x = q - 1, sign %d" % sign] = signed(Q - 1, sign)
        out["x = q, sign %d" % sign] = signed(Q, sign)
        out["the smallest x >= 1 without a point, sign %d" % sign] = signed(smallest_x(False), sign)
        out["the smallest x with a point, sign %d" % sign] = signed(smallest_x(True), sign)
    return out
