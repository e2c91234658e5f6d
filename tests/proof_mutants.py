"""Wrong proofs for the verifier's tests, made from a good one: every element of a proof located and named, then changed
one at a time.  Nothing of the library under test: the proof's shape is proof_ref.counts / proof_ref.n_point_sets, a
point's width and a scalar's byte order are the transcript reader's (tests/transcript_ref.py).

  spans(cs, N, scheme, transcript)     (kind, offset, length, label) per element, in the order proof_ref.replay reads them
  well_formed_mutants(proof, spans)    one or two per element, each a well-formed proof: only the algebra can reject it
  encoding_mutants(proof, spans)       non-canonical scalars, invalid points and wrong lengths at the first and the last
                                       element of each family

This file asserts nothing about a mutant's verdict: proof_ref.verify decides its class."""
from collections import namedtuple

import proof_ref
from circuit import R
from proof_ref import n_sets, phases_of, shuffles_of
from transcript_ref import BLAKE2B, EVM, READER, Q

POINT, SCALAR = "point", "scalar"
Span = namedtuple("Span", "kind offset length label")
Mutant = namedtuple("Mutant", "label proof span")  # span: index into the spans, None for a change of the whole proof

LOOKUP_EV = ["z(x)", "z(wx)", "a'(x)", "a'(w^-1 x)", "s'(x)"]
SHUFFLE_EV = ["z(x)", "z(wx)"]
# the families of encoding_mutants, by a label's first words
FAMILIES = [("advice commitments", ("adv c",)), ("argument commitments", ("pin ", "ptab ", "pz c", "lz ", "sz ")),
            ("quotient commitments", ("random", "h piece")), ("advice evaluations", ("adv ev",)),
            ("shared evaluations", ("fixed ev", "random ev", "sigma ev")), ("argument evaluations", ("pz ev", "lk ev", "sh ev")),
            ("opening points", ("W ",))]


def _labels(cs, N, scheme, advice_phase):
    """(front points, scalars, tail points): the names, in replay's order"""
    A, NL, S, NS, P = cs.n_advice, len(cs.lookups), n_sets(cs), len(shuffles_of(cs)), len(cs.perm_columns)
    circuits = range(N)
    front = ["adv c%d col%d" % (c, col) for cols, _ in phases_of(cs, advice_phase, []) for c in circuits for col in cols]
    front += ["%s c%d l%d" % (f, c, l) for c in circuits for l in range(NL) for f in ("pin", "ptab")]
    front += ["pz c%d set%d" % (c, s) for c in circuits for s in range(S)]
    front += ["lz c%d l%d" % (c, l) for c in circuits for l in range(NL)]
    front += ["sz c%d j%d" % (c, j) for c in circuits for j in range(NS)]
    front += ["random"] + ["h piece %d" % i for i in range(cs.degree() - 1)]
    scalars = ["adv ev c%d q%d" % (c, i) for c in circuits for i in range(len(cs.advice_queries))]
    scalars += ["fixed ev %d" % i for i in range(len(cs.fixed_queries))] + ["random ev"] + ["sigma ev %d" % pc for pc in range(P)]
    scalars += ["pz ev c%d set%d ev%d" % (c, s, e) for c in circuits for s in range(S) for e in range(3 if s + 1 < S else 2)]
    scalars += ["lk ev c%d l%d %s" % (c, l, e) for c in circuits for l in range(NL) for e in LOOKUP_EV]
    scalars += ["sh ev c%d j%d %s" % (c, j, e) for c in circuits for j in range(NS) for e in SHUFFLE_EV]
    tail = ["W %d" % i for i in range(2 if scheme == proof_ref.SHPLONK else proof_ref.n_point_sets(cs))]
    return front, scalars, tail


def spans(cs, N, scheme, transcript, advice_phase=None):
    """Every element of a proof of N circuits: the front points, every scalar, the tail points (GWC: one W per point set,
    SHPLONK: two).  advice_phase only orders the advice commitments' names (a phase's columns of every circuit, then the
    next phase's); offsets and lengths do not depend on it."""
    front, scalars, tail = _labels(cs, N, scheme, advice_phase)
    points, n_scalars = proof_ref.counts(cs, N, scheme)
    assert len(front) + len(tail) == points and len(scalars) == n_scalars, (len(front), len(tail), points, len(scalars), n_scalars)
    width = READER[transcript].point_bytes
    out, at = [], 0
    for kind, length, names in ((POINT, width, front), (SCALAR, 32, scalars), (POINT, width, tail)):
        for label in names:
            out.append(Span(kind, at, length, label))
            at += length
    # the spans tile the proof: no gap, no overlap, its whole length
    assert [s.offset for s in out] == [sum(t.length for t in out[:i]) for i in range(len(out))]
    assert at == width * points + 32 * n_scalars == proof_ref.proof_len(cs, N, scheme, transcript)
    assert len({s.label for s in out}) == len(out)
    return out


def _put(proof: bytes, span, new: bytes) -> bytes:
    assert len(new) == span.length
    return proof[:span.offset] + new + proof[span.offset + span.length:]


def _take(proof: bytes, span) -> bytes:
    return proof[span.offset:span.offset + span.length]


def _byteorder(spans_):
    """the transcript, from a point's width: 64 bytes x || y big-endian (EVM), 32 bytes compressed little-endian (BLAKE2B)"""
    width = next(s.length for s in spans_ if s.kind == POINT)
    t = {READER[t].point_bytes: t for t in (EVM, BLAKE2B)}[width]
    return t, READER[t].byteorder


def well_formed_mutants(proof: bytes, spans_):
    """Per element one proof that differs in that element only and still parses: a scalar becomes value + 1 mod r; a
    point becomes another point of the same proof with other bytes (the next such one, cyclically); a compressed point
    also becomes its negative, the sign bit flipped."""
    assert len(proof) == spans_[-1].offset + spans_[-1].length
    t, order = _byteorder(spans_)
    points = [i for i, s in enumerate(spans_) if s.kind == POINT]
    for i, s in enumerate(spans_):
        old = _take(proof, s)
        if s.kind == SCALAR:
            v = int.from_bytes(old, order)
            assert v < R
            yield Mutant(s.label + ": value + 1", _put(proof, s, ((v + 1) % R).to_bytes(32, order)), i)
            continue
        at = points.index(i)
        other = next(j for j in points[at + 1:] + points[:at] if _take(proof, spans_[j]) != old)
        yield Mutant("%s: replaced by %s" % (s.label, spans_[other].label), _put(proof, s, _take(proof, spans_[other])), i)
        if t == BLAKE2B:
            neg = bytearray(old)
            neg[31] ^= 0x80
            yield Mutant(s.label + ": negated", _put(proof, s, bytes(neg)), i)


def family(label: str) -> str:
    for name, prefixes in FAMILIES:
        if label.startswith(prefixes):
            return name
    raise AssertionError(label)


def encoding_places(spans_):
    """the first and the last element of each family that the proof has"""
    out = []
    for name, _ in FAMILIES:
        members = [i for i, s in enumerate(spans_) if family(s.label) == name]
        for i in members[:1] + members[-1:]:
            if i not in out:
                out.append(i)
    return out


def _no_root(x: int) -> int:
    """the next x at or above the given one for which x^3 + 3 has no square root in Fq"""
    while pow((x * x * x + 3) % Q, (Q - 1) // 2, Q) != Q - 1:
        x += 1
    assert x < Q
    return x


def encoding_mutants(proof: bytes, spans_):
    """At the first and the last element of each family -- scalar: exactly r, 2^256 - 1; EVM point: x + q (where it fits
    in 32 bytes), (0, 0), y + 1; compressed point: an x off the curve, the identity's encoding, 32 bytes 0xff -- and the
    whole proof one byte shorter and one byte longer."""
    t, order = _byteorder(spans_)
    for i in encoding_places(spans_):
        s = spans_[i]
        old = _take(proof, s)
        if s.kind == SCALAR:
            new = [("r", R.to_bytes(32, order)), ("2^256 - 1", b"\xff" * 32)]
        elif t == EVM:
            x, y = int.from_bytes(old[:32], "big"), int.from_bytes(old[32:], "big")
            new = [("x + q", (x + Q).to_bytes(32, "big") + old[32:])] if x + Q < 1 << 256 else []
            new += [("(0, 0)", bytes(64)), ("y + 1", old[:32] + (y + 1).to_bytes(32, "big"))]
        else:
            x = int.from_bytes(old, "little") & ((1 << 255) - 1)
            off = bytearray(_no_root(x).to_bytes(32, "little"))
            off[31] |= old[31] & 0x80
            new = [("x off the curve", bytes(off)), ("the identity", bytes(32)), ("0xff bytes", b"\xff" * 32)]
        for what, b in new:
            yield Mutant("%s: %s" % (s.label, what), _put(proof, s, b), i)
    yield Mutant("proof: the last byte cut off", proof[:-1], None)
    yield Mutant("proof: one zero byte appended", proof + b"\x00", None)
