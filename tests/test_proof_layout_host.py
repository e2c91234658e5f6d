"""csrc/proof_layout.h -- the one statement of a proof's order that prover, verifier and the proof-size functions share --
against the Python references, through tests/abi/proof_layout_probe (a stand-alone host program): the opening queries in
create_proof's order (proof_ref.circuit_queries and the shared tail), the evaluations in transcript order, GWC's point
sets (proof_ref.n_point_sets, point_set_lengths), SHPLONK's commitments, rotation sets and T
(proof_ref.intermediate_sets on the same queries), the exact lengths of all four (scheme, transcript) pairs and the
bound the ABI returns (orc.proof_size).  No device needed."""
import os
import subprocess

import proof_ref
from test_shplonk_host import CIRCUITS, many_queries_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "abi", "proof_layout_probe")
SRC = os.path.join(ROOT, "tests", "abi", "proof_layout_probe.cpp")
NS = (1, 2, 3)


class Shape:
    """What the references read of a ConstraintSystem, for a list of queries that no circuit of the suite has."""

    def __init__(self, k, n_advice, advice_queries, fixed_queries=(), n_fixed=0, perm=0, lookups=0, degree=3):
        self.k, self.n_advice, self.n_fixed, self._degree = k, n_advice, n_fixed, degree
        self.advice_queries, self.fixed_queries = list(advice_queries), list(fixed_queries)
        self.perm_columns, self.lookups = [None] * perm, [None] * lookups

    def degree(self):
        return self._degree

    def blinding_factors(self):
        per_col = {}
        for c, _ in self.advice_queries:
            per_col[c] = per_col.get(c, 0) + 1
        return max(3, max(per_col.values(), default=0)) + 2


# test_shplonk_host.py::test_intermediate_sets_on_a_hand_written_list, commitment i as advice column i: x, wx, w3x, w-1x
HAND_WRITTEN = [(0, 0), (0, 1), (1, 0), (2, -1), (2, 0), (3, 0), (3, 1), (3, 3), (4, 1), (4, 0), (5, 0)]


def shapes():
    out = {name: make()[0] for name, make in CIRCUITS.items()}
    out["many_queries"] = many_queries_circuit(5, [[0], [0, 1], [1, 2], [0, 1, 2], [2], [0, 1]])[0]
    for cs in out.values():
        cs.to_c()  # (the image the device is given: selectors compressed into fixed columns)
    out["hand_written"] = Shape(5, 6, HAND_WRITTEN)
    # rotation r and r - n are one point: one point set, one rotation set for the two columns
    out["wrapped"] = Shape(5, 2, [(0, 3), (1, 3 - 32), (0, 0), (1, 32)], fixed_queries=[(0, -31)], n_fixed=1, perm=3, lookups=1, degree=4)
    return out


def script_line(cs, N):
    head = [cs.n_advice, cs.n_fixed, len(cs.perm_columns), len(cs.lookups), proof_ref.n_sets(cs), cs.degree() - 1, cs.blinding_factors(), cs.k, N]
    for qs in (cs.advice_queries, cs.fixed_queries):
        head.append(len(qs))
        for col, rot in qs:
            head += [col, rot]
    return " ".join(str(v) for v in head)


def run(exe, tmp_path, cases):
    """cases: [(cs, N)] -> per case {"gwc": {key: tokens}, "shplonk": {...}}"""
    script = tmp_path / "layout_script.txt"
    script.write_text("\n".join(script_line(cs, N) for cs, N in cases) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out, cur = [], None
    for line in r.stdout.splitlines():
        tok = line.split()
        if tok[0] == "case":
            cur = {"gwc": {}, "shplonk": {}}
        elif tok[0] == "end":
            out.append(cur)
        else:
            cur[tok[0]][tok[1]] = tok[2:]
    assert len(out) == len(cases)
    return out


def expected_queries(cs, N):
    """(rotation, (family, circuit, index), evaluation index) in create_proof's order: every circuit's own queries
    (proof_ref.circuit_queries), then what the circuits share -- fixed queries, sigmas, h, random, the last three at 0.
    Evaluations in transcript order: every circuit's advice | fixed, random, sigma | every circuit's permutation
    evaluations (3 per set, 2 for the last) | every circuit's lookup evaluations (5 each) | the expected h(x)."""
    AQ, FQ, P, NL, S = len(cs.advice_queries), len(cs.fixed_queries), len(cs.perm_columns), len(cs.lookups), proof_ref.n_sets(cs)
    npz = 3 * S - 1 if S else 0
    ev_fix = N * AQ
    ev_rand = ev_fix + FQ
    ev_sig = ev_rand + 1
    ev_pz = ev_sig + P
    ev_lk = ev_pz + N * npz
    ev_h = ev_lk + N * 5 * NL
    poly = {"adv": lambda i: ("adv", i), "pz": lambda i: ("pz", i), "lz": lambda i: ("lz", i), "pin": lambda i: ("perm", 2 * i),
            "ptab": lambda i: ("perm", 2 * i + 1)}
    out = []
    for c in range(N):
        for rot, fam, index, key in proof_ref.circuit_queries(cs):
            ev = {"adv": lambda i: c * AQ + i, "pz": lambda s, j: ev_pz + c * npz + 3 * s + j, "lk": lambda l, j: ev_lk + c * 5 * NL + 5 * l + j}[key[0]](*key[1:])
            f, i = poly[fam](index)
            out.append((rot, (f, c, i), ev))
    out += [(rot, ("fix", 0, col), ev_fix + i) for i, (col, rot) in enumerate(cs.fixed_queries)]
    out += [(0, ("sig", 0, c), ev_sig + c) for c in range(P)]
    out += [(0, ("h", 0, 0), ev_h), (0, ("rand", 0, 0), ev_rand)]
    return out, ev_h


def poly_of(tok):
    f, c, i = tok.split(":")
    return (f, int(c), int(i))


def ints(tok):
    return [int(v) for v in tok.split(",")] if tok else []


def check_case(cs, N, got):
    n = 1 << cs.k
    want, ev_h = expected_queries(cs, N)
    for scheme in ("gwc", "shplonk"):
        g = got[scheme]
        rotations = [int(r) % n for r in g["rotations"]]
        assert len(set(rotations)) == len(rotations) == proof_ref.n_point_sets(cs)
        queries = []
        for tok in g["queries"]:
            p, rest = tok.split("@")
            point, ev = rest.split("=")
            queries.append((rotations[int(point)], poly_of(p), int(ev)))
        assert queries == [(rot % n, p, ev) for rot, p, ev in want]
        # points by first appearance
        first = []
        for rot, _, _ in queries:
            if rot not in first:
                first.append(rot)
        assert rotations == first
        # the evaluations in transcript order are the queries by evaluation index, each evaluation once, h(x) last
        by_ev = sorted(queries, key=lambda q: q[2])
        assert [q[2] for q in by_ev] == list(range(ev_h + 1))
        assert [(poly_of(t.split("@")[0]), rotations[int(t.split("@")[1])]) for t in g["transcript"]] == [(q[1], q[0]) for q in by_ev]
        code = proof_ref.SHPLONK if scheme == "shplonk" else proof_ref.GWC
        points, scalars = proof_ref.counts(cs, N=N, scheme=code)
        sizes = dict(zip(g["sizes"][::2], (int(v) for v in g["sizes"][1::2])))
        assert (sizes["points"], sizes["scalars"]) == (points, scalars) and scalars == ev_h
        assert sizes["evm"] == proof_ref.proof_len(cs, N=N, scheme=code, transcript=proof_ref.EVM)
        assert sizes["blake2b"] == proof_ref.proof_len(cs, N=N, scheme=code, transcript=proof_ref.BLAKE2B)
        # the families tile the points and the evaluations in the stated order; the Blake2b items: the evaluations stand
        # between the h pieces and the argument's points
        fam = [t.split(":") for t in g["points"]]
        A, NL, S = cs.n_advice, len(cs.lookups), proof_ref.n_sets(cs)
        tail = 2 if scheme == "shplonk" else len(rotations)
        assert [(f, int(c)) for f, _, c in fam] == [("adv", N * A), ("perm", N * 2 * NL), ("pz", N * S), ("lz", N * NL), ("rand", 1),
                                                   ("hp", cs.degree() - 1), ("open", tail)]
        assert [int(a) for _, a, _ in fam] == [sum(int(c) for _, _, c in fam[:i]) for i in range(len(fam))]
        before = points - tail
        assert [int(v) for v in g["items"]] == list(range(before)) + [before + scalars + i for i in range(tail)]
        evf = [t.split(":") for t in g["evals"]]
        assert [f for f, _, _ in evf] == ["adv", "fix", "rand", "sig", "pz", "lk", "h"]
        assert [int(a) for _, a, _ in evf] == [sum(int(c) for _, _, c in evf[:i]) for i in range(len(evf))] and int(evf[-1][1]) == ev_h
        max_open = 2 if scheme == "shplonk" else 2 + len(cs.advice_queries) + len(cs.fixed_queries)
        assert sizes["bound_evm"] == sizes["evm"] + 64 * (max_open - tail) and sizes["bound_blake2b"] == sizes["blake2b"] + 32 * (max_open - tail)
    # GWC: one set per point, its queries in order
    sets = [ints(t) for t in got["gwc"]["sets"]]
    qs = [(rot % n, p) for rot, p, _ in want]
    assert sets == [[i for i, q in enumerate(qs) if q[0] == rot] for rot in rotations]
    assert {rot: len(s) for rot, s in zip(rotations, sets)} == proof_ref.point_set_lengths(cs, N)
    # SHPLONK: proof_ref.intermediate_sets on the same queries
    ref_sets, T = proof_ref.intermediate_sets(qs)
    g = got["shplonk"]
    coms = []
    for tok in g["coms"]:
        p, s, place, q = tok.split("/")
        coms.append((poly_of(p), int(s), int(place), ints(q)))
    got_sets = [(ints(t.split("/")[0]), ints(t.split("/")[1])) for t in g["sets"]]
    assert [c[0] for c in coms] == [key for key in dict.fromkeys(p for _, p in qs)]  # first appearance
    assert [[coms[c][0] for c in cs_] for _, cs_ in got_sets] == [keys for _, keys in ref_sets]
    assert [set(rotations[p] for p in pts) for pts, _ in got_sets] == [set(pts) for pts, _ in ref_sets]
    assert all(pts == sorted(pts) for pts, _ in got_sets)
    assert T == rotations and int(g["T"][0]) == len(T) and int(g["T"][2]) == sum(len(pts) for pts, _ in ref_sets)
    for ci, (p, s, place, q) in enumerate(coms):
        assert got_sets[s][1][place] == ci
        # one query per point of the set, in the set's order: the first that opens the commitment there
        assert [qs[i] for i in q] == [(rotations[pt], p) for pt in got_sets[s][0]]
        assert all(i == qs.index(qs[i]) for i in q)


def check(exe, tmp_path):
    all_shapes = shapes()
    cases = [(cs, N) for cs in all_shapes.values() for N in NS]
    for (cs, N), got in zip(cases, run(exe, tmp_path, cases)):
        check_case(cs, N, got)
    return all_shapes


def test_the_shapes_cover_what_they_are_here_for():
    s = shapes()
    n = 32
    qs = [(r % n, p) for r, p, _ in expected_queries(s["many_queries"], 1)[0]]
    assert len(set(frozenset(p) for p, _ in proof_ref.intermediate_sets(qs)[0])) >= 4
    sets, T = proof_ref.intermediate_sets([(r % n, p) for r, p, _ in expected_queries(s["hand_written"], 1)[0]])
    adv = [[k[2] for k in keys if k[0] == "adv"] for _, keys in sets]
    assert adv == [[0, 4], [1, 5], [2], [3]] and [len(p) for p, _ in sets] == [2, 1, 2, 3] and len(T) == 4
    # 3 = -29 and 0 = 32: the two advice columns share the rotation set {3, 0}; 1 = -31 puts the fixed column with z(wx)
    sets, T = proof_ref.intermediate_sets([(r % n, p) for r, p, _ in expected_queries(s["wrapped"], 1)[0]])
    assert sets[0] == ([3, 0], [("adv", 0, 0), ("adv", 0, 1)])
    assert proof_ref.n_point_sets(s["wrapped"]) == len(T) == 5 and sorted(T) == [0, 1, 3, 26, 31]
    assert len(s["two_lookups"].lookups) == 2 and proof_ref.n_sets(s["toy"]) == 2


def test_host_build_meets_the_references(tmp_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    check(EXE, tmp_path)


def test_the_bound_is_the_oracles_proof_size(orc, tmp_path):
    """GWC with the EVM transcript at N = 1: what zg_prover_proof_size returns, pinned to orc.proof_size by the GPU tests"""
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    made = {name: make()[0] for name, make in CIRCUITS.items()}
    made["many_queries"] = many_queries_circuit(5, [[0], [0, 1], [1, 2], [0, 1, 2], [2], [0, 1]])[0]
    images = {name: cs.to_c() for name, cs in made.items()}
    got = run(EXE, tmp_path, [(cs, 1) for cs in made.values()])
    for (name, img), g in zip(images.items(), got):
        cs, c = made[name], img.c  # (the references' view of the circuit is the image's)
        assert (c.n_advice, c.n_fixed, c.n_perm_columns, c.n_lookups, c.cs_degree, c.blinding_factors, c.k) == (
            cs.n_advice, cs.n_fixed, len(cs.perm_columns), len(cs.lookups), cs.degree(), cs.blinding_factors(), cs.k)
        assert [(q.column, q.rotation) for q in c.advice_queries[:c.n_advice_queries]] == cs.advice_queries
        assert [(q.column, q.rotation) for q in c.fixed_queries[:c.n_fixed_queries]] == cs.fixed_queries
        sizes = dict(zip(g["gwc"]["sizes"][::2], (int(v) for v in g["gwc"]["sizes"][1::2])))
        assert sizes["bound_evm"] == orc.proof_size(img), name


def test_host_build_under_the_sanitizers(tmp_path):
    """a second build of the probe under UBSan and ASan (a stand-alone host program: nothing preloaded, nothing loaded into
    Python); the first finding ends it"""
    exe = str(tmp_path / "proof_layout_probe_san")
    subprocess.run(["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
                    "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe], check=True)
    check(exe, tmp_path)
