"""The shuffle argument without a device: csrc/proof_layout.h with NS shuffles against tests/proof_ref.py's order,
through tests/abi/shuffle_layout_probe (a stand-alone host program); the ABI's new entries and zg_shuffle's layout;
proof_ref against the oracle on circuits without shuffles; the test circuits themselves."""
import ctypes
import json
import os
import subprocess

import pytest

import proof_ref
import shuffle_circuits
import test_proof_layout_host as plh
from circuits import toy_circuit, variant_circuit
from test_abi import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "abi", "shuffle_layout_probe")
SRC = os.path.join(ROOT, "tests", "abi", "shuffle_layout_probe.cpp")
OLD_EXE = os.path.join(ROOT, "tests", "abi", "proof_layout_probe")
NEW_ENTRIES = ["zg_prover_create_shuffles", "zg_prover_create_shared_shuffles", "zg_prover_shuffles", "zg_verifier_create_shuffles"]
GWC, SHPLONK, EVM, BLAKE2B = 0, 1, 0, 1


def with_shuffles(cs, ns):
    cs.shuffles = [None] * ns
    return cs


def script_line(cs, N):
    tok = plh.script_line(cs, N).split()
    return " ".join(tok[:9] + [str(len(proof_ref.shuffles_of(cs)))] + tok[9:])


def run(exe, tmp_path, cases, line=script_line):
    script = tmp_path / "shuffle_script.txt"
    script.write_text("\n".join(line(cs, N) for cs, N in cases) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def parse(stdout, count):
    out, cur = [], None
    for ln in stdout.splitlines():
        tok = ln.split()
        if tok[0] == "case":
            cur = {"gwc": {}, "shplonk": {}}
        elif tok[0] == "end":
            out.append(cur)
        else:
            cur[tok[0]][tok[1]] = tok[2:]
    assert len(out) == count
    return out


def expected_queries(cs):
    """(rotation, (family, 0, index), evaluation index) of ONE circuit in create_proof's order, from proof_ref.circuit_queries
    and the shared tail; the evaluations in transcript order: advice | fixed, random, sigma | permutation | lookups |
    shuffles (z, z(wx) each) | the expected h(x)"""
    AQ, FQ, P, NL, S = len(cs.advice_queries), len(cs.fixed_queries), len(cs.perm_columns), len(cs.lookups), proof_ref.n_sets(cs)
    NS = len(proof_ref.shuffles_of(cs))
    ev_fix = AQ
    ev_rand = ev_fix + FQ
    ev_sig = ev_rand + 1
    ev_pz = ev_sig + P
    ev_lk = ev_pz + (3 * S - 1 if S else 0)
    ev_sh = ev_lk + 5 * NL
    ev_h = ev_sh + 2 * NS
    poly = {"adv": lambda i: ("adv", i), "pz": lambda i: ("pz", i), "lz": lambda i: ("lz", i), "pin": lambda i: ("perm", 2 * i),
            "ptab": lambda i: ("perm", 2 * i + 1), "sz": lambda i: ("sz", i)}
    where = {"adv": lambda i: i, "pz": lambda s, j: ev_pz + 3 * s + j, "lk": lambda l, j: ev_lk + 5 * l + j, "sh": lambda j, e: ev_sh + 2 * j + e}
    out = []
    for rot, fam, index, key in proof_ref.circuit_queries(cs):
        f, i = poly[fam](index)
        out.append((rot, (f, 0, i), where[key[0]](*key[1:])))
    out += [(rot, ("fix", 0, col), ev_fix + i) for i, (col, rot) in enumerate(cs.fixed_queries)]
    out += [(0, ("sig", 0, c), ev_sig + c) for c in range(P)]
    out += [(0, ("h", 0, 0), ev_h), (0, ("rand", 0, 0), ev_rand)]
    return out, ev_sh, ev_h


def check_case(cs, got):
    n, NS = 1 << cs.k, len(proof_ref.shuffles_of(cs))
    A, NL, S = cs.n_advice, len(cs.lookups), proof_ref.n_sets(cs)
    want, ev_sh, ev_h = expected_queries(cs)
    qs = [(rot % n, p) for rot, p, _ in want]
    for scheme in ("gwc", "shplonk"):
        g = got[scheme]
        code = SHPLONK if scheme == "shplonk" else GWC
        rotations = [int(r) % n for r in g["rotations"]]
        assert len(set(rotations)) == len(rotations) == proof_ref.n_point_sets(cs)
        queries = []
        for tok in g["queries"]:
            p, rest = tok.split("@")
            point, ev = rest.split("=")
            queries.append((rotations[int(point)], plh.poly_of(p), int(ev)))
        assert queries == [(rot % n, p, ev) for rot, p, ev in want]
        assert rotations == list(dict.fromkeys(q[0] for q in queries))  # points by first appearance
        by_ev = sorted(queries, key=lambda q: q[2])
        assert [q[2] for q in by_ev] == list(range(ev_h + 1))
        assert [(plh.poly_of(t.split("@")[0]), rotations[int(t.split("@")[1])]) for t in g["transcript"]] == [(q[1], q[0]) for q in by_ev]
        # lengths: both transcripts, and the bounds
        points, scalars = proof_ref.counts(cs, N=1, scheme=code)
        sizes = dict(zip(g["sizes"][::2], (int(v) for v in g["sizes"][1::2])))
        assert (sizes["points"], sizes["scalars"]) == (points, scalars) and scalars == ev_h
        assert sizes["evm"] == proof_ref.proof_len(cs, scheme=code, transcript=EVM) and sizes["blake2b"] == proof_ref.proof_len(cs, scheme=code, transcript=BLAKE2B)
        tail = 2 if scheme == "shplonk" else len(rotations)
        max_open = 2 if scheme == "shplonk" else 2 + len(cs.advice_queries) + len(cs.fixed_queries)
        assert sizes["bound_evm"] == sizes["evm"] + 64 * (max_open - tail) and sizes["bound_blake2b"] == sizes["blake2b"] + 32 * (max_open - tail)
        # the point families in transcript order: the shuffle products between the lookup products and the random polynomial
        fam = [(f, int(a), int(c)) for f, a, c in (t.split(":") for t in g["points"])]
        evf = [(f, int(a), int(c)) for f, a, c in (t.split(":") for t in g["evals"])]
        if NS:
            sp, se = (t.split(":") for t in g["shuffles"])
            fam.insert(4, ("sz", int(sp[1]), int(sp[2])))
            evf.insert(6, ("sz", int(se[1]), int(se[2])))
        else:
            assert "shuffles" not in g
            fam.insert(4, ("sz", fam[4][1], 0))
            evf.insert(6, ("sz", evf[6][1], 0))
        assert [(f, c) for f, _, c in fam] == [("adv", A), ("perm", 2 * NL), ("pz", S), ("lz", NL), ("sz", NS), ("rand", 1),
                                               ("hp", cs.degree() - 1), ("open", tail)]
        assert [a for _, a, _ in fam] == [sum(c for _, _, c in fam[:i]) for i in range(len(fam))]
        assert [f for f, _, _ in evf] == ["adv", "fix", "rand", "sig", "pz", "lk", "sz", "h"]
        assert [a for _, a, _ in evf] == [sum(c for _, _, c in evf[:i]) for i in range(len(evf))]
        assert evf[6][1:] == (ev_sh, 2 * NS) and evf[7][1] == ev_h
        before = points - tail
        assert [int(v) for v in g["items"]] == list(range(before)) + [before + scalars + i for i in range(tail)]
    sets = [plh.ints(t) for t in got["gwc"]["sets"]]
    assert sets == [[i for i, q in enumerate(qs) if q[0] == rot] for rot in rotations]
    ref_sets, T = proof_ref.intermediate_sets(qs)
    g = got["shplonk"]
    coms = []
    for tok in g["coms"]:
        p, s, place, q = tok.split("/")
        coms.append((plh.poly_of(p), int(s), int(place), plh.ints(q)))
    got_sets = [(plh.ints(t.split("/")[0]), plh.ints(t.split("/")[1])) for t in g["sets"]]
    assert [c[0] for c in coms] == list(dict.fromkeys(p for _, p in qs))
    assert [[coms[c][0] for c in cs_] for _, cs_ in got_sets] == [keys for _, keys in ref_sets]
    assert [set(rotations[p] for p in pts) for pts, _ in got_sets] == [set(pts) for pts, _ in ref_sets]
    assert T == rotations and int(g["T"][0]) == len(T) and int(g["T"][2]) == sum(len(pts) for pts, _ in ref_sets)
    for ci, (p, s, place, q) in enumerate(coms):
        assert got_sets[s][1][place] == ci
        assert [qs[i] for i in q] == [(rotations[pt], p) for pt in got_sets[s][0]]
    if NS:  # every shuffle product is opened at x and wx, and stands in a set with exactly those points
        for j in range(NS):
            (s,) = [c[1] for c in coms if c[0] == ("sz", 0, j)]
            assert sorted(rotations[p] for p in got_sets[s][0]) == [0, 1]


def check(exe, tmp_path):
    cases = []
    for ns in (0, 1, 3):
        for name, cs in plh.shapes().items():
            cases.append((with_shuffles(cs, ns), 1))
    # (a circuit whose ONLY queries at wx are the shuffles': the point appears with them)
    cases.append((with_shuffles(plh.Shape(5, 2, [(0, 0), (1, 0)]), 2), 1))
    for (cs, _), got in zip(cases, parse(run(exe, tmp_path, cases), len(cases))):
        check_case(cs, got)


def test_layout_with_shuffles_meets_the_reference(tmp_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    check(EXE, tmp_path)


def test_without_shuffles_the_layout_is_what_it_was(tmp_path):
    """NS = 0: the new probe prints what the existing probe prints for the same shape, N = 1, 2, 3"""
    assert os.path.exists(EXE) and os.path.exists(OLD_EXE), "run __graft_entry__.build() first"
    cases = [(with_shuffles(cs, 0), N) for cs in plh.shapes().values() for N in (1, 2, 3)]
    assert run(EXE, tmp_path, cases) == run(OLD_EXE, tmp_path, cases, plh.script_line)


def test_layout_probe_under_the_sanitizers(tmp_path):
    """a second build of the probe under UBSan and ASan (a stand-alone host program: nothing preloaded, nothing loaded into
    Python); the first finding ends it"""
    exe = str(tmp_path / "shuffle_layout_probe_san")
    subprocess.run(["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
                    "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe], check=True)
    check(exe, tmp_path)


def test_header_declares_and_library_exports_the_new_entries(zg):
    names = header_functions()
    lib = zg.load()
    for name in NEW_ENTRIES:
        assert name in names and name in zg.ABI_SYMBOLS and hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "zg_halo2.h")).read()
    assert "ZG_MAX_SHUFFLES = 16" in text and "} zg_shuffle;" in text


def test_zg_shuffle_matches_its_ctypes_mirror_and_zg_lookup(zg, tmp_path):
    exe = str(tmp_path / "shuffle_layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi", "shuffle_layout.c"), "-o", exe], check=True)
    c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert ctypes.sizeof(zg.Shuffle) == c["size"] == c["lookup_size"]
    for field, off in c["fields"].items():
        assert getattr(zg.Shuffle, field).offset == off, field
    assert [f[0] for f in zg.Shuffle._fields_] == list(c["fields"])
    assert c["fields"]["shuffles"] == c["lookup_tables"]
    assert (zg.MAX_SHUFFLES, zg.MAX_LOOKUP_WIDTH) == (c["max_shuffles"], c["max_width"])
    arr, count = zg.shuffle_array([([(3, 2)], [(5, 1)]), ([(0, 1), (1, 1)], [(2, 1), (9, 4)])])
    assert count == 2 and arr[0].width == 1 and (arr[0].shuffles[0].first, arr[0].shuffles[0].count) == (5, 1)
    assert arr[1].width == 2 and (arr[1].inputs[1].first, arr[1].shuffles[1].count) == (1, 4)


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("make", [lambda: toy_circuit(5), lambda: variant_circuit("wide_lookup")], ids=["toy", "wide_lookup"])
def test_reference_without_shuffles_is_phases_ref_and_the_oracle(orc, make):
    cs, asg, ilen = make()
    img = cs.to_c()
    params = orc.params_new(cs.k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x1234567)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    pk = orc.ProvingKey(img, fixed, sigma, params, vk_repr)
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    st, proof, _ = orc.create_proof(pk, adv, inst, 7)
    assert st == 0
    vk = proof_ref.Vk(cs, params, fixed, sigma, vk_repr)
    late = bytearray(proof)
    late[-70] ^= 1
    for i, prf in enumerate((proof, bytes(late), proof[:-1], proof + b"\0")):
        want = orc.verify_proof_pairing(pk, inst, prf)
        got = proof_ref.verify(vk, [inst], prf)
        assert got.verdict == (1 if want == 1 else 0 if want == 0 else -1), i


# ---------------------------------------------------------------------------------------------- the circuits themselves
@pytest.mark.parametrize("name", sorted(shuffle_circuits.SMALL))
def test_circuits_state_shuffles_and_the_bad_witness_is_none(name):
    pc = shuffle_circuits.SMALL[name]()
    cs = pc.cs
    ch = [12345] * len(pc.challenge_phase)
    img = cs.to_c()
    assert img.c.n_lookups == len(cs.lookups) and img.c.cs_degree == cs.degree() >= cs.shuffle_degree()
    assert len(img.shuffles) == len(cs.shuffles) and all(f + c <= img.c.n_monomials for ins, shs in img.shuffles for f, c in ins + shs)
    for variant, holds in ((0, True), (1, True), (shuffle_circuits.BAD, False)):
        cols = {}
        for ph in range(pc.n_phases):
            cols.update(pc.witness(ph, ch, variant))
        at = shuffle_circuits.cell_at(pc, cols, ch)
        ends = [proof_ref.shuffle_product(cs, j, at, 0x1234, 0x5678)[pc.usable] for j in range(len(cs.shuffles))]
        assert all(e == 1 for e in ends) == holds, (variant, ends)


def test_the_circuits_are_what_they_are_here_for():
    s = {name: make() for name, make in shuffle_circuits.SMALL.items()}
    assert len(s["wide"].cs.shuffles[0][0]) == 4 and s["wide"].cs.degree() == s["wide"].cs.shuffle_degree() == 4
    t = s["three"].cs
    assert (len(t.shuffles), len(t.lookups), len(t.perm_columns)) == (3, 2, 2)
    o = s["only"].cs
    assert o.shuffles and not (o.gates or o.lookups or o.perm_columns or o.n_fixed)
    assert sorted(r for _, r in s["rotated"].cs.advice_queries) == [-1, 1, 1]
    assert s["with_challenge"].challenge_phase == [0] and s["with_challenge_phased"].advice_phase == [0, 0, 1, 1]
    assert shuffle_circuits.wide(14, high_gate=True).cs.degree() == 6
