"""Advice phases and challenges, the host side: tests/proof_ref.py (the Python-integer verify_proof, here its phases) held
against the oracle's pairing verifier where both apply; csrc/proof_layout.h's phase order, boundaries, challenge lists
and point_index against the order proof_ref walks, through tests/abi/phases_layout_probe (a stand-alone host program,
built once more under the sanitizers); and the test circuits of tests/phases_circuits.py against a mock check.  No device."""
import os
import random
import subprocess

import numpy as np
import pytest

import phases_circuits
import proof_ref
from circuit import ADVICE, FIXED, INSTANCE, R
from circuits import toy_circuit, variant_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "abi", "phases_layout_probe")
SRC = os.path.join(ROOT, "tests", "abi", "phases_layout_probe.cpp")


# ---------------------------------------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("make", [lambda: toy_circuit(5), lambda: variant_circuit("no_lookup"), lambda: variant_circuit("wide_lookup")],
                         ids=["toy", "no_lookup", "wide_lookup"])
def test_reference_gives_the_oracles_verdicts_on_one_phase_circuits(orc, make):
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
    wrong = inst.copy()
    wrong[0, 0] = orc.fr_from_int(5)
    tampered = bytearray(proof)
    tampered[64 * cs.n_advice + 5] ^= 1  # (inside a commitment behind the advice: most likely off the curve)
    late = bytearray(proof)
    late[-70] ^= 1                       # (an evaluation or a W)
    cases = [(inst, proof), (wrong, proof), (inst, bytes(tampered)), (inst, bytes(late)), (inst, proof[:-1]), (inst, proof[:200]),
             (inst, proof + b"\0")]
    for i, (ins, prf) in enumerate(cases):
        want = orc.verify_proof_pairing(pk, ins, prf)
        got = proof_ref.verify(vk, [ins], prf)
        assert got.verdict == (1 if want == 1 else 0 if want == 0 else -1), (i, want, got.verdict)
    ok = proof_ref.verify(vk, [inst], proof)
    assert ok.verdict == 1 and ok.challenges == {} and ok.order == [(0, 0, c) for c in range(cs.n_advice)]
    assert len(proof) == proof_ref.proof_len(cs)


# ---------------------------------------------------------------------------------------------- the test circuits themselves
@pytest.mark.parametrize("name", sorted(phases_circuits.SMALL))
def test_circuits_are_satisfied_for_any_challenges(name):
    """gates vanish on the usable rows and every lookup input is in its table, for two sets of challenge values and two
    witness variants; the copies hold"""
    pc = phases_circuits.SMALL[name]()
    cs, n, usable = pc.cs, pc.n, pc.usable
    fixed = [[int(v) for v in col] for col in pc.asg.fixed]
    assert len(pc.advice_phase) == cs.n_advice and max(pc.challenge_phase) < pc.n_phases
    for variant, seed in ((0, 1), (1, 2)):
        rng = random.Random(seed)
        ch = [rng.randrange(R) for _ in pc.challenge_phase]
        cols = {}
        for ph in range(pc.n_phases):
            # a phase sees the challenges squeezed behind the phases before it, zero for the others
            seen = [c if pc.challenge_phase[j] < ph else 0 for j, c in enumerate(ch)]
            cols.update(pc.witness(ph, seen, variant))
        inst = pc._instance(variant) if cs.n_instance else []

        def cell_at(row):
            def f(qi):
                kind, c, rot = cs.queries[qi]
                if kind == phases_circuits.CHALLENGE:
                    return ch[c]
                if kind == INSTANCE:
                    col = inst[c] + [0] * n
                    return col[(row + rot) % n]
                return (fixed if kind == FIXED else cols)[c][(row + rot) % n]
            return f

        for row in range(usable):
            for gi, g in enumerate(cs.gates):
                assert g.eval(cell_at(row)) == 0, (name, gi, row)
        for ins, tabs in cs.lookups:
            table = {tuple(t.eval(cell_at(r)) for t in tabs) for r in range(usable)}
            for row in range(usable):
                assert tuple(e.eval(cell_at(row)) for e in ins) in table, (name, row)
        for pcol, (kind, c) in enumerate(cs.perm_columns):
            for row in range(n):
                oc, orow = pc.asg.mapping[pcol][row]
                okind, ocol = cs.perm_columns[oc]
                here = cols[c][row] if kind == ADVICE else (inst[c] + [0] * n)[row]
                there = cols[ocol][orow] if okind == ADVICE else (inst[ocol] + [0] * n)[orow]
                assert here == there, (name, pcol, row)


def test_the_circuits_are_what_the_issue_asks_for():
    c = {name: make() for name, make in phases_circuits.SMALL.items()}
    assert c["rlc"].advice_phase == [0, 0, 1] and c["rlc"].challenge_phase == [0] and c["rlc"].cs.perm_columns
    assert c["shuffle"].advice_phase == [0, 0, 1]
    assert c["interleaved"].advice_phase == [1, 0, 1]
    assert sorted(r for _, r in c["interleaved"].cs.advice_queries) == [-1, 0, 0, 0, 1]
    t = c["three_phase"]
    assert t.advice_phase == [0, 1, 2] and t.challenge_phase == [0, 0, 1, 2]
    ins, tabs = t.cs.lookups[0]
    chal_queries = {i for i, q in enumerate(t.cs.queries) if q[0] == phases_circuits.CHALLENGE}
    assert len(ins) == 2 and any(chal_queries & set(k) for k in ins[1].terms) and any(chal_queries & set(k) for k in tabs[1].terms)
    c3 = t.cs.queries.index((phases_circuits.CHALLENGE, 3, 0))
    assert not any(c3 in k for e in ins + tabs for k in e.terms) and any(c3 in k for g in t.cs.gates for k in g.terms)
    g = c["gates_only_challenge"]
    assert g.n_phases == 1 and not g.cs.lookups and not g.cs.perm_columns and not g.cs.n_instance
    # a challenge has degree 0: the degree is what the circuit without it has
    assert c["rlc"].cs.degree() == 3 and t.cs.degree() == 5 and g.cs.degree() == 3
    # the flattened image carries the challenge as query kind 3
    img = g.cs.to_c()
    assert [(q.kind, q.column, q.rotation) for q in img.c.queries[:img.c.n_queries]].count((3, 0, 0)) == 1


# ---------------------------------------------------------------------------------------------- the layout
def script_line(cs, N, advice_phase, challenge_phase):
    head = [cs.n_advice, cs.n_fixed, len(cs.perm_columns), len(cs.lookups), proof_ref.n_sets(cs), cs.degree() - 1, cs.blinding_factors(), cs.k, N]
    for qs in (cs.advice_queries, cs.fixed_queries):
        head.append(len(qs))
        for col, rot in qs:
            head += [col, rot]
    for ph in (advice_phase, challenge_phase):
        head.append(len(ph))
        head += list(ph)
    return " ".join(str(v) for v in head)


def run(exe, tmp_path, lines):
    script = tmp_path / "phases_script.txt"
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out, cur = [], None
    for line in r.stdout.splitlines():
        tok = line.split()
        if tok[0] == "case":
            cur = {"gwc": {}, "shplonk": {}}
        elif tok[0] == "legal":
            cur["legal"] = " ".join(tok[1:])
        elif tok[0] == "end":
            out.append(cur)
        else:
            cur[tok[0]][tok[1]] = tok[2:]
    assert len(out) == len(lines)
    return out


def check(exe, tmp_path):
    made = {name: make() for name, make in phases_circuits.SMALL.items()}
    cases = [(name, N) for name in sorted(made) for N in (1, 3)]
    lines = [script_line(made[name].cs, N, made[name].advice_phase, made[name].challenge_phase) for name, N in cases]
    # ... and per circuit the all-zero and the empty phase vector, no challenge squeezed
    flat = [(name, N, z) for name in sorted(made) for N in (1, 3) for z in (True, False)]
    lines += [script_line(made[name].cs, N, [0] * made[name].cs.n_advice if z else [], []) for name, N, z in flat]
    got = run(exe, tmp_path, lines)
    for (name, N), g in zip(cases, got):
        pc = made[name]
        cs, A = pc.cs, pc.cs.n_advice
        assert g["legal"] == "yes", (name, g["legal"])
        order = proof_ref.advice_order(cs, N, pc.advice_phase)
        walk = proof_ref.phases_of(cs, pc.advice_phase, pc.challenge_phase)
        for scheme in ("gwc", "shplonk"):
            s = g[scheme]
            # where each (circuit, column) stands: the order the reference reads the commitments in
            index = {tuple(int(v) for v in tok.split("=")[0].split(":")): int(tok.split("=")[1]) for tok in s["advice"]}
            assert sorted(index.values()) == list(range(N * A)), (name, N)
            assert [index[c, col] for _, c, col in order] == list(range(N * A)), (name, N, scheme)
            # the phases: boundaries, columns, challenges
            assert len(s["phases"]) == len(walk)
            end = 0
            for tok, (cols, squeezed) in zip(s["phases"], walk):
                e, c, j = tok.split("/")
                end += N * len(cols)
                assert int(e) == end and [int(v) for v in c.split(",") if v] == cols and [int(v) for v in j.split(",") if v] == squeezed
            assert end == N * A
            # nothing else moves, and the proof is as long as without phases
            sizes = dict(zip(s["sizes"][::2], (int(v) for v in s["sizes"][1::2])))
            sch = proof_ref.SHPLONK if scheme == "shplonk" else proof_ref.GWC
            assert sizes["evm"] == proof_ref.proof_len(cs, N=N, scheme=sch, transcript=proof_ref.EVM)
            assert sizes["blake2b"] == proof_ref.proof_len(cs, N=N, scheme=sch, transcript=proof_ref.BLAKE2B)
    by_case = {}
    for (name, N, z), g in zip(flat, got[len(cases):]):
        by_case[name, N, z] = g
    for (name, N) in cases:
        zero, empty = by_case[name, N, True], by_case[name, N, False]
        assert zero["legal"] == "yes"
        assert zero["gwc"] == empty["gwc"] and zero["shplonk"] == empty["shplonk"], (name, N)  # field for field
        A = made[name].cs.n_advice
        assert [tok.split("=")[1] for tok in empty["gwc"]["advice"]] == [str(v) for v in range(N * A)]
        assert empty["gwc"]["adv_tables"] == ["0", "0", "0"] and len(empty["gwc"]["phases"]) == 1
        phased = got[cases.index((name, N))]
        for key in ("sizes", "families", "others", "queries"):  # only the ADVICE order depends on the phases
            assert phased["gwc"][key] == empty["gwc"][key] and phased["shplonk"][key] == empty["shplonk"][key], (name, N, key)
    # what the set_phases entries refuse
    cs = made["rlc"].cs
    bad = [([0, 0, 3], [0]), ([0, 0, 2], [0]), ([0, 0, 1], [2]), ([0, 0, 1], [0] * 17)]
    refused = run(exe, tmp_path, [script_line(cs, 1, a, c) for a, c in bad])
    assert all(r["legal"] != "yes" for r in refused), [r["legal"] for r in refused]


def test_layout_states_the_phase_order(tmp_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    check(EXE, tmp_path)


def test_layout_probe_under_the_sanitizers(tmp_path):
    """a second build of the probe under UBSan and ASan (a stand-alone host program: nothing preloaded, nothing loaded into
    Python); the first finding ends it"""
    exe = str(tmp_path / "phases_layout_probe_san")
    subprocess.run(["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
                    "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe], check=True)
    check(exe, tmp_path)


def test_interleaved_commitment_order_differs_from_column_order():
    pc = phases_circuits.interleaved()
    assert proof_ref.advice_order(pc.cs, 1, pc.advice_phase) == [(0, 0, 1), (1, 0, 0), (1, 0, 2)]
    assert proof_ref.advice_order(pc.cs, 2, pc.advice_phase) == [(0, 0, 1), (0, 1, 1), (1, 0, 0), (1, 0, 2), (1, 1, 0), (1, 1, 2)]
