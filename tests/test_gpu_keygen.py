"""keygen on the device: the coset generator as a parameter (zg_ctx_set_coset_generator), sigma from the permutation
mapping (zg_permutation_sigma) and the export of what keygen_pk derives (zg_prover_export_key).

Everything is integer arithmetic, so every comparison is exact equality.  Under the default generator (root 0) the
oracle is the reference; it knows no other generator, so under root 1 the reference is Python-integer Horner evaluation
at zeta' * omega_ext^i -- and, for proofs, the oracle's bytes again, because the quotient h does not depend on the coset
it was interpolated from.  The session's shared context is never touched: a generator is only ever set on a context the
test made itself."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the first HIP call of the process)

from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
RINV = pow(1 << 256, -1, R)
DELTA = pow(7, 1 << 28, R)


def ints(a):
    """Montgomery limbs uint64[m, 4] -> canonical Python integers"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    return [(int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192) * RINV % R for x in a]


def omega_int(zg, log_n):
    return zg.fr_to_int(zg.domain_omega(log_n)[0])


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def on_coset(zg, coeff_arr, g, ext_k, points=None):
    """the polynomial with these coefficients at g * omega_ext^i, for every i (or the listed ones)"""
    w = omega_int(zg, ext_k)
    cs = ints(coeff_arr)
    idx = range(1 << ext_k) if points is None else points
    return [horner(cs, g * pow(w, i, R) % R) for i in idx]


@pytest.fixture()
def roots(zg):
    return zg.fr_cube_root(0), zg.fr_cube_root(1)


@pytest.fixture()
def ctx1(zg, roots):
    """a context of the test's own, under root 1"""
    c = zg.Ctx(0)
    c.set_coset_generator(roots[1])
    yield c
    c.close()


class Keys:
    def __init__(self, orc, zg, ctx, circuit, seed=0xABCDEF):
        self.cs, self.asg, self.ilen = circuit
        self.k = self.cs.k
        self.img = self.cs.to_c()
        self.params = orc.params_new(self.k, seed)
        self.vk_repr = orc.fr_from_int(0x1234567)
        self.fixed, self.sigma = self.asg.fixed_values(), self.asg.sigma_values()
        self.pk = orc.ProvingKey(self.img, self.fixed, self.sigma, self.params, self.vk_repr)
        self.prover = zg.Prover(ctx, self.img, self.fixed, self.sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr)
        self.adv, self.inst = self.asg.advice_values(), self.asg.instance_values(self.ilen)

    def want(self, orc, seed, adv=None):
        st, proof, _ = orc.create_proof(self.pk, self.adv if adv is None else adv, self.inst, seed)
        assert st == 0
        return proof


CIRCUITS_K5 = {"toy": lambda: toy_circuit(5), "toy degree 6": lambda: toy_circuit(5, force_degree=6),
               "gates_only": lambda: variant_circuit("gates_only")}


# ------------------------------------------------------------------ 1. sigma from the mapping
@pytest.mark.parametrize("make", [lambda: toy_circuit(5), lambda: toy_circuit(6), lambda: variant_circuit("no_lookup", k=5)],
                         ids=["toy k5", "toy k6", "no_lookup k5"])
def test_sigma_is_the_inverse_of_the_mapping(ctx, zg, make):
    cs, asg, _ = make()
    sigma = asg.sigma_values()
    assert sigma.shape[0] >= 2
    next_col, next_row = zg.permutation_mapping(sigma, cs.k)
    assert (next_col != np.arange(sigma.shape[0], dtype=np.uint32)[:, None]).any()  # (cycles do cross columns)
    assert np.array_equal(zg.permutation_sigma(ctx, next_col, next_row, cs.k), sigma)


@pytest.mark.parametrize("n_perm", [1, 8])
def test_sigma_of_the_identity_mapping_is_delta_c_omega_r(ctx, zg, n_perm):
    k, n = 4, 16
    col = np.repeat(np.arange(n_perm, dtype=np.uint32)[:, None], n, axis=1)
    row = np.repeat(np.arange(n, dtype=np.uint32)[None, :], n_perm, axis=0)
    got = zg.permutation_sigma(ctx, col, row, k)
    w = omega_int(zg, k)
    want = [pow(DELTA, c, R) * pow(w, r, R) % R for c in range(n_perm) for r in range(n)]
    assert ints(got) == want
    # ... and a mapping that is no identity, cell by cell
    rng = np.random.default_rng(5)
    col2 = rng.integers(0, n_perm, size=col.shape, dtype=np.uint32)
    row2 = rng.integers(0, n, size=row.shape, dtype=np.uint32)
    got = zg.permutation_sigma(ctx, col2, row2, k)
    assert ints(got) == [pow(DELTA, int(c), R) * pow(w, int(r), R) % R for c, r in zip(col2.ravel(), row2.ravel())]
    back = zg.permutation_mapping(got, k)
    assert np.array_equal(back[0], col2) and np.array_equal(back[1], row2)


def test_sigma_refuses_indices_out_of_range(ctx, zg):
    k, n, n_perm = 4, 16, 3
    col = np.repeat(np.arange(n_perm, dtype=np.uint32)[:, None], n, axis=1)
    row = np.repeat(np.arange(n, dtype=np.uint32)[None, :], n_perm, axis=0)
    for arr, cell, bad in ((row, (1, 5), n), (row, (2, 15), 0xFFFFFFFF), (col, (0, 0), n_perm), (col, (2, 7), 1 << 31)):
        keep = arr[cell]
        arr[cell] = bad
        with pytest.raises(zg.ZgError) as e:
            zg.permutation_sigma(ctx, col, row, k)
        assert e.value.status == -1
        arr[cell] = keep
    assert zg.permutation_sigma(ctx, col, row, k).shape == (n_perm, n, 4)  # (the arrays are whole again, and accepted)


# ------------------------------------------------------------------ 2. the transforms under each root
@pytest.mark.parametrize("k,ext_k", [(4, 4), (4, 5), (4, 6), (4, 7), (10, 12)])
def test_transforms_under_each_root(zg, orc, roots, k, ext_k):
    n, en = 1 << k, 1 << ext_k
    coeffs = orc.fill_fr(100 + ext_k, n)
    points = None if k == 4 else sorted(int(i) for i in np.random.default_rng(7).choice(en, size=64, replace=False))
    d = orc.domain((1 << (ext_k - k)) + 1, k)
    assert (d.k, d.extended_k) == (k, ext_k)
    c = zg.Ctx(0)
    try:
        for which in (0, 1):
            c.set_coset_generator(roots[which])
            g = zg.fr_to_int(roots[which])
            want = on_coset(zg, coeffs, g, ext_k, points)
            for nine in (0, 1):  # both limb forms of the butterflies
                zg.tuning_set("ZG_NTT9", nine)
                ext = c.coeff_to_extended(coeffs, k, ext_k)
                got = ints(ext)
                assert (got if points is None else [got[i] for i in points]) == want, (which, nine)
                assert np.array_equal(c.extended_to_coeff(ext, k, ext_k, n), coeffs), (which, nine)
                if which == 0:
                    assert np.array_equal(ext, orc.coeff_to_extended(d, coeffs)), nine
                else:
                    assert not np.array_equal(ext, orc.coeff_to_extended(d, coeffs))
    finally:
        zg.tuning_set("ZG_NTT9", -1)
        c.close()


# ------------------------------------------------------------------ 3. / 4. export
def key_families(zg, prover, F, P):
    fams = {"fixed_polys": [prover.export_key(zg.KEY_FIXED_POLY, c) for c in range(F)],
            "sigma_polys": [prover.export_key(zg.KEY_SIGMA_POLY, c) for c in range(P)],
            "fixed_cosets": [prover.export_key(zg.KEY_FIXED_COSET, c) for c in range(F)],
            "sigma_cosets": [prover.export_key(zg.KEY_SIGMA_COSET, c) for c in range(P)],
            "l0": [prover.export_key(zg.KEY_L0)], "l_last": [prover.export_key(zg.KEY_L_LAST)],
            "l_active_row": [prover.export_key(zg.KEY_L_ACTIVE_ROW)]}
    for family, limit in ((zg.KEY_FIXED_POLY, F), (zg.KEY_FIXED_COSET, F), (zg.KEY_SIGMA_POLY, P), (zg.KEY_SIGMA_COSET, P),
                          (zg.KEY_L0, 1), (zg.KEY_L_LAST, 1), (zg.KEY_L_ACTIVE_ROW, 1), (7, 0)):
        with pytest.raises(zg.ZgError) as e:
            prover.export_key(family, limit)
        assert e.value.status == -1
    return fams


def l_coefficients(orc, cs, d):
    """coefficient forms of l_0, l_last and l_active_row: the unit vectors at rows 0 and n - bf - 1, and 1 - l_last - the sum
    of the unit vectors of the blinding rows (= the indicator of the rows below n - bf - 1: the transforms are linear and
    exact, so this is the same array)"""
    n, last = 1 << cs.k, (1 << cs.k) - cs.blinding_factors() - 1
    one = orc.fr_from_int(1)
    e0, el, act = (np.zeros((n, 4), np.uint64) for _ in range(3))
    e0[0], el[last], act[:last] = one, one, one
    return [orc.lagrange_to_coeff(d, v) for v in (e0, el, act)]


@pytest.mark.parametrize("name", ["toy k5", "toy k7 degree 6", "gates_only"])
def test_export_matches_the_oracle_under_root_0(ctx, zg, orc, roots, name):
    circuit = {"toy k5": lambda: toy_circuit(5), "toy k7 degree 6": lambda: toy_circuit(7, force_degree=6),
               "gates_only": lambda: variant_circuit("gates_only")}[name]()
    assert np.array_equal(ctx.coset_generator(), roots[0])
    s = Keys(orc, zg, ctx, circuit)
    cs = s.cs
    F, P = s.fixed.shape[0], s.sigma.shape[0]
    assert (P == 0) == (name == "gates_only")
    d = orc.domain(cs.degree(), cs.k)
    want = {"fixed_polys": [orc.lagrange_to_coeff(d, v) for v in s.fixed], "sigma_polys": [orc.lagrange_to_coeff(d, v) for v in s.sigma]}
    want["fixed_cosets"] = [orc.coeff_to_extended(d, p) for p in want["fixed_polys"]]
    want["sigma_cosets"] = [orc.coeff_to_extended(d, p) for p in want["sigma_polys"]]
    l0, l_last, l_active = l_coefficients(orc, cs, d)
    want["l0"], want["l_last"], want["l_active_row"] = ([orc.coeff_to_extended(d, p)] for p in (l0, l_last, l_active))
    # l_active_row = 1 - l_last - sum of the blinding rows' polynomials, on the coset too
    n, bf = 1 << cs.k, cs.blinding_factors()
    blind = np.zeros((n, 4), np.uint64)
    blind[n - bf:] = orc.fr_from_int(1)
    blind_ext = ints(orc.coeff_to_extended(d, orc.lagrange_to_coeff(d, blind)))
    assert ints(want["l_active_row"][0]) == [(1 - a - b) % R for a, b in zip(ints(want["l_last"][0]), blind_ext)]

    def check(prover, where):
        got = key_families(zg, prover, F, P)
        for fam, arrays in want.items():
            assert len(got[fam]) == len(arrays), (where, fam)
            for c, (g, w) in enumerate(zip(got[fam], arrays)):
                assert np.array_equal(g, w), (where, fam, c)

    ctx2 = zg.Ctx(0)
    try:
        for overlap in (True, False):  # once in each scheduling form, a proof on either side of the export
            s.prover.set_overlap(overlap)
            assert s.prover.prove(s.adv, s.inst, 3) == s.want(orc, 3)
            check(s.prover, "latency form" if overlap else "throughput form")
            assert s.prover.prove(s.adv, s.inst, 4) == s.want(orc, 4)
        child = s.prover.fork(ctx2)
        check(child, "fork")
        assert child.prove(s.adv, s.inst, 5) == s.want(orc, 5)
        child.close()
    finally:
        ctx2.close()
        s.prover.close()


@pytest.mark.parametrize("name", list(CIRCUITS_K5))
def test_export_under_root_1_is_horner_on_the_other_coset(ctx, ctx1, zg, orc, roots, name):
    circuit = CIRCUITS_K5[name]()
    s0, s1 = Keys(orc, zg, ctx, circuit), Keys(orc, zg, ctx1, circuit)
    cs = s0.cs
    F, P = s0.fixed.shape[0], s0.sigma.shape[0]
    ext_k, g1 = cs.extended_k(), zg.fr_to_int(roots[1])
    assert np.array_equal(s0.prover.coset_generator(), roots[0]) and np.array_equal(s1.prover.coset_generator(), roots[1])
    d = orc.domain(cs.degree(), cs.k)
    coeff_of = {"fixed_cosets": [orc.lagrange_to_coeff(d, v) for v in s0.fixed], "sigma_cosets": [orc.lagrange_to_coeff(d, v) for v in s0.sigma]}
    coeff_of["l0"], coeff_of["l_last"], coeff_of["l_active_row"] = ([p] for p in l_coefficients(orc, cs, d))
    for overlap in (True, False):
        s1.prover.set_overlap(overlap)
        got0, got1 = key_families(zg, s0.prover, F, P), key_families(zg, s1.prover, F, P)
        for fam in ("fixed_polys", "sigma_polys"):  # the coefficient forms know no coset
            src = coeff_of[fam.replace("polys", "cosets")]
            assert len(got1[fam]) == len(src)
            for a, b, w in zip(got0[fam], got1[fam], src):
                assert np.array_equal(a, b) and np.array_equal(b, w), fam
        for fam, polys in coeff_of.items():
            assert len(got1[fam]) == len(polys), fam
            for c, (g, p) in enumerate(zip(got1[fam], polys)):
                assert ints(g) == on_coset(zg, p, g1, ext_k), (fam, c)
                assert not np.array_equal(g, got0[fam][c]), (fam, c)
    s0.prover.close()
    s1.prover.close()


# ------------------------------------------------------------------ 5. proofs do not depend on the root
PROOF_CIRCUITS = {"toy k6": lambda: toy_circuit(6), "toy k7 degree 6": lambda: toy_circuit(7, force_degree=6),
                  "no_lookup": lambda: variant_circuit("no_lookup"), "gates_only": lambda: variant_circuit("gates_only"),
                  "wide_lookup": lambda: variant_circuit("wide_lookup")}


@pytest.mark.parametrize("name", list(PROOF_CIRCUITS))
def test_proofs_under_root_1_are_the_oracles_bytes(ctx1, zg, orc, roots, name):
    s = Keys(orc, zg, ctx1, PROOF_CIRCUITS[name]())
    assert np.array_equal(s.prover.coset_generator(), roots[1])
    want = {seed: s.want(orc, seed) for seed in (1, 2, 3)}
    try:
        for overlap in (True, False):
            s.prover.set_overlap(overlap)
            s.prover.set_batch(1)
            assert s.prover.prove(s.adv, s.inst, 1) == want[1], overlap
            s.prover.set_batch(3)
            got, sts = s.prover.prove_batch([s.adv] * 3, [s.inst] * 3, [1, 2, 3])
            assert sts == [0, 0, 0] and got == [want[1], want[2], want[3]], overlap
        # a repeated lone proof behind the gate
        s.prover.set_batch(1)
        s.prover.set_overlap(True)
        zg.tuning_set("ZG_LAT_GATE", 1)
        before = s.prover.gate_stats()
        for seed in (1, 2, 3):
            assert s.prover.prove(s.adv, s.inst, seed) == want[seed]
        after = s.prover.gate_stats()
        assert after["gated_proofs"] - before["gated_proofs"] == 2 and after["remade_plain"] == before["remade_plain"]
    finally:
        zg.tuning_set("ZG_LAT_GATE", -1)
        s.prover.close()


def test_tiny_model_under_root_1_is_the_oracles_bytes(ctx1, zg, orc):
    import witness_tape
    import wnn_circuit
    import wnn_model

    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    wnn = wnn_model.load_checked_in(name)
    image = wnn_model.load_test_image()
    cs, asg, ilen, _ = wnn_circuit.build(wnn, image, k)
    img = cs.to_c()
    params = orc.params_new(k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    prover = zg.Prover(ctx1, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr)
    plan = zg.WitnessPlan(ctx1, witness_tape.trace(wnn, k).arrays())
    proofs, _, sts = prover.prove_images(plan, image[None], [7])
    pk = orc.ProvingKey(img, fixed, sigma, params, vk_repr)
    st, want, _ = orc.create_proof(pk, asg.advice_values(), asg.instance_values(ilen), 7)
    assert st == 0 and sts == [0] and proofs[0] == want
    plan.close()
    prover.close()


def test_unsatisfied_statements_under_root_1_are_deterministic_and_rejected(ctx1, zg, orc):
    """Outside the claim above: in the latency form the unverifiable bytes of an unsatisfied statement are cut from a coset
    interpolant, so they may differ by root.  What holds: the same bytes every time, and no verifier accepts them."""
    s = Keys(orc, zg, ctx1, toy_circuit(6))
    unsat = s.adv.copy()
    unsat[2, 3] = orc.fr_from_int(99)  # (a gate fails; no lookup does, so a proof is made)
    for overlap in (True, False):
        s.prover.set_overlap(overlap)
        first = s.prover.prove(unsat, s.inst, 1)
        assert s.prover.prove(unsat, s.inst, 1) == first and len(first) == len(s.want(orc, 1))
        assert orc.verify_proof_pairing(s.pk, s.inst, first) != 1
    s.prover.close()


# ------------------------------------------------------------------ 6. stand-alone evaluate_h under root 1
@pytest.mark.parametrize("k,force_degree", [(6, None), (7, 6)])
def test_stand_alone_evaluate_h_under_root_1(ctx1, zg, orc, k, force_degree):
    s = Keys(orc, zg, ctx1, toy_circuit(k, force_degree=force_degree))
    cs, adv, inst, ilen = s.cs, s.adv, s.inst, s.ilen
    seed = 21
    st, _, tr = orc.create_proof(s.pk, adv, inst, seed, want_trace=True)
    assert st == 0
    n, en = 1 << k, 1 << cs.extended_k()
    bf = cs.blinding_factors()
    usable = n - (bf + 1)
    blinded = adv.copy()
    for c in range(cs.n_advice):  # create_proof's advice blinding: tag 1, index = column * (bf + 1) + j
        for j in range(bf + 1):
            blinded[c, usable + j] = orc.rand_fr(seed, 1, c * (bf + 1) + j)
    inst_cols = np.zeros((cs.n_instance, n, 4), np.uint64)
    inst_cols[:, :ilen] = inst
    d = orc.domain(cs.degree(), k)
    nl, sets = len(cs.lookups), tr.n_sets
    pin = tr.array("permuted_input", nl * n).reshape(nl, n, 4)
    ptab = tr.array("permuted_table", nl * n).reshape(nl, n, 4)
    permuted = np.stack([x for l in range(nl) for x in (pin[l], ptab[l])]) if nl else np.zeros((0, n, 4), np.uint64)

    def coeffs(cols):
        return np.stack([orc.lagrange_to_coeff(d, c) for c in cols]) if len(cols) else np.zeros((0, n, 4), np.uint64)

    got = s.prover.evaluate_h(coeffs(blinded), coeffs(inst_cols), coeffs(tr.array("perm_z", sets * n).reshape(sets, n, 4)),
                              coeffs(tr.array("lookup_z", nl * n).reshape(nl, n, 4)), coeffs(permuted), tr.fe("theta"),
                              tr.fe("beta"), tr.fe("gamma"), tr.fe("y"), en)
    qpd = cs.degree() - 1
    assert not np.array_equal(got, tr.array("h_ext", en))  # (the oracle's h sits on the other coset)
    assert np.array_equal(ctx1.extended_to_coeff(got, k, cs.extended_k(), qpd * n), tr.array("h_pieces", qpd * n))
    orc.trace_free(tr)
    assert s.prover.prove(adv, inst, 5) == s.want(orc, 5)
    s.prover.close()


# ------------------------------------------------------------------ 7. state rules
def test_generator_state_rules(ctx, zg, orc, roots):
    c1, c2 = zg.Ctx(0), zg.Ctx(0)
    try:
        assert np.array_equal(c1.coset_generator(), roots[0])  # (the default)
        c1.set_coset_generator(roots[1])
        # what is no primitive cube root of unity is refused and changes nothing
        r_limbs = zg.int_to_limbs(zg.limbs_to_int(roots[1]) + R)  # (root 1 + r: the same residue, not canonical)
        assert zg.limbs_to_int(r_limbs) < 1 << 256
        for bad in (np.zeros(4, np.uint64), zg.fr_from_int(1), zg.fr_from_int(7), zg.int_to_limbs(zg.fr_to_int(roots[1])), r_limbs,
                    zg.fr_from_int(R - 1)):
            with pytest.raises(zg.ZgError) as e:
                c1.set_coset_generator(bad)
            assert e.value.status == -1
            assert np.array_equal(c1.coset_generator(), roots[1])
        s = Keys(orc, zg, c1, toy_circuit(6))
        child = s.prover.fork(c2)  # (c2 is under root 0)
        assert np.array_equal(c2.coset_generator(), roots[0])
        c1.set_coset_generator(roots[0])
        c2.set_coset_generator(roots[0])
        late = Keys(orc, zg, c1, toy_circuit(6))  # a prover made now takes the context's new root
        assert np.array_equal(late.prover.coset_generator(), roots[0])
        want = s.want(orc, 1)
        l0_root1 = on_coset(zg, l_coefficients(orc, s.cs, orc.domain(s.cs.degree(), s.k))[0], zg.fr_to_int(roots[1]), s.cs.extended_k())
        for p in (s.prover, child):
            assert np.array_equal(p.coset_generator(), roots[1])
            assert ints(p.export_key(zg.KEY_L0)) == l0_root1
            assert p.prove(s.adv, s.inst, 1) == want
        # the witness check and the verifier take the root-1 prover's word
        assert s.prover.check_batch([s.adv], [s.inst]) == [([0, 0, 0], [])]
        fc, sc = s.prover.vk_commitments()
        fc0, sc0 = late.prover.vk_commitments()
        assert np.array_equal(fc, fc0) and np.array_equal(sc, sc0)  # (commitments are over the Lagrange basis: no coset)
        verifier = zg.Verifier(ctx, s.img, fc, sc, s.params.g_np()[0], np.array(s.params.g2, np.uint64), np.array(s.params.s_g2, np.uint64),
                               s.vk_repr)
        proofs = [s.prover.prove(s.adv, s.inst, 2), child.prove(s.adv, s.inst, 3)]
        assert verifier.verify(proofs, [s.inst] * 2, 11) == [1, 1]
        verifier.close()
        for p in (child, s.prover, late.prover):
            p.close()
    finally:
        c2.close()
        c1.close()


# ------------------------------------------------------------------ 8. the key file
def test_key_file_from_the_device(tmp_path, ctx, zg, orc):
    import formats

    cs, asg, ilen = toy_circuit(6)
    k, n, en = cs.k, 1 << cs.k, 1 << cs.extended_k()
    fixed = asg.fixed_values()
    sigma = zg.permutation_sigma(ctx, *zg.permutation_mapping(asg.sigma_values(), k), k)  # sigma from the mapping, on the device
    assert np.array_equal(sigma, asg.sigma_values())
    F, P = fixed.shape[0], sigma.shape[0]
    img = cs.to_c()
    params = orc.params_new(k, 0x5EED)
    vk_repr = orc.fr_from_int(0xC0FFEE)
    prover = zg.Prover(ctx, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr)
    fc, sc = prover.vk_commitments()
    fam = lambda family, count: np.stack([prover.export_key(family, c) for c in range(count)])
    written = formats.ProvingKeyFile(
        k, fixed_commitments=fc, permutation_commitments=sc, selectors=np.zeros((0, n), bool), l0=prover.export_key(zg.KEY_L0),
        l_last=prover.export_key(zg.KEY_L_LAST), l_active_row=prover.export_key(zg.KEY_L_ACTIVE_ROW), fixed_values=fixed,
        fixed_polys=fam(zg.KEY_FIXED_POLY, F), fixed_cosets=fam(zg.KEY_FIXED_COSET, F), permutations=sigma,
        permutation_polys=fam(zg.KEY_SIGMA_POLY, P), permutation_cosets=fam(zg.KEY_SIGMA_COSET, P))
    path = str(tmp_path / "pk.bin")
    formats.write_pk(path, written)
    back = formats.read_pk(path, 0, P)
    assert back.k == k
    for f in formats.ProvingKeyFile.FIELDS:
        a, b = np.asarray(getattr(written, f)), np.asarray(getattr(back, f))
        assert a.shape == b.shape and np.array_equal(a, b), f
        if f not in ("selectors",):
            assert a.size and a.any(), f  # (no placeholder is left)
    assert back.l0.shape == (en, 4) and back.fixed_cosets.shape == (F, en, 4) and back.permutation_polys.shape == (P, n, 4)
    verifier = zg.Verifier(ctx, img, np.array(back.fixed_commitments), np.array(back.permutation_commitments), params.g_np()[0],
                           np.array(params.g2, np.uint64), np.array(params.s_g2, np.uint64), vk_repr)
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    proof = prover.prove(adv, inst, 9)
    assert verifier.verify([proof], [inst], 4) == [1]
    verifier.close()
    prover.close()
