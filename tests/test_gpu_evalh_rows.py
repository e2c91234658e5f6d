"""evaluate_h's default kernel row by row: the scaled permutation term (one product per column fewer, the key's sigma slabs
divided by delta^col zeta^a), small integer coefficients without a Montgomery product (f9_mul_small) and the batch's shared
row tiles.  Field arithmetic is exact, so every comparison here is equality: h on the extended coset and the proof bytes
against the oracle, and the default kernel against the unscaled one (ZG_EVALH_GROUPED=0) on inputs that satisfy nothing."""
import random

import numpy as np
import pytest

from circuit import ADVICE, FIXED, R, Assignment, ConstraintSystem
from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu

SMALL_MAX = 1 << 12  # F9_SMALL_MAX of csrc/field9.h: the classifier's bound
BIG = R - (1 << 200) - 12345  # a 254-bit coefficient


def perm_circuit(k, n_cols, gate_degree, seed=5):
    """n_cols advice columns under the permutation argument (chunk = gate_degree - 2 columns per set), one gate of the given
    degree; every column holds the same values, so copies between columns hold on any row."""
    rng = random.Random(seed)
    cs = ConstraintSystem(k)
    q = cs.fixed_column()
    cols = [cs.advice_column() for _ in range(n_cols)]
    out = cs.advice_column()
    for c in cols:
        cs.enable_equality(ADVICE, c)
    e = cs.advice(cols[0])
    for _ in range(gate_degree - 2):
        e = e * cs.advice(cols[-1])
    cs.create_gate([cs.fixed(q) * (e - cs.advice(out))])
    asg = Assignment(cs)
    usable = cs.usable_rows()
    for r in range(usable):
        v = rng.randrange(R)
        asg.set(FIXED, q, r, 1)
        for c in cols:
            asg.set(ADVICE, c, r, v)
        asg.set(ADVICE, out, r, pow(v, gate_degree - 1, R))
    for r in range(0, usable, 3):
        for i in range(n_cols - 1):
            asg.copy((ADVICE, cols[i], r), (ADVICE, cols[i + 1], r))
    if n_cols > 1:
        asg.copy((ADVICE, cols[0], 1), (ADVICE, cols[-1], 1))
    return cs, asg, 0


def coefficient_circuit(k=7, seed=9):
    """Gates whose coefficients sit at the edges of the small-integer classifier -- bound - 1, bound, bound + 1, r - bound,
    r - bound - 1, r - 1, 2, -2, 0 and a 254-bit one -- on cells with full-size values: as the coefficient of a bare cell
    and of a product, behind a common selector, without one, and behind a univariate factor (where the classifier sees the
    coefficient after the division by the factor's common coefficient).  Satisfied: every gate has an output column."""
    rng = random.Random(seed)
    B = SMALL_MAX
    cs = ConstraintSystem(k)
    q, q2 = cs.fixed_column(), cs.fixed_column()
    a0, a1, a2 = cs.advice_column(), cs.advice_column(), cs.advice_column()
    o1, o2, o3, o4, a7 = (cs.advice_column() for _ in range(5))
    A = cs.advice
    lin = ((B - 1) * A(a0) + B * A(a1) + (B + 1) * A(a2) - B * A(a0, 1) - (B + 1) * A(a1, 1) + 2 * A(a2, 1) - 2 * A(a0, -1)
           + BIG * A(a1, -1) - A(o1))
    g1 = cs.fixed(q) * lin
    zero_key = next(key for key in (cs.fixed(q) * A(a2, -1)).terms)
    g1.terms[zero_key] = 0  # (Expr drops zero terms: put one back, the image then holds a monomial with coefficient 0)
    prod = (B * A(a0) * A(a1) - (B + 1) * A(a1) * A(a2) + 509 * A(a0) * A(a2) + BIG * A(a0) * A(a0) - B * A(a2) * A(a2) * A(a0)
            + (B - 1) * A(a1) * A(a1) * A(a2) - A(o2))
    g2 = cs.fixed(q) * prod
    g3 = 3 * cs.fixed(q) * A(a0) * A(a1) - cs.fixed(q) * A(o3) + 256 * cs.fixed(q2) * A(a7) - 2048 * cs.fixed(q2)
    x = A(a0, 1)
    g4 = x * (1 - x) * (2 - x) * cs.fixed(q) * (256 * A(a1) - 512 * A(a2) + 768 * A(o4))
    cs.create_gate([g1, g2, g3, g4])
    asg = Assignment(cs)
    usable = cs.usable_rows()
    val = {c: [rng.randrange(R) for _ in range(usable)] for c in (a0, a1, a2)}
    for c in (a0, a1, a2):
        for r in range(usable):
            asg.set(ADVICE, c, r, val[c][r])
    inv768 = pow(768, R - 2, R)
    for r in range(1, usable - 1):
        asg.set(FIXED, q, r, 1)
        x0, x1, x2 = val[a0][r], val[a1][r], val[a2][r]
        asg.set(ADVICE, o1, r, ((B - 1) * x0 + B * x1 + (B + 1) * x2 - B * val[a0][r + 1] - (B + 1) * val[a1][r + 1]
                                + 2 * val[a2][r + 1] - 2 * val[a0][r - 1] + BIG * val[a1][r - 1]) % R)
        asg.set(ADVICE, o2, r, (B * x0 * x1 - (B + 1) * x1 * x2 + 509 * x0 * x2 + BIG * x0 * x0 - B * x2 * x2 * x0
                                + (B - 1) * x1 * x1 * x2) % R)
        asg.set(ADVICE, o3, r, 3 * x0 * x1 % R)
        asg.set(ADVICE, o4, r, (512 * x2 - 256 * x1) * inv768 % R)
        if r % 2 == 0:
            asg.set(FIXED, q2, r, 1)
            asg.set(ADVICE, a7, r, 8)
        else:
            asg.set(ADVICE, a7, r, rng.randrange(R))
    return cs, asg, 0


def keys(orc, zg, ctx, built, k, **knobs):
    cs, asg, ilen = built
    img = cs.to_c()
    params = orc.params_new(k, 0xABCDEF)
    vk_repr = orc.fr_from_int(0x7654321)
    fixed, sigma = asg.fixed_values(), asg.sigma_values()
    pk = orc.ProvingKey(img, fixed, sigma, params, vk_repr)
    before = {name: zg.tuning_get(name) for name in knobs}
    try:
        for name, v in knobs.items():
            zg.tuning_set(name, v)
        prover = zg.Prover(ctx, img, fixed, sigma, params.g_np(), params.g_lagrange_np(), vk_repr)
    finally:
        for name, v in before.items():
            zg.tuning_set(name, v)
    return cs, asg, ilen, pk, prover, img


def same_h_and_bytes(orc, prover, cs, pk, adv, inst, seeds=(3, 4)):
    """both scheduling forms: the latency form's single coset, then the throughput form (the split domain where it applies)"""
    en = 1 << cs.extended_k()
    for seed, overlap in zip(seeds, (True, False)):
        prover.set_overlap(overlap)
        st, want, tr = orc.create_proof(pk, adv, inst, seed, want_trace=True)
        assert st == 0
        got = prover.prove(adv, inst, seed)
        assert np.array_equal(prover.fetch(0, 0, en), tr.array("h_ext", en)), ("h_ext", overlap)
        assert got == want, ("proof bytes", overlap)
        orc.trace_free(tr)


CIRCUITS = {
    "toy k8 degree 6 (5 columns, sets of 4 + 1)": lambda: (toy_circuit(8, force_degree=6), 8),
    "merged selectors": lambda: (variant_circuit("merged_selectors", k=6), 6),
    "wide lookup": lambda: (variant_circuit("wide_lookup", k=6), 6),
    "no permutation": lambda: (variant_circuit("gates_only", k=6), 6),
    "one set only (3 columns, chunk 3)": lambda: (perm_circuit(6, 3, 5), 6),
    "7 columns, chunk 3": lambda: (perm_circuit(6, 7, 5), 6),
    "17 columns in 9 sets: more than the scaled term holds constants for": lambda: (perm_circuit(6, 17, 4), 6),
    "coefficients at the classifier's edges": lambda: (coefficient_circuit(7), 7),
}


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_h_and_proof_bytes_match_the_oracle(ctx, zg, orc, name):
    built, k = CIRCUITS[name]()
    cs, asg, ilen, pk, prover, _img = keys(orc, zg, ctx, built, k)
    same_h_and_bytes(orc, prover, cs, pk, asg.advice_values(), asg.instance_values(ilen))
    prover.close()


@pytest.mark.parametrize("split", [0, 1])
def test_split_and_single_extended_domain(ctx, zg, orc, split):
    cs, asg, ilen, pk, prover, _img = keys(orc, zg, ctx, toy_circuit(7, force_degree=6), 7, ZG_SPLIT_DOMAIN=split)
    same_h_and_bytes(orc, prover, cs, pk, asg.advice_values(), asg.instance_values(ilen))
    prover.close()


def test_a_batch_of_three_with_different_seeds(ctx, zg, orc):
    cs, asg, ilen, pk, prover, _img = keys(orc, zg, ctx, toy_circuit(8, force_degree=6), 8)
    adv, inst = asg.advice_values(), asg.instance_values(ilen)
    en = 1 << cs.extended_k()
    prover.set_batch(3)
    seeds = [11, 12, 13]
    for overlap in (False,):  # (lock-step batches are the throughput form's)
        prover.set_overlap(overlap)
        proofs, sts = prover.prove_batch([adv] * 3, [inst] * 3, seeds)
        assert sts == [0, 0, 0]
        for b, seed in enumerate(seeds):
            st, want, tr = orc.create_proof(pk, adv, inst, seed, want_trace=True)
            assert st == 0
            assert np.array_equal(prover.fetch(0, 0, en, slot=b), tr.array("h_ext", en)), ("h_ext", overlap, b)
            assert proofs[b] == want, ("proof bytes", overlap, b)
            orc.trace_free(tr)
    prover.close()


def test_tiny_model_k14_in_both_scheduling_forms(ctx, zg, orc):
    import wnn_circuit
    import wnn_model

    orc.load().orc_set_threads(16)
    k, name = wnn_model.MNIST_TINY
    cs, asg, ilen, _scores = wnn_circuit.build(wnn_model.load_checked_in(name), wnn_model.load_test_image(), k)
    cs, asg, ilen, pk, prover, _img = keys(orc, zg, ctx, (cs, asg, ilen), k)
    same_h_and_bytes(orc, prover, cs, pk, asg.advice_values(), asg.instance_values(ilen), seeds=(21, 22))
    prover.close()


def random_evaluate_h(orc, prover, cs, k, seed, beta=None):
    """zg_prover_evaluate_h on random polynomials and challenges: full-size values in every cell"""
    n, en = 1 << k, 1 << cs.extended_k()
    chunk = cs.degree() - 2
    sets = (len(cs.perm_columns) + chunk - 1) // chunk if cs.perm_columns else 0
    nl = len(cs.lookups)

    def fam(i, count):
        return orc.fill_fr(seed * 16 + i, count * n).reshape(count, n, 4) if count else np.zeros((0, n, 4), np.uint64)

    ch = orc.fill_fr(seed * 16 + 9, 4)
    return prover.evaluate_h(fam(0, cs.n_advice), fam(1, cs.n_instance), fam(2, sets), fam(3, nl), fam(4, 2 * nl), ch[0],
                             ch[1] if beta is None else beta, ch[2], ch[3], en)


UNSATISFIED = {
    "toy k8 degree 6": lambda: (toy_circuit(8, force_degree=6), 8),
    "toy k7 two lookups": lambda: (toy_circuit(7, two_lookups=True), 7),
    "7 columns, chunk 3": lambda: (perm_circuit(6, 7, 5), 6),
    "coefficients at the classifier's edges": lambda: (coefficient_circuit(7), 7),
    "merged selectors": lambda: (variant_circuit("merged_selectors", k=6), 6),
    "tiny model k14": None,
}


@pytest.mark.parametrize("name", list(UNSATISFIED))
def test_default_kernel_equals_the_unscaled_one_on_random_inputs(ctx, zg, orc, name):
    if UNSATISFIED[name] is None:
        import wnn_circuit
        import wnn_model

        k, model = wnn_model.MNIST_TINY
        built = wnn_circuit.build(wnn_model.load_checked_in(model), wnn_model.load_test_image(), k)[:3]
    else:
        built, k = UNSATISFIED[name]()
    cs, _asg, _ilen, _pk, new, _i1 = keys(orc, zg, ctx, built, k)
    _cs, _asg, _ilen, _pk, old, _i2 = keys(orc, zg, ctx, built, k, ZG_EVALH_GROUPED=0)
    for seed in (1, 2):
        assert np.array_equal(random_evaluate_h(orc, new, cs, k, seed), random_evaluate_h(orc, old, cs, k, seed)), seed
    # beta = 0 has no inverse: the default kernel takes the unscaled term for that proof
    zero = np.zeros(4, np.uint64)
    assert np.array_equal(random_evaluate_h(orc, new, cs, k, 3, beta=zero), random_evaluate_h(orc, old, cs, k, 3, beta=zero))
    new.close()
    old.close()
