"""The arithmetic-level entries on device pointers (include/zg_halo2.h, "the arithmetic level on device pointers"), each
against Python integers or the oracle's Trace, for EQUALITY of field elements:

  zg_permute_expression_pair(_dev)   lookup_cases.permute_ref / check_permuted on the adversarial value families, at
                                     k = 4 (less than one sort chunk), 10 (exactly one), 11 (first global stride), 12
  zg_prover_lookup_compress_dev      width 1 and width 2 with a rotation of -1 that wraps, theta = 0, 1, random
  zg_lookup_product_terms_dev        n = 1, 255, 256, 257, 1025; beta = gamma = 0; every value r - 1
  zg_prover_permutation_terms_dev    two sets, the last not full, chained through zg_grand_product_dev == Trace.perm_z
  zg_fr_lincomb_dev                  counts around the chunk of ZG_LINCOMB_CHUNK = 64 terms and twice it, the lazy sum's worst case
  zg_prover_evaluate_h_dev           == Trace.h_ext, the inputs of the host form's test
  zg_fr_random_dev                   == orc.rand_fr

(pow2_gaps needs 505 distinct values: it does not exist at k = 4, where a column has 10 usable rows.)"""
import random

import numpy as np
import pytest
import torch

import arith_level
import lookup_cases as lc
import poly_ref as pr
from circuits import toy_circuit, variant_circuit

pytestmark = pytest.mark.gpu

R = pr.R
CHUNK = 64  # ZG_LINCOMB_CHUNK
SIZES = [1, 255, 256, 257, 1025]


def dev(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def filled(shape) -> torch.Tensor:
    t = torch.full(shape, -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def host(ctx, t: torch.Tensor) -> np.ndarray:
    ctx.sync()
    return t.cpu().numpy().view(np.uint64)


def status_of(zg, call) -> int:
    with pytest.raises(zg.ZgError) as e:
        call()
    return e.value.status


# ------------------------------------------------------------------ permute_expression_pair
FAMILIES = ["all_equal", "permutation", "one_heavy_table", "runs", "half_r", "pow2_gaps"]
PERMUTE_CASES = [(name, k) for k in (4, 10, 11, 12) for name in FAMILIES if not (name == "pow2_gaps" and k == 4)]


def permute_case(ctx, k, usable, table, inputs, host_form=True):
    n = 1 << k
    junk = [(7 * i + 3) % R for i in range(n - usable)]  # rows >= usable: not part of the argument
    a_in, a_tab = pr.from_ints(inputs + junk), pr.from_ints(table + junk[::-1])
    d_in, d_tab, d_a, d_s = dev(a_in), dev(a_tab), filled((n, 4)), filled((n, 4))
    ctx.permute_expression_pair_dev(d_in.data_ptr(), d_tab.data_ptr(), k, usable, d_a.data_ptr(), d_s.data_ptr())
    got_a, got_s = host(ctx, d_a), host(ctx, d_s)
    lc.check_permuted(inputs, table, pr.to_ints(got_a[:usable]), pr.to_ints(got_s[:usable]))
    assert not got_a[usable:].any() and not got_s[usable:].any(), "rows >= usable are zero"
    assert np.array_equal(host(ctx, d_in), a_in) and np.array_equal(host(ctx, d_tab), a_tab), "the inputs are untouched"
    if host_form:
        h_a, h_s = ctx.permute_expression_pair(a_in, a_tab, usable)
        assert np.array_equal(h_a, got_a) and np.array_equal(h_s, got_s), "host form == device form"


@pytest.mark.parametrize("name,k", PERMUTE_CASES)
def test_permute_families(ctx, name, k):
    table, inputs = lc.make(name, k)
    permute_case(ctx, k, lc.usable_rows(k), table, inputs)


def test_permute_every_row_usable(ctx):
    k = 10
    n = 1 << k
    table, inputs = lc.FAMILIES["runs"](n, random.Random("full"))
    permute_case(ctx, k, n, table, inputs)


def test_permute_missing_input_and_argument_errors(ctx, zg):
    k = 10
    n, usable = 1 << k, lc.usable_rows(k)
    table, inputs = lc.make("runs", k)
    stranger = next(v for v in range(1, R) if v not in set(table))
    inputs = list(inputs)
    inputs[usable // 2] = stranger
    d_in, d_tab = dev(pr.from_ints(inputs + [0] * (n - usable))), dev(pr.from_ints(table + [0] * (n - usable)))
    d_a, d_s = filled((n, 4)), filled((n, 4))

    def call(kk=k, u=usable, out_a=d_a):
        ctx.permute_expression_pair_dev(d_in.data_ptr(), d_tab.data_ptr(), kk, u, out_a.data_ptr(), d_s.data_ptr())

    assert status_of(zg, call) == -5  # ZG_ERR_CONSTRAINT
    assert status_of(zg, lambda: call(u=0)) == -1
    assert status_of(zg, lambda: call(u=n + 1)) == -1
    assert status_of(zg, lambda: call(out_a=d_in)) == -1
    assert status_of(zg, lambda: call(kk=3, u=2)) == -4
    assert status_of(zg, lambda: call(kk=21)) == -4
    ctx.sync()


# ------------------------------------------------------------------ one prover per circuit, shared by the tests below
class Setup:
    def __init__(self, orc, zg, ctx, circuit, seed=21):
        self.cs, self.asg, self.ilen = circuit
        cs, asg = self.cs, self.asg
        self.k, self.n = cs.k, 1 << cs.k
        self.img = cs.to_c()
        self.params = orc.params_new(cs.k, 0xABCDEF)
        self.vk_repr = orc.fr_from_int(0x1234567)
        self.fixed, self.sigma = asg.fixed_values(), asg.sigma_values()
        self.pk = orc.ProvingKey(self.img, self.fixed, self.sigma, self.params, self.vk_repr)
        self.prover = zg.Prover(ctx, self.img, self.fixed, self.sigma, self.params.g_np(), self.params.g_lagrange_np(), self.vk_repr)
        self.seed = seed
        bf = cs.blinding_factors()
        self.bf, self.usable = bf, self.n - (bf + 1)
        self.adv = asg.advice_values().copy()
        for c in range(cs.n_advice):  # create_proof's advice blinding: tag 1, index = column * (bf + 1) + j
            for j in range(bf + 1):
                self.adv[c, self.usable + j] = orc.rand_fr(seed, 1, c * (bf + 1) + j)
        self.inst = np.zeros((cs.n_instance, self.n, 4), np.uint64)
        self.inst[:, :self.ilen] = asg.instance_values(self.ilen)
        self.ref = arith_level.HostBackend(orc, cs, self.fixed, self.sigma, self.params, seed, None)

    def trace(self, orc):
        st, _, tr = orc.create_proof(self.pk, self.asg.advice_values(), self.asg.instance_values(self.ilen), self.seed, want_trace=True)
        assert st == 0
        return tr


@pytest.fixture(scope="module")
def two_lookups(orc, zg, ctx):
    cs, asg, ilen = toy_circuit(k=5, two_lookups=True)
    for r in range(1 << cs.k):  # the second lookup's selector (fixed column 3) is off in the circuit as it comes: switch it on,
        asg.set(0, 3, r, 1)     # so that its inputs a1 and a1(-1) show in the compressed column (compression proves nothing)
    s = Setup(orc, zg, ctx, (cs, asg, ilen))
    yield s
    s.prover.close()


@pytest.fixture(scope="module")
def toy5(orc, zg, ctx):
    s = Setup(orc, zg, ctx, toy_circuit(k=5))
    yield s
    s.prover.close()


# ------------------------------------------------------------------ compress_expressions
@pytest.mark.parametrize("theta", [0, 1, 0x2B1D5A3C9E7F00112233445566778899AABBCCDDEEFF0123456789ABCDEF0123 % R])
def test_lookup_compress(ctx, zg, two_lookups, theta):
    s = two_lookups
    assert [len(ins) for ins, _ in s.cs.lookups] == [1, 2]
    assert any(s.cs.queries[q][2] == -1 for ins, _ in s.cs.lookups for e in ins for key in e.terms for q in key), "a rotation of -1"
    d_adv, d_inst = dev(s.adv), dev(s.inst)
    for l in range(2):
        want_in, want_tab = np.zeros((s.n, 4), np.uint64), np.zeros((s.n, 4), np.uint64)
        s.ref.compress(l, s.adv, s.inst, theta, want_in, want_tab)
        d_in, d_tab = filled((s.n, 4)), filled((s.n, 4))
        s.prover.lookup_compress_dev(l, d_adv.data_ptr(), d_inst.data_ptr(), zg.fr_from_int(theta), d_in.data_ptr(), d_tab.data_ptr())
        assert np.array_equal(host(ctx, d_in), want_in), (l, "input")
        assert np.array_equal(host(ctx, d_tab), want_tab), (l, "table")
    assert want_in[0].any() and not np.array_equal(want_in[0], want_in[1]), "row 0 reads the blinded last row through rotation -1"
    assert status_of(zg, lambda: s.prover.lookup_compress_dev(2, d_adv.data_ptr(), d_inst.data_ptr(), zg.fr_from_int(theta),
                                                              d_in.data_ptr(), d_tab.data_ptr())) == -1


# ------------------------------------------------------------------ lookup product terms
def terms_case(ctx, zg, cols, beta, gamma):
    n = len(cols[0])
    d = [dev(pr.from_ints(c)) for c in cols]
    d_num, d_den = filled((n, 4)), filled((n, 4))
    ctx.lookup_product_terms_dev(*[t.data_ptr() for t in d], zg.fr_from_int(beta), zg.fr_from_int(gamma), n, d_num.data_ptr(),
                                 d_den.data_ptr())
    inp, tab, a, sp = cols
    assert pr.to_ints(host(ctx, d_num)) == [(x + beta) * (y + gamma) % R for x, y in zip(inp, tab)]
    assert pr.to_ints(host(ctx, d_den)) == [(x + beta) * (y + gamma) % R for x, y in zip(a, sp)]


@pytest.mark.parametrize("n", SIZES)
def test_lookup_product_terms(ctx, zg, n):
    rng = random.Random(n)
    cols = [[rng.randrange(R) for _ in range(n)] for _ in range(4)]
    terms_case(ctx, zg, cols, rng.randrange(R), rng.randrange(R))


def test_lookup_product_terms_edges(ctx, zg):
    rng = random.Random(5)
    cols = [[rng.randrange(R) for _ in range(257)] for _ in range(4)]
    terms_case(ctx, zg, cols, 0, 0)
    terms_case(ctx, zg, [[R - 1] * 257] * 4, R - 1, R - 1)


# ------------------------------------------------------------------ permutation terms, chained
def perm_chain_case(ctx, zg, orc, s):
    cs, n, usable = s.cs, s.n, s.usable
    sets = s.prover.permutation_sets()
    assert sets == arith_level.n_sets(cs)
    tr = s.trace(orc)
    beta, gamma = pr.to_int(tr.fe("beta")), pr.to_int(tr.fe("gamma"))
    want_z = tr.array("perm_z", sets * n).reshape(sets, n, 4)
    orc.trace_free(tr)
    d_adv, d_inst = dev(s.adv), dev(s.inst)
    z0 = zg.fr_from_int(1)
    for st in range(sets):
        want_num, want_den = np.zeros((n, 4), np.uint64), np.zeros((n, 4), np.uint64)
        s.ref.perm_terms(st, s.adv, s.inst, beta, gamma, want_num, want_den)
        d_num, d_den, d_z = filled((n, 4)), filled((n, 4)), filled((n, 4))
        s.prover.permutation_terms_dev(st, d_adv.data_ptr(), d_inst.data_ptr(), zg.fr_from_int(beta), zg.fr_from_int(gamma),
                                       d_num.data_ptr(), d_den.data_ptr())
        assert np.array_equal(host(ctx, d_num), want_num), (st, "num")
        assert np.array_equal(host(ctx, d_den), want_den), (st, "den")
        ctx.grand_product_dev(d_num.data_ptr(), d_den.data_ptr(), z0, n, d_z.data_ptr())
        z = host(ctx, d_z)
        assert np.array_equal(z[:usable + 1], want_z[st][:usable + 1]), (st, "z on rows <= usable")
        z0 = z[usable]  # chaining is the caller's job
    assert status_of(zg, lambda: s.prover.permutation_terms_dev(sets, d_adv.data_ptr(), d_inst.data_ptr(), z0, z0,
                                                                d_num.data_ptr(), d_den.data_ptr())) == -1
    return sets


def test_permutation_terms_two_sets_last_not_full(ctx, zg, orc, toy5):
    assert len(toy5.cs.perm_columns) == 5 and toy5.cs.degree() - 2 == 3
    assert perm_chain_case(ctx, zg, orc, toy5) == 2


def test_permutation_terms_no_lookup_variant(ctx, zg, orc):
    s = Setup(orc, zg, ctx, variant_circuit("no_lookup"))
    try:
        assert perm_chain_case(ctx, zg, orc, s) >= 1
    finally:
        s.prover.close()


# ------------------------------------------------------------------ linear combinations
def lincomb_case(ctx, polys, coeffs, n, sub0):
    """polys: list of lists of canonical integers (or a Montgomery array [count, n, 4])"""
    arr = polys if isinstance(polys, np.ndarray) else (np.stack([pr.from_ints(p) for p in polys]) if polys else np.zeros((0, n, 4), np.uint64))
    ints = [pr.to_ints(a) for a in arr]
    d_polys, d_out = dev(arr) if len(arr) else None, filled((n, 4))
    ptrs = [d_polys[j].data_ptr() for j in range(len(arr))]
    ctx.fr_lincomb_dev(ptrs, pr.from_ints(coeffs) if coeffs else [], n, d_out.data_ptr(), None if sub0 is None else pr.from_int(sub0))
    want = [sum(c * p[i] for c, p in zip(coeffs, ints)) % R for i in range(n)]
    if sub0 is not None:
        want[0] = (want[0] - sub0) % R
    got = host(ctx, d_out)
    assert pr.to_ints(got) == want
    assert all(v < R for v in pr._rows(got)), "what leaves the kernel is canonical"


@pytest.mark.parametrize("count", [0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1])
@pytest.mark.parametrize("with_sub", [False, True])
def test_lincomb_counts(ctx, count, with_sub):
    n = 257
    rng = random.Random(count)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(count)]
    coeffs = [rng.randrange(R) for _ in range(count)]
    for j, special in zip(range(count), (0, 1, R - 1)):  # among the coefficients: 0, 1 and r - 1
        coeffs[-1 - j] = special
    lincomb_case(ctx, polys, coeffs, n, rng.randrange(R) if with_sub else None)


@pytest.mark.parametrize("n", SIZES)
def test_lincomb_sizes(ctx, n):
    rng = random.Random(n)
    count = CHUNK + 1
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(count)]
    lincomb_case(ctx, polys, [rng.randrange(R) for _ in range(count)], n, R - 1)


def test_lincomb_worst_case_of_the_lazy_sum(ctx):
    """chunk bound + 1 terms, every coefficient and every value r - 1 -- as canonical values, and as the largest STORED bit
    pattern r - 1 a kernel can meet."""
    n, count = 256, CHUNK + 1
    lincomb_case(ctx, [[R - 1] * n] * count, [R - 1] * count, n, R - 1)
    stored = np.stack([pr.stored([R - 1] * n)] * count)
    lincomb_case(ctx, stored, [R - 1] * count, n, None)
    lincomb_case(ctx, stored, pr.to_ints(pr.stored([R - 1] * count)), n, None)  # ... and stored coefficients


def test_lincomb_aliasing_is_refused(ctx, zg):
    d = dev(pr.from_ints(list(range(3 * 16))).reshape(3, 16, 4))
    cf = pr.from_ints([1, 2, 3])
    ptrs = [d[j].data_ptr() for j in range(3)]
    for j in range(3):
        assert status_of(zg, lambda: ctx.fr_lincomb_dev(ptrs, cf, 16, ptrs[j])) == -1
    ctx.sync()


# ------------------------------------------------------------------ evaluate_h on device pointers
def test_evaluate_h_dev_equals_the_trace(ctx, zg, orc, toy5):
    s = toy5
    cs, n, en = s.cs, s.n, 1 << s.cs.extended_k()
    tr = s.trace(orc)
    d = orc.domain(cs.degree(), s.k)
    nl, sets = len(cs.lookups), tr.n_sets
    pin = tr.array("permuted_input", nl * n).reshape(nl, n, 4)
    ptab = tr.array("permuted_table", nl * n).reshape(nl, n, 4)
    permuted = np.stack([x for l in range(nl) for x in (pin[l], ptab[l])])

    def coeffs(cols):
        return dev(np.stack([orc.lagrange_to_coeff(d, c) for c in cols]))

    fams = [coeffs(s.adv), coeffs(s.inst), coeffs(tr.array("perm_z", sets * n).reshape(sets, n, 4)),
            coeffs(tr.array("lookup_z", nl * n).reshape(nl, n, 4)), coeffs(permuted)]
    d_h = filled((en, 4))
    s.prover.evaluate_h_dev(*[t.data_ptr() for t in fams], tr.fe("theta"), tr.fe("beta"), tr.fe("gamma"), tr.fe("y"), d_h.data_ptr())
    assert np.array_equal(host(ctx, d_h), tr.array("h_ext", en))
    orc.trace_free(tr)
    # the prover still proves afterwards (slot 0 was used as scratch)
    adv, inst = s.asg.advice_values(), s.asg.instance_values(s.ilen)
    assert s.prover.prove(adv, inst, 5) == orc.create_proof(s.pk, adv, inst, 5)[1]


# ------------------------------------------------------------------ rand_fr on the device
def test_fr_random_dev(ctx, orc):
    count, tag, seed = 1000, 6, 0xC0DE
    d = filled((count, 4))
    ctx.fr_random_dev(seed, tag, d.data_ptr(), count)
    got = host(ctx, d)
    for i in (0, 1, count - 1):
        assert np.array_equal(got[i], orc.rand_fr(seed, tag, i)), i
