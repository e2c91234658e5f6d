"""create_proof walked by the CALLER over the library's arithmetic-level entries.

`create_proof(be, ...)` is halo2's own schedule -- halo2_proofs v2023_04_20 src/plonk/prover.rs, in the order of
oracle/prover.c from its transcript on -- with every array behind a small backend interface and everything the host keeps
(the Keccak EvmTranscript, the challenges, the evaluations, the opening point sets) as Python integers.  Two backends:

  HostBackend    numpy arrays and the oracle's pieces (orc.msm, orc.lagrange_to_coeff, orc.grand_product, orc.eval_poly,
                 orc.kate_division, ...), Python integers for the steps the oracle has no entry for, lookup_cases.permute_ref
                 for the permuted columns -- and h taken from the oracle's Trace: it pins the DRIVER on a machine without a GPU.
  DeviceBackend  torch tensors in HBM and the library's *_dev entries; only commitments, evaluations and the one chained z
                 value per permutation set cross to the host.

The interface (arrays are [rows][n][4] uint64 / int64 "matrices", m[i] a column, v[None] a matrix of one column; scalars are
canonical integers; outputs are written into arrays the driver allocated):
  cols(np) zeros(rows) rand(tag, count) put(dst, row0, src, src0, count) get1(v, row)
  commit(m, lagrange) -> [(x, y)]     to_coeff(m) -> m'       evals(m, [(row, point)]) -> [int]
  compress(l, adv, inst, theta, out_in, out_tab)   permute(inp, tab, usable, out_a, out_s)
  lookup_terms(inp, tab, a, s, beta, gamma, num, den)   perm_terms(set, adv, inst, beta, gamma, num, den)
  grand_product(num, den, z0, out)   evaluate_h(adv_p, inst_p, pz_p, lz_p, perm_p, theta, beta, gamma, y) -> h
  h_pieces(h) -> m   lincomb(vs, coeffs, sub0, out)   kate(v, z, out)   keccak(bytes)
  fixed_polys / sigma_polys: the coefficient forms halo2's ProvingKey holds."""
import numpy as np

import poly_ref as pr
from circuit import ADVICE, DELTA, FIXED, INSTANCE, R, omega_for
from transcript_ref import EvmWriter

# blinding tags of oracle/prover.h (rand_fr(key, tag, index))
TAG_ADVICE_BLIND, TAG_PERMUTED_INPUT, TAG_PERMUTED_TABLE, TAG_PERM_Z, TAG_LOOKUP_Z, TAG_RANDOM_POLY = 1, 2, 3, 4, 5, 6


def n_sets(cs) -> int:
    chunk = cs.degree() - 2
    return (len(cs.perm_columns) + chunk - 1) // chunk if cs.perm_columns else 0


def create_proof(be, cs, vk_repr, advice, instance, writer=EvmWriter) -> bytes:
    """advice: uint64[A][n][4] as assigned (the blinding rows are overwritten here); instance: uint64[I][len][4];
    writer: the transcript's writer class (tests/transcript_ref.py)."""
    k = cs.k
    n, bf = 1 << k, cs.blinding_factors()
    usable = n - (bf + 1)
    A, I, NL, P = cs.n_advice, cs.n_instance, len(cs.lookups), len(cs.perm_columns)
    sets, qpd, w = n_sets(cs), cs.degree() - 1, omega_for(k)
    tr = writer(be.keccak)

    # 1. vk and instance scalars
    tr.common_scalar(pr.to_int(vk_repr))
    instance = np.ascontiguousarray(instance, dtype=np.uint64).reshape(I, -1, 4) if I else np.zeros((0, 0, 4), np.uint64)
    inst_cols = np.zeros((I, n, 4), np.uint64)
    inst_cols[:, :instance.shape[1]] = instance
    for c in range(I):
        for v in pr.to_ints(instance[c]) if instance.shape[1] else []:
            tr.common_scalar(v)
    d_inst = be.cols(inst_cols)

    # 2. advice: blind the last bf + 1 rows, commit_lagrange, theta
    d_adv = be.cols(np.ascontiguousarray(advice, dtype=np.uint64).reshape(A, n, 4))
    if A:
        rnd = be.rand(TAG_ADVICE_BLIND, A * (bf + 1))
        for c in range(A):
            be.put(d_adv[c], usable, rnd, c * (bf + 1), bf + 1)
    for pt in be.commit(d_adv, True):
        tr.write_point(pt)
    theta = tr.squeeze()

    # 3. lookups: compress, permute, blind, commit; beta, gamma
    cin, ctab, permuted = be.zeros(NL), be.zeros(NL), be.zeros(2 * NL)  # permuted: a'_0, s'_0, a'_1, ...
    if NL:
        r_in, r_tab = be.rand(TAG_PERMUTED_INPUT, NL * (bf + 1)), be.rand(TAG_PERMUTED_TABLE, NL * (bf + 1))
    for l in range(NL):
        be.compress(l, d_adv, d_inst, theta, cin[l], ctab[l])
        be.permute(cin[l], ctab[l], usable, permuted[2 * l], permuted[2 * l + 1])
        be.put(permuted[2 * l], usable, r_in, l * (bf + 1), bf + 1)
        be.put(permuted[2 * l + 1], usable, r_tab, l * (bf + 1), bf + 1)
    for pt in be.commit(permuted, True):
        tr.write_point(pt)
    beta, gamma = tr.squeeze(), tr.squeeze()

    # 4. permutation sets: z of set s starts from z of set s - 1 at row `usable`
    pz, lz, nd = be.zeros(sets), be.zeros(NL), be.zeros(2)
    z0 = 1
    if sets:
        r_pz = be.rand(TAG_PERM_Z, sets * bf)
    for s in range(sets):
        be.perm_terms(s, d_adv, d_inst, beta, gamma, nd[0], nd[1])
        be.grand_product(nd[0], nd[1], z0, pz[s])
        z0 = be.get1(pz[s], usable)
        be.put(pz[s], n - bf, r_pz, s * bf, bf)
    for pt in be.commit(pz, True):
        tr.write_point(pt)

    # 5. lookup products
    if NL:
        r_lz = be.rand(TAG_LOOKUP_Z, NL * bf)
    for l in range(NL):
        be.lookup_terms(cin[l], ctab[l], permuted[2 * l], permuted[2 * l + 1], beta, gamma, nd[0], nd[1])
        be.grand_product(nd[0], nd[1], 1, lz[l])
        be.put(lz[l], n - bf, r_lz, l * bf, bf)
    for pt in be.commit(lz, True):
        tr.write_point(pt)

    # 6. vanishing::commit's random polynomial (coefficient basis); y
    random_poly = be.rand(TAG_RANDOM_POLY, n)
    tr.write_point(be.commit(random_poly[None], False)[0])
    y = tr.squeeze()

    # 7. lagrange_to_coeff   8. evaluate_h   9. extended_to_coeff, pieces, commitments; x
    adv_p, inst_p, pz_p, lz_p, perm_p = (be.to_coeff(m) for m in (d_adv, d_inst, pz, lz, permuted))
    h = be.evaluate_h(adv_p, inst_p, pz_p, lz_p, perm_p, theta, beta, gamma, y)
    pieces = be.h_pieces(h)
    for pt in be.commit(pieces, False):
        tr.write_point(pt)
    x = tr.squeeze()
    xn = pow(x, n, R)

    # 10. evaluations, in create_proof's order
    def rot(r):
        return x * pow(w, r % n, R) % R

    x_next, x_inv, x_last = rot(1), rot(-1), rot(-(bf + 1))
    queries = []  # (point, polynomial, evaluation) in create_proof's query order
    adv_ev = be.evals(adv_p, [(c, rot(r)) for c, r in cs.advice_queries])
    for (c, r), e in zip(cs.advice_queries, adv_ev):
        tr.write_scalar(e)
        queries.append((rot(r), adv_p[c], e))
    fix_ev = be.evals(be.fixed_polys, [(c, rot(r)) for c, r in cs.fixed_queries])
    for e in fix_ev:
        tr.write_scalar(e)
    h_poly = be.zeros(1)[0]  # vanishing::evaluate: sum_i x^(n i) h_i
    be.lincomb([pieces[i] for i in range(qpd)], [pow(xn, i, R) for i in range(qpd)], None, h_poly)
    random_eval = be.evals(random_poly[None], [(0, x)])[0]
    tr.write_scalar(random_eval)
    sig_ev = be.evals(be.sigma_polys, [(c, x) for c in range(P)])
    for e in sig_ev:
        tr.write_scalar(e)
    pz_pairs = [(s, pt) for s in range(sets) for pt in ((x, x_next, x_last) if s + 1 < sets else (x, x_next))]
    pz_ev = dict(zip(pz_pairs, be.evals(pz_p, pz_pairs)))
    for key in pz_pairs:
        tr.write_scalar(pz_ev[key])
    lz_ev = be.evals(lz_p, [(l, pt) for l in range(NL) for pt in (x, x_next)])
    pm_ev = be.evals(perm_p, [(2 * l + j, pt) for l in range(NL) for j, pt in ((0, x), (0, x_inv), (1, x))])
    for l in range(NL):
        for e in (lz_ev[2 * l], lz_ev[2 * l + 1], pm_ev[3 * l], pm_ev[3 * l + 1], pm_ev[3 * l + 2]):
            tr.write_scalar(e)
    for s in range(sets):
        queries += [(x, pz_p[s], pz_ev[(s, x)]), (x_next, pz_p[s], pz_ev[(s, x_next)])]
    for s in reversed(range(sets - 1)):
        queries.append((x_last, pz_p[s], pz_ev[(s, x_last)]))
    for l in range(NL):
        queries += [(x, lz_p[l], lz_ev[2 * l]), (x, perm_p[2 * l], pm_ev[3 * l]), (x, perm_p[2 * l + 1], pm_ev[3 * l + 2]),
                    (x_inv, perm_p[2 * l], pm_ev[3 * l + 1]), (x_next, lz_p[l], lz_ev[2 * l + 1])]
    queries += [(rot(r), be.fixed_polys[c], e) for (c, r), e in zip(cs.fixed_queries, fix_ev)]
    queries += [(x, be.sigma_polys[c], sig_ev[c]) for c in range(P)]
    queries.append((x, h_poly, be.evals(h_poly[None], [(0, x)])[0]))
    queries.append((x, random_poly, random_eval))

    # 11. v   12. GWC: one witness polynomial per point, points in first-appearance order
    v = tr.squeeze()
    points = list(dict.fromkeys(q[0] for q in queries))
    wit, batch = be.zeros(len(points)), be.zeros(1)[0]
    for s, z in enumerate(points):
        group = [q for q in queries if q[0] == z]
        coeffs = [pow(v, len(group) - 1 - j, R) for j in range(len(group))]
        eval_batch = sum(c * q[2] for c, q in zip(coeffs, group)) % R
        be.lincomb([q[1] for q in group], coeffs, eval_batch, batch)
        be.kate(batch, z, wit[s])
    for pt in be.commit(wit, False):
        tr.write_point(pt)
    return bytes(tr.out)


# ---------------------------------------------------------------------------------------------------- the CPU backend
class HostBackend:
    def __init__(self, orc, cs, fixed_values, sigma_values, params, seed, h_ext, challenges=None):
        """h_ext: the oracle Trace's h on the extended coset (this backend does not evaluate h);
        challenges: the Trace's (theta, beta, gamma, y) as integers, checked when evaluate_h is reached."""
        import lookup_cases

        self.orc, self.cs, self.seed, self.h_ext, self.challenges = orc, cs, seed, h_ext, challenges
        self.permute_ref = lookup_cases.permute_ref
        self.n = 1 << cs.k
        self.d = orc.domain(cs.degree(), cs.k)
        self.g, self.gl = params.g_np(), params.g_lagrange_np()
        self.fixed_ints = [pr.to_ints(c) for c in fixed_values]
        self.sigma_ints = [pr.to_ints(c) for c in sigma_values]
        self.fixed_polys, self.sigma_polys = self.to_coeff(fixed_values), self.to_coeff(sigma_values)
        self.keccak = orc.keccak256

    def cols(self, a):
        return np.array(a, dtype=np.uint64).reshape(-1, self.n, 4)

    def zeros(self, rows):
        return np.zeros((rows, self.n, 4), np.uint64)

    def rand(self, tag, count):
        return np.stack([self.orc.rand_fr(self.seed, tag, i) for i in range(count)])

    def put(self, dst, row0, src, src0, count):
        dst[row0:row0 + count] = src[src0:src0 + count]

    def get1(self, v, row):
        return pr.to_int(v[row])

    def commit(self, m, lagrange):
        out = []
        for v in m:
            j = self.orc.msm(v, self.gl if lagrange else self.g)
            out.append((self.orc.fq_to_int(j[0:4]), self.orc.fq_to_int(j[4:8])) if j[8:12].any() else (0, 0))
        return out

    def to_coeff(self, m):
        return np.stack([self.orc.lagrange_to_coeff(self.d, c) for c in m]) if len(m) else self.zeros(0)

    def evals(self, m, pairs):
        return [pr.to_int(self.orc.eval_poly(m[i], pr.from_int(pt))) for i, pt in pairs]

    def _cells(self, adv, inst):
        return {FIXED: self.fixed_ints, ADVICE: [pr.to_ints(c) for c in adv], INSTANCE: [pr.to_ints(c) for c in inst]}

    def compress(self, l, adv, inst, theta, out_in, out_tab):
        cols, n, cs = self._cells(adv, inst), self.n, self.cs
        for exprs, out in zip(cs.lookups[l], (out_in, out_tab)):
            vals = []
            for row in range(n):
                def cell(qi):
                    kind, c, r = cs.queries[qi]
                    return cols[kind][c][(row + r) % n]
                acc = 0
                for e in exprs:
                    acc = (acc * theta + e.eval(cell)) % R
                vals.append(acc)
            out[:] = pr.from_ints(vals)

    def permute(self, inp, tab, usable, out_a, out_s):
        a, s = self.permute_ref(pr.to_ints(inp[:usable]), pr.to_ints(tab[:usable]))
        out_a[:], out_s[:] = 0, 0
        out_a[:usable], out_s[:usable] = pr.from_ints(a), pr.from_ints(s)

    def lookup_terms(self, inp, tab, a, s, beta, gamma, num, den):
        i, t, pa, ps = (pr.to_ints(v) for v in (inp, tab, a, s))
        num[:] = pr.from_ints([(x + beta) * (y + gamma) % R for x, y in zip(i, t)])
        den[:] = pr.from_ints([(x + beta) * (y + gamma) % R for x, y in zip(pa, ps)])

    def perm_terms(self, s, adv, inst, beta, gamma, num, den):
        cols, n, cs = self._cells(adv, inst), self.n, self.cs
        chunk, w = cs.degree() - 2, omega_for(cs.k)
        nu, de = [1] * n, [1] * n
        for c in range(s * chunk, min((s + 1) * chunk, len(cs.perm_columns))):
            kind, col = cs.perm_columns[c]
            vals, dw = cols[kind][col], pow(DELTA, c, R)
            for i in range(n):
                de[i] = de[i] * (vals[i] + beta * self.sigma_ints[c][i] + gamma) % R
                nu[i] = nu[i] * (vals[i] + beta * dw + gamma) % R
                dw = dw * w % R
        num[:], den[:] = pr.from_ints(nu), pr.from_ints(de)

    def grand_product(self, num, den, z0, out):
        out[:] = self.orc.grand_product(num, den, pr.from_int(z0))

    def evaluate_h(self, adv_p, inst_p, pz_p, lz_p, perm_p, theta, beta, gamma, y):
        if self.challenges is not None:
            assert (theta, beta, gamma, y) == tuple(self.challenges), "the driver's challenges differ from the oracle's"
        return self.h_ext.copy()

    def h_pieces(self, h):
        return self.orc.extended_to_coeff(self.d, h).reshape(-1, self.n, 4)

    def lincomb(self, vs, coeffs, sub0, out):
        acc = [0] * self.n
        for v, c in zip(vs, coeffs):
            acc = [(a + c * x) % R for a, x in zip(acc, pr.to_ints(v))]
        if sub0 is not None:
            acc[0] = (acc[0] - sub0) % R
        out[:] = pr.from_ints(acc)

    def kate(self, v, z, out):
        out[:] = self.orc.kate_division(v, pr.from_int(z))


# ---------------------------------------------------------------------------------------------------- the device backend
class DeviceBackend:
    """Every array is a torch tensor in HBM; the library's context stream and torch's stream are fenced wherever torch
    itself touches an array (allocation, the blinding rows' copies, the one element read back per permutation set)."""

    def __init__(self, zg, ctx, prover, cs, fixed_values, sigma_values, g_bases, gl_bases, seed):
        import torch

        self.torch, self.zg, self.ctx, self.prover, self.cs, self.seed = torch, zg, ctx, prover, cs, seed
        self.g, self.gl = g_bases, gl_bases
        self.k, self.n, self.en = cs.k, 1 << cs.k, 1 << cs.extended_k()
        _, self.omega_inv = zg.domain_omega(cs.k)
        self.ifft_div = zg.fr_from_int(pow(self.n, -1, R))
        assert prover.permutation_sets() == n_sets(cs)
        # the coefficient forms halo2's ProvingKey holds (pk.fixed_polys, pk.permutation.polys): zg_intt
        self.fixed_polys = self.cols(self._intt_host(fixed_values))
        self.sigma_polys = self.cols(self._intt_host(sigma_values))
        self.keccak = zg.keccak256

    def _intt_host(self, values):
        if not len(values):
            return np.zeros((0, self.n, 4), np.uint64)
        return np.stack([self.ctx.ntt(c, self.omega_inv, self.ifft_div) for c in values])

    def _fr(self, v: int):
        return self.zg.fr_from_int(v)

    def _torch_done(self):  # before the library reads or writes what torch produced
        self.torch.cuda.synchronize()

    def _lib_done(self):  # before torch reads or writes what the library produced
        self.ctx.sync()

    def cols(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, self.n, 4)
        t = self.torch.from_numpy(a.view(np.int64)).cuda()
        self._torch_done()
        return t

    def zeros(self, rows, n=None):
        t = self.torch.zeros((rows, n or self.n, 4), dtype=self.torch.int64, device="cuda")
        self._torch_done()
        return t

    def rand(self, tag, count):
        t = self.torch.empty((count, 4), dtype=self.torch.int64, device="cuda")
        self._torch_done()
        self.ctx.fr_random_dev(self.seed, tag, t.data_ptr(), count)
        return t

    def put(self, dst, row0, src, src0, count):
        self._lib_done()
        dst[row0:row0 + count] = src[src0:src0 + count]
        self._torch_done()

    def get1(self, v, row):
        self._lib_done()
        return pr.to_int(v[row].cpu().numpy().view(np.uint64))

    def commit(self, m, lagrange):
        rows = m.shape[0]
        if not rows:
            return []
        xyzz = self.torch.empty((rows, 16), dtype=self.torch.int64, device="cuda")
        self._torch_done()
        self.ctx.msm_batch_dev(self.gl if lagrange else self.g, m.data_ptr(), self.n, rows, self.n, xyzz.data_ptr())
        jac = self.ctx.msm_finish(xyzz.data_ptr(), rows)
        return [(self.zg.fq_to_int(j[0:4]), self.zg.fq_to_int(j[4:8])) if j[8:12].any() else (0, 0) for j in jac]

    def to_coeff(self, m):
        self._lib_done()
        t = m.clone()
        self._torch_done()
        if t.shape[0]:
            self.ctx.ntt_batch_dev(t.data_ptr(), self.n, t.shape[0], self.k, self.omega_inv, self.ifft_div)
        return t

    def evals(self, m, pairs):
        if not pairs:
            return []
        pts = np.stack([self._fr(pt) for _, pt in pairs])
        out = self.ctx.eval_polys_dev(m.data_ptr(), self.n, self.n, [i for i, _ in pairs], pts)
        return pr.to_ints(out)

    def compress(self, l, adv, inst, theta, out_in, out_tab):
        self.prover.lookup_compress_dev(l, adv.data_ptr() if adv.shape[0] else 0, inst.data_ptr() if inst.shape[0] else 0,
                                        self._fr(theta), out_in.data_ptr(), out_tab.data_ptr())

    def permute(self, inp, tab, usable, out_a, out_s):
        self.ctx.permute_expression_pair_dev(inp.data_ptr(), tab.data_ptr(), self.k, usable, out_a.data_ptr(), out_s.data_ptr())

    def lookup_terms(self, inp, tab, a, s, beta, gamma, num, den):
        self.ctx.lookup_product_terms_dev(inp.data_ptr(), tab.data_ptr(), a.data_ptr(), s.data_ptr(), self._fr(beta),
                                          self._fr(gamma), self.n, num.data_ptr(), den.data_ptr())

    def perm_terms(self, s, adv, inst, beta, gamma, num, den):
        self.prover.permutation_terms_dev(s, adv.data_ptr() if adv.shape[0] else 0, inst.data_ptr() if inst.shape[0] else 0,
                                          self._fr(beta), self._fr(gamma), num.data_ptr(), den.data_ptr())

    def grand_product(self, num, den, z0, out):
        self.ctx.grand_product_dev(num.data_ptr(), den.data_ptr(), self._fr(z0), self.n, out.data_ptr())

    def evaluate_h(self, adv_p, inst_p, pz_p, lz_p, perm_p, theta, beta, gamma, y):
        h = self.zeros(1, self.en)[0]
        ptrs = [m.data_ptr() if m.shape[0] else 0 for m in (adv_p, inst_p, pz_p, lz_p, perm_p)]
        self.prover.evaluate_h_dev(*ptrs, self._fr(theta), self._fr(beta), self._fr(gamma), self._fr(y), h.data_ptr())
        return h

    def h_pieces(self, h):
        qpd = self.cs.degree() - 1
        out = self.zeros(qpd)
        self.ctx.extended_to_coeff_dev(h.data_ptr(), self.k, self.cs.extended_k(), qpd * self.n, out.data_ptr())
        return out

    def lincomb(self, vs, coeffs, sub0, out):
        cf = np.stack([self._fr(c) for c in coeffs]) if coeffs else np.zeros((0, 4), np.uint64)
        self.ctx.fr_lincomb_dev([v.data_ptr() for v in vs], cf, self.n, out.data_ptr(),
                                None if sub0 is None else self._fr(sub0))

    def kate(self, v, z, out):
        self.ctx.kate_division_dev(v.data_ptr(), self.n, self._fr(z), out.data_ptr())
