// BN254 optimal-ate pairing on the host: the last step of a batched GWC verification (verify.hip) and the
// zg_pairing_check helper.  Replaces halo2curves 0.3.3 `bn256::{multi_miller_loop, Gt::final_exponentiation}` as
// `DualMSM::check` (halo2_proofs v2023_04_20 src/poly/kzg/msm.rs) calls it.
//
// Tower: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), xi = 9 + u.  G2 is the D-type twist
// y^2 = x^3 + 3/xi, untwisted by (x, y) -> (x w^2, y w^3).  The Miller loop runs over 6x + 2 with affine G2 steps
// (one Fq2 inversion each: a pairing check is once per batch, so simplicity beats the projective formulas), the two
// Frobenius lines of the optimal ate loop follow, and the final exponentiation is (p^6 - 1)(p^2 + 1) by conjugation,
// inversion and one p^2 power, then (p^4 - p^2 + 1)/r by square-and-multiply.  Vertical lines lie in Fq6 and are
// dropped (the final exponentiation sends them to 1).
#include <cstring>

#include "common.h"

namespace zg {
namespace {

struct Fq2 {
    Fe c0, c1;
};
struct Fq6 {
    Fq2 c0, c1, c2;
};
struct Fq12 {
    Fq6 c0, c1;
};

Fq2 f2_zero() { return {fe_zero(), fe_zero()}; }
Fq2 f2_one() { return {Fq::one(), fe_zero()}; }
bool f2_is_zero(const Fq2& a) { return fe_is_zero(a.c0) && fe_is_zero(a.c1); }
bool f2_eq(const Fq2& a, const Fq2& b) { return fe_eq(a.c0, b.c0) && fe_eq(a.c1, b.c1); }
Fq2 f2_add(const Fq2& a, const Fq2& b) { return {Fq::add(a.c0, b.c0), Fq::add(a.c1, b.c1)}; }
Fq2 f2_sub(const Fq2& a, const Fq2& b) { return {Fq::sub(a.c0, b.c0), Fq::sub(a.c1, b.c1)}; }
Fq2 f2_neg(const Fq2& a) { return {Fq::neg(a.c0), Fq::neg(a.c1)}; }
Fq2 f2_conj(const Fq2& a) { return {a.c0, Fq::neg(a.c1)}; }
Fq2 f2_mul(const Fq2& a, const Fq2& b) {
    const Fe t0 = Fq::mul(a.c0, b.c0), t1 = Fq::mul(a.c1, b.c1);
    const Fe m = Fq::mul(Fq::add(a.c0, a.c1), Fq::add(b.c0, b.c1));
    return {Fq::sub(t0, t1), Fq::sub(Fq::sub(m, t0), t1)};
}
Fq2 f2_sqr(const Fq2& a) { return f2_mul(a, a); }
Fq2 f2_mul_fq(const Fq2& a, const Fe& s) { return {Fq::mul(a.c0, s), Fq::mul(a.c1, s)}; }
Fq2 f2_inv(const Fq2& a) {
    const Fe d = Fq::inv(Fq::add(Fq::sqr(a.c0), Fq::sqr(a.c1)));
    return {Fq::mul(a.c0, d), Fq::neg(Fq::mul(a.c1, d))};
}
// (9 + u)(a + bu) = (9a - b) + (a + 9b)u
Fq2 f2_mul_xi(const Fq2& a) {
    const Fe a8 = Fq::dbl(Fq::dbl(Fq::dbl(a.c0))), b8 = Fq::dbl(Fq::dbl(Fq::dbl(a.c1)));
    return {Fq::sub(Fq::add(a8, a.c0), a.c1), Fq::add(Fq::add(b8, a.c1), a.c0)};
}
// a^e, e a big-endian-walked array of little-endian 32-bit limbs
Fq2 f2_pow(const Fq2& a, const uint32_t* e, int nlimbs) {
    Fq2 r = f2_one();
    for (int i = nlimbs - 1; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = f2_sqr(r);
            if ((e[i] >> b) & 1) r = f2_mul(r, a);
        }
    return r;
}

Fq6 f6_zero() { return {f2_zero(), f2_zero(), f2_zero()}; }
Fq6 f6_one() { return {f2_one(), f2_zero(), f2_zero()}; }
Fq6 f6_add(const Fq6& a, const Fq6& b) { return {f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
Fq6 f6_sub(const Fq6& a, const Fq6& b) { return {f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
Fq6 f6_neg(const Fq6& a) { return {f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
Fq6 f6_mul(const Fq6& a, const Fq6& b) {
    const Fq2 t00 = f2_mul(a.c0, b.c0), t11 = f2_mul(a.c1, b.c1), t22 = f2_mul(a.c2, b.c2);
    const Fq2 t12 = f2_add(f2_mul(a.c1, b.c2), f2_mul(a.c2, b.c1));
    const Fq2 t01 = f2_add(f2_mul(a.c0, b.c1), f2_mul(a.c1, b.c0));
    const Fq2 t02 = f2_add(f2_mul(a.c0, b.c2), f2_mul(a.c2, b.c0));
    return {f2_add(t00, f2_mul_xi(t12)), f2_add(t01, f2_mul_xi(t22)), f2_add(t02, t11)};
}
Fq6 f6_mul_v(const Fq6& a) { return {f2_mul_xi(a.c2), a.c0, a.c1}; }
Fq6 f6_inv(const Fq6& a) {
    const Fq2 A = f2_sub(f2_sqr(a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
    const Fq2 B = f2_sub(f2_mul_xi(f2_sqr(a.c2)), f2_mul(a.c0, a.c1));
    const Fq2 C = f2_sub(f2_sqr(a.c1), f2_mul(a.c0, a.c2));
    const Fq2 F = f2_add(f2_mul(a.c0, A), f2_mul_xi(f2_add(f2_mul(a.c2, B), f2_mul(a.c1, C))));
    const Fq2 fi = f2_inv(F);
    return {f2_mul(A, fi), f2_mul(B, fi), f2_mul(C, fi)};
}

Fq12 f12_one() { return {f6_one(), f6_zero()}; }
Fq12 f12_mul(const Fq12& a, const Fq12& b) {
    const Fq6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    return {f6_add(t0, f6_mul_v(t1)), f6_add(f6_mul(a.c0, b.c1), f6_mul(a.c1, b.c0))};
}
Fq12 f12_sqr(const Fq12& a) { return f12_mul(a, a); }
Fq12 f12_conj(const Fq12& a) { return {a.c0, f6_neg(a.c1)}; }  // a^(p^6)
Fq12 f12_inv(const Fq12& a) {
    const Fq6 d = f6_inv(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return {f6_mul(a.c0, d), f6_neg(f6_mul(a.c1, d))};
}
Fq12 f12_pow(const Fq12& a, const uint64_t* e, int nlimbs) {
    Fq12 r = f12_one();
    bool started = false;
    for (int i = nlimbs - 1; i >= 0; i--)
        for (int b = 63; b >= 0; b--) {
            if (started) r = f12_sqr(r);
            if ((e[i] >> b) & 1) {
                r = started ? f12_mul(r, a) : a;
                started = true;
            }
        }
    return r;
}
bool f12_is_one(const Fq12& a) {
    const Fq6 o = f6_one();
    const Fq2* x = &a.c0.c0;
    const Fq2* y = &o.c0;
    for (int i = 0; i < 3; i++)
        if (!f2_eq(x[i], y[i])) return false;
    const Fq2* z = &a.c1.c0;
    for (int i = 0; i < 3; i++)
        if (!f2_is_zero(z[i])) return false;
    return true;
}

// p^2 and (p^4 - p^2 + 1)/r, little-endian 64-bit limbs
constexpr uint64_t P_SQ[8] = {0x3b5458a2275d69b1ULL, 0xa602072d09eac101ULL, 0x4a50189c6d96cadcULL,
                              0x04689e957a1242c8ULL, 0x26edfa5c34c6b38dULL, 0xb00b855116375606ULL,
                              0x599a6f7c0348d21cULL, 0x0925c4b8763cbf9cULL};
constexpr uint64_t HARD[12] = {0xe81bb482ccdf42b1ULL, 0x5abf5cc4f49c36d4ULL, 0xf1154e7e1da014fdULL,
                               0xdcc7b44c87cdbacfULL, 0xaaa441e3954bcf8aULL, 0x6b887d56d5095f23ULL,
                               0x79581e16f3fd90c6ULL, 0x3b1b1355d189227dULL, 0x4e529a5861876f6bULL,
                               0x6c0eb522d5b12278ULL, 0x331ec15183177fafULL, 0x01baaa710b0759adULL};
constexpr uint64_t ATE_LO = 0x9d797039be763ba8ULL;  // 6x + 2 = 2^64 + ATE_LO, x = 4965661367192848881

struct G2 {
    Fq2 x, y;
    bool inf;
};

// Frobenius on the twist: (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2))
struct FrobConst {
    Fq2 g2, g3;
    FrobConst() {
        uint32_t pm1[8], e3[8], e2[8];
        for (int i = 0; i < 8; i++) pm1[i] = FqParams::p(i);
        pm1[0] -= 1;
        uint64_t rem3 = 0, rem2 = 0;
        for (int i = 7; i >= 0; i--) {  // long division of p - 1 by 3 and by 2
            uint64_t c3 = (rem3 << 32) | pm1[i], c2 = (rem2 << 32) | pm1[i];
            e3[i] = (uint32_t)(c3 / 3);
            rem3 = c3 % 3;
            e2[i] = (uint32_t)(c2 / 2);
            rem2 = c2 % 2;
        }
        const Fq2 xi = {Fq::from_u64(9), Fq::one()};
        g2 = f2_pow(xi, e3, 8);
        g3 = f2_pow(xi, e2, 8);
    }
};
const FrobConst& frob() {
    static const FrobConst c;
    return c;
}
G2 g2_frob(const G2& q) {
    return {f2_mul(f2_conj(q.x), frob().g2), f2_mul(f2_conj(q.y), frob().g3), q.inf};
}

// line through the untwisted T with twist slope lam, at P: yP - lam xP w + (lam xT - yT) v w
Fq12 line_eval(const Fq2& lam, const G2& t, const Affine& p) {
    Fq12 l;
    l.c0 = f6_zero();
    l.c1 = f6_zero();
    l.c0.c0 = {p.y, fe_zero()};
    l.c1.c0 = f2_neg(f2_mul_fq(lam, p.x));
    l.c1.c1 = f2_sub(f2_mul(lam, t.x), t.y);
    return l;
}

// f *= line(T, T)(P); T = 2T
void step_dbl(Fq12& f, G2& t, const Affine& p) {
    if (t.inf) return;
    if (f2_is_zero(t.y)) {  // vertical tangent: the line lies in Fq6
        t.inf = true;
        return;
    }
    const Fq2 xx = f2_sqr(t.x);
    const Fq2 lam = f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(t.y, t.y)));
    f = f12_mul(f, line_eval(lam, t, p));
    const Fq2 x3 = f2_sub(f2_sqr(lam), f2_add(t.x, t.x));
    t.y = f2_sub(f2_mul(lam, f2_sub(t.x, x3)), t.y);
    t.x = x3;
}

// f *= line(T, Q)(P); T = T + Q
void step_add(Fq12& f, G2& t, const G2& q, const Affine& p) {
    if (q.inf) return;
    if (t.inf) {
        t = q;
        return;
    }
    if (f2_eq(t.x, q.x)) {
        if (f2_eq(t.y, q.y)) {
            step_dbl(f, t, p);
            return;
        }
        t.inf = true;  // T = -Q: vertical line
        return;
    }
    const Fq2 lam = f2_mul(f2_sub(q.y, t.y), f2_inv(f2_sub(q.x, t.x)));
    f = f12_mul(f, line_eval(lam, t, p));
    const Fq2 x3 = f2_sub(f2_sub(f2_sqr(lam), t.x), q.x);
    t.y = f2_sub(f2_mul(lam, f2_sub(t.x, x3)), t.y);
    t.x = x3;
}

Fq12 miller_loop(const Affine& p, const G2& q) {
    Fq12 f = f12_one();
    G2 t = q;
    for (int b = 63; b >= 0; b--) {  // bit 64 is the leading one
        f = f12_sqr(f);
        step_dbl(f, t, p);
        if ((ATE_LO >> b) & 1) step_add(f, t, q, p);
    }
    const G2 q1 = g2_frob(q);
    G2 q2 = g2_frob(q1);
    q2.y = f2_neg(q2.y);
    step_add(f, t, q1, p);
    step_add(f, t, q2, p);
    return f;
}

Fq12 final_exp(const Fq12& f) {
    Fq12 t = f12_mul(f12_conj(f), f12_inv(f));  // ^(p^6 - 1)
    t = f12_mul(f12_pow(t, P_SQ, 8), t);        // ^(p^2 + 1)
    return f12_pow(t, HARD, 12);                // ^((p^4 - p^2 + 1)/r)
}

// affine group law on the twist (no line values): what the subgroup test of g2_point_fault walks
G2 g2_dbl(const G2& t) {
    if (t.inf || f2_is_zero(t.y)) return {f2_zero(), f2_zero(), true};
    const Fq2 xx = f2_sqr(t.x);
    const Fq2 lam = f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(t.y, t.y)));
    const Fq2 x3 = f2_sub(f2_sqr(lam), f2_add(t.x, t.x));
    return {x3, f2_sub(f2_mul(lam, f2_sub(t.x, x3)), t.y), false};
}
G2 g2_add(const G2& t, const G2& q) {
    if (q.inf) return t;
    if (t.inf) return q;
    if (f2_eq(t.x, q.x)) return f2_eq(t.y, q.y) ? g2_dbl(t) : G2{f2_zero(), f2_zero(), true};
    const Fq2 lam = f2_mul(f2_sub(q.y, t.y), f2_inv(f2_sub(q.x, t.x)));
    const Fq2 x3 = f2_sub(f2_sub(f2_sqr(lam), t.x), q.x);
    return {x3, f2_sub(f2_mul(lam, f2_sub(t.x, x3)), t.y), false};
}

bool fq_canonical(const Fe& v) {
    for (int i = 7; i >= 0; i--) {
        if (v.l[i] < FqParams::p(i)) return true;
        if (v.l[i] > FqParams::p(i)) return false;
    }
    return false;
}

}  // namespace

// Is q a point a verifying key may hold -- canonical coordinates, on y^2 = x^3 + 3/(9+u), not the identity, and in the
// subgroup of order r (the twist's cofactor is ~2^254: a point of the curve need not be)?  nullptr = yes, else why not.
const char* g2_point_fault(const zg_g2_affine& q) {
    G2 g;
    std::memcpy(&g.x, &q.x, sizeof(Fq2));
    std::memcpy(&g.y, &q.y, sizeof(Fq2));
    g.inf = false;
    if (!fq_canonical(g.x.c0) || !fq_canonical(g.x.c1) || !fq_canonical(g.y.c0) || !fq_canonical(g.y.c1))
        return "a coordinate is not below q";
    if (f2_is_zero(g.x) && f2_is_zero(g.y)) return "the identity";
    const Fq2 xi = {Fq::from_u64(9), Fq::one()};
    const Fq2 b = f2_mul_fq(f2_inv(xi), Fq::from_u64(3));
    if (!f2_eq(f2_sqr(g.y), f2_add(f2_mul(f2_sqr(g.x), g.x), b))) return "not on the twist y^2 = x^3 + 3/(9+u)";
    G2 acc = {f2_zero(), f2_zero(), true};  // r * Q, left to right over the bits of r
    for (int i = 7; i >= 0; i--)
        for (int bit = 31; bit >= 0; bit--) {
            acc = g2_dbl(acc);
            if ((FrParams::p(i) >> bit) & 1) acc = g2_add(acc, g);
        }
    return acc.inf ? nullptr : "outside the subgroup of order r";
}

// prod_i e(p_i, q_i) == 1; identities contribute 1
bool pairing_product_is_one(const Affine* p, const zg_g2_affine* q, size_t n) {
    static_assert(sizeof(zg_g2_affine) == 128 && sizeof(Fq2) == 64, "G2 affine layout");
    Fq12 acc = f12_one();
    for (size_t i = 0; i < n; i++) {
        G2 g;
        std::memcpy(&g.x, &q[i].x, sizeof(Fq2));
        std::memcpy(&g.y, &q[i].y, sizeof(Fq2));
        g.inf = f2_is_zero(g.x) && f2_is_zero(g.y);
        if (g.inf || affine_is_identity(p[i])) continue;
        acc = f12_mul(acc, miller_loop(p[i], g));
    }
    return f12_is_one(final_exp(acc));
}

// t * q on the twist, t a Montgomery scalar: left to right over the bits of the canonical integer, with the affine group
// law above (an SRS contribution multiplies two G2 points, once).  q must have canonical coordinates and lie on the
// twist, or be the identity (0,0), which gives the identity; the subgroup is not asked for.  nullptr = done, else why not.
const char* g2_mul_host(const zg_g2_affine& q, const Fe& t, zg_g2_affine* out) {
    G2 g;
    std::memcpy(&g.x, &q.x, sizeof(Fq2));
    std::memcpy(&g.y, &q.y, sizeof(Fq2));
    if (!fq_canonical(g.x.c0) || !fq_canonical(g.x.c1) || !fq_canonical(g.y.c0) || !fq_canonical(g.y.c1))
        return "a coordinate is not below q";
    g.inf = f2_is_zero(g.x) && f2_is_zero(g.y);
    if (!g.inf) {
        const Fq2 xi = {Fq::from_u64(9), Fq::one()};
        const Fq2 b = f2_mul_fq(f2_inv(xi), Fq::from_u64(3));
        if (!f2_eq(f2_sqr(g.y), f2_add(f2_mul(f2_sqr(g.x), g.x), b))) return "not on the twist y^2 = x^3 + 3/(9+u)";
    }
    const Fe e = Fr::to_raw(t);
    G2 acc = {f2_zero(), f2_zero(), true};
    for (int i = 7; i >= 0; i--)
        for (int bit = 31; bit >= 0; bit--) {
            acc = g2_dbl(acc);
            if ((e.l[i] >> bit) & 1) acc = g2_add(acc, g);
        }
    if (acc.inf) acc.x = acc.y = f2_zero();
    std::memcpy(&out->x, &acc.x, sizeof(Fq2));
    std::memcpy(&out->y, &acc.y, sizeof(Fq2));
    return nullptr;
}

// bn256::G2Affine::generator()
zg_g2_affine g2_generator() {
    static const uint32_t RAW[4][8] = {
        {0xd992f6ed, 0x46debd5c, 0xf75edadd, 0x674322d4, 0x5e5c4479, 0x426a0066, 0x121f1e76, 0x1800deef},   // x.c0
        {0xaef312c2, 0x97e485b7, 0x35a9e712, 0xf1aa4933, 0x31fb5d25, 0x7260bfb7, 0x920d483a, 0x198e9393},   // x.c1
        {0x66fa7daa, 0x4ce6cc01, 0x0c43d37b, 0xe3d1e769, 0x8dcb408f, 0x4aab7180, 0xdb8c6deb, 0x12c85ea5},   // y.c0
        {0xd122975b, 0x55acdadc, 0x70b38ef3, 0xbc4b3133, 0x690c3395, 0xec9e99ad, 0x585ff075, 0x090689d0}};  // y.c1
    Fe m[4];
    for (int c = 0; c < 4; c++) {
        Fe r;
        for (int j = 0; j < 8; j++) r.l[j] = RAW[c][j];
        m[c] = Fq::from_raw(r);
    }
    zg_g2_affine o;
    std::memcpy(&o.x, &m[0], 2 * sizeof(Fe));
    std::memcpy(&o.y, &m[2], 2 * sizeof(Fe));
    return o;
}

}  // namespace zg

static bool fr_scalar_canonical(const zg_fr* t) {
    zg::Fe v;
    std::memcpy(&v, t, sizeof v);
    for (int i = 7; i >= 0; i--) {
        if (v.l[i] < zg::FrParams::p(i)) return true;
        if (v.l[i] > zg::FrParams::p(i)) return false;
    }
    return false;
}

extern "C" int zg_g2_mul(const zg_g2_affine* q, const zg_fr* t, zg_g2_affine* out) {
    ZG_REQUIRE(q && t && out, ZG_ERR_INVALID_ARG, "zg_g2_mul: null argument");
    ZG_REQUIRE(fr_scalar_canonical(t), ZG_ERR_INVALID_ARG, "zg_g2_mul: the scalar's limbs are not below r");
    zg::Fe tv;
    std::memcpy(&tv, t, sizeof tv);
    zg_g2_affine r;
    const char* why = zg::g2_mul_host(*q, tv, &r);
    ZG_REQUIRE(!why, ZG_ERR_INVALID_ARG, "zg_g2_mul: q: %s", why);
    *out = r;
    return ZG_OK;
}

extern "C" int zg_params_g2(const zg_fr* s, zg_g2_affine* g2, zg_g2_affine* s_g2) {
    ZG_REQUIRE(s && g2 && s_g2, ZG_ERR_INVALID_ARG, "zg_params_g2: null argument");
    ZG_REQUIRE(fr_scalar_canonical(s), ZG_ERR_INVALID_ARG, "zg_params_g2: the scalar's limbs are not below r");
    const zg_g2_affine gen = zg::g2_generator();
    *g2 = gen;
    return zg_g2_mul(&gen, s, s_g2);
}

extern "C" int zg_pairing_check(const zg_g1_affine* p, const zg_g2_affine* q, size_t n, int* result) {
    ZG_REQUIRE(result && ((p && q) || n == 0), ZG_ERR_INVALID_ARG, "zg_pairing_check: null argument");
    *result = zg::pairing_product_is_one(reinterpret_cast<const zg::Affine*>(p), q, n) ? 1 : 0;
    return ZG_OK;
}
