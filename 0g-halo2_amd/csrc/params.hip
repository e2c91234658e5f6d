// KZG structured reference string on the GPU -- replaces ParamsKZG::<Bn256>::new(k)
// (halo2_proofs v2023_04_20 src/poly/kzg/commitment.rs `ParamsKZG::setup`; reference call sites
// /root/reference/benches/bench.rs:19 and src/main.rs:232).  Upstream draws the toxic scalar s from
// OsRng; here the caller passes it so that runs are reproducible.
//   g[i]          = s^i * G
//   g_lagrange[i] = L_i(s) * G,  L_i(s) = (s^n - 1)/n * omega^i / (s - omega^i)
// One lane per point: 254-step double-and-add in XYZZ, one Fermat inversion to go affine.  This is a
// one-off (outside the timed region of the reference's bench, benches/bench.rs:30-36).
//
// zg_params_check is the other side: a caller who was GIVEN g, g_lagrange, g2 and s_g2 (a ceremony's output, one large
// file shared by all models) and not s asks whether they are a structured reference string at all.  Upstream has no
// counterpart (ParamsKZG::read trusts the file); the relations checked are the ones ParamsKZG::setup establishes:
//   points    every coordinate canonical, every point on its curve, no identity among g, g2 and s_g2 in the r-torsion;
//   powers    g[i+1] = s g[i]:  with random r_i, A = sum r_i g[i], B = sum r_i g[i+1] -- two scalar vectors, one the
//             other shifted by one, against ONE base set in one MSM batch -- and e(B, g2) e(-A, s_g2) = 1;
//   lagrange  g_lagrange = g_to_lagrange(g):  for a random polynomial c, sum_j c_j g[j] = c(s) G = sum_i c(omega^i)
//             g_lagrange[i] -- one more vector of that batch, one NTT, one MSM against g_lagrange.
// A wrong file passes a relation with the probability that a fixed non-zero linear form vanishes on random scalars
// the file's maker did not know: ~2^-254.
#include "poly.h"

namespace zg {

bool pairing_product_is_one(const Affine* p, const zg_g2_affine* q, size_t n);
const char* g2_point_fault(const zg_g2_affine& q);

__device__ __forceinline__ void st_affine(Affine* p, const Affine& v) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(v.x.l[0], v.x.l[1], v.x.l[2], v.x.l[3]);
    q[1] = make_uint4(v.x.l[4], v.x.l[5], v.x.l[6], v.x.l[7]);
    q[2] = make_uint4(v.y.l[0], v.y.l[1], v.y.l[2], v.y.l[3]);
    q[3] = make_uint4(v.y.l[4], v.y.l[5], v.y.l[6], v.y.l[7]);
}

__global__ void srs_kernel(Affine* __restrict__ g, Affine* __restrict__ gl, Fe s, Fe omega, Fe mult,
                           uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine gen;
    gen.x = Fq::from_u64(1);
    gen.y = Fq::from_u64(2);
    Fe si = Fr::pow_u64(s, i);
    Fe raw = Fr::to_raw(si);
    st_affine(g + i, xyzz_to_affine(xyzz_mul_raw(gen, raw.l)));
    Fe wi = Fr::pow_u64(omega, i);
    Fe li = Fr::mul(Fr::mul(mult, wi), Fr::inv(Fr::sub(s, wi)));
    raw = Fr::to_raw(li);
    st_affine(gl + i, xyzz_to_affine(xyzz_mul_raw(gen, raw.l)));
}

// first[0] = lowest i with g[i] malformed (a coordinate not below q, or off y^2 = x^3 + 3), first[1] = lowest i with
// g[i] the identity, first[2] = lowest i with g_lagrange[i] malformed (its identities are points); untouched when none
__global__ void srs_points_kernel(const Affine* __restrict__ g, const Affine* __restrict__ gl, uint32_t n, uint32_t* first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto malformed = [](const Affine& p) {
        bool below = true;
        for (int c = 0; c < 2; c++) {
            const Fe& v = c ? p.y : p.x;
            bool lt = false;
            for (int j = 7; j >= 0; j--) {
                if (v.l[j] < FqParams::p(j)) { lt = true; break; }
                if (v.l[j] > FqParams::p(j)) break;
            }
            below = below && lt;
        }
        return !below || !affine_on_curve(p);
    };
    const Affine p = g[i];
    if (malformed(p)) atomicMin(first + 0, i);
    else if (affine_is_identity(p)) atomicMin(first + 1, i);
    if (gl && malformed(gl[i])) atomicMin(first + 2, i);
}

namespace {
struct BasesGuard {  // a base set that lives for one call
    zg_bases* b = nullptr;
    ~BasesGuard() { zg_bases_free(b); }
};
}  // namespace

}  // namespace zg

using namespace zg;

extern "C" int zg_params_check(zg_ctx* ctx, uint32_t k, const zg_g1_affine* g, const zg_g1_affine* g_lagrange,
                               const zg_g2_affine* g2, const zg_g2_affine* s_g2, const uint8_t key[32], int* verdict,
                               uint32_t* failed) {
    ZG_REQUIRE(ctx && g && g2 && s_g2 && key && verdict && failed, ZG_ERR_INVALID_ARG, "zg_params_check: null argument");
    ZG_REQUIRE(k <= 22, ZG_ERR_UNSUPPORTED, "zg_params_check: k=%u > 22", k);
    *verdict = 0;
    *failed = 0;
    uint32_t bits = 0;
    const char* what2 = g2_point_fault(*g2);
    const char* whats = g2_point_fault(*s_g2);
    if (what2 || whats) bits |= ZG_SRS_G2;
    const uint32_t n = 1u << k;
    uint32_t first[3];
    XYZZ sums[4];  // A, B, C (against g), D (against g_lagrange)
    for (XYZZ& s : sums) s = xyzz_identity();
    {
        // the device part holds the context; the host pairing below does not
        ZG_ENTER(ctx);
        WsScope ws(ctx);
        Affine* dg = ws.get<Affine>(n);
        Affine* dl = g_lagrange ? ws.get<Affine>(n) : nullptr;
        uint32_t* d_first = ws.get<uint32_t>(4);
        Fe* sc = ws.get<Fe>((size_t)4 * n);  // r (ends in 0) | r shifted by one (starts with 0) | c | evaluations of c
        XYZZ* d_sums = ws.get<XYZZ>(4);
        if (ws.failed) return ZG_ERR_OOM;
        hipStream_t st = ctx->stream;
        ZG_HIP(hipMemcpyAsync(dg, g, (size_t)n * sizeof(Affine), hipMemcpyHostToDevice, st));
        if (dl) ZG_HIP(hipMemcpyAsync(dl, g_lagrange, (size_t)n * sizeof(Affine), hipMemcpyHostToDevice, st));
        ZG_HIP(hipMemsetAsync(d_first, 0xff, 4 * sizeof(uint32_t), st));
        ZG_LAUNCH(ctx, "srs_points", (double)n * (dl ? 128 : 64), srs_points_kernel, dim3((n + 63) / 64), dim3(64), 0, dg, dl, n,
                  d_first);
        ZG_HIP(hipGetLastError());
        ZG_HIP(hipMemcpyAsync(first, d_first, sizeof(first), hipMemcpyDeviceToHost, st));
        ZG_HIP(hipStreamSynchronize(st));
        if (first[0] != 0xffffffffu || first[2] != 0xffffffffu) bits |= ZG_SRS_G1_MALFORMED;
        if (first[1] != 0xffffffffu) bits |= ZG_SRS_G1_IDENTITY;
        if (bits) {
            *failed = bits;
            if (first[0] != 0xffffffffu)
                set_error("zg_params_check: g[%u] has a coordinate not below q or is off y^2 = x^3 + 3", first[0]);
            else if (first[2] != 0xffffffffu)
                set_error("zg_params_check: g_lagrange[%u] has a coordinate not below q or is off y^2 = x^3 + 3", first[2]);
            else if (first[1] != 0xffffffffu)
                set_error("zg_params_check: g[%u] is the identity", first[1]);
            else
                set_error("zg_params_check: %s is %s", what2 ? "g2" : "s_g2", what2 ? what2 : whats);
            return ZG_OK;
        }
        uint32_t kw[8];
        memcpy(kw, key, 32);
        const bool powers = k > 0;
        if (powers) {
            ZG_TRY(poly_rand_fill(ctx, kw, TAG_SRS_POWERS, sc, n - 1));
            ZG_HIP(hipMemsetAsync(sc + (n - 1), 0, sizeof(Fe), st));
            ZG_HIP(hipMemsetAsync(sc + n, 0, sizeof(Fe), st));
            ZG_HIP(hipMemcpyAsync(sc + n + 1, sc, (size_t)(n - 1) * sizeof(Fe), hipMemcpyDeviceToDevice, st));
        }
        if (dl) ZG_TRY(poly_rand_fill(ctx, kw, TAG_SRS_LAGRANGE, sc + (size_t)2 * n, n));
        const size_t v0 = powers ? 0 : 2, v1 = dl ? 3 : 2;  // the vectors multiplied against g
        if (v1 > v0) {
            BasesGuard bg;
            ZG_TRY(bases_register_dev(ctx, dg, n, 0, &bg.b));
            MsmJob j;
            j.bases = bg.b; j.split = v1 - v0;
            j.scalars = sc + v0 * n; j.stride = n;
            j.batch = v1 - v0; j.n = n;
            j.out = d_sums + v0;
            ZG_TRY(msm_dev(ctx, j));
            ZG_HIP(hipStreamSynchronize(st));  // (the guard frees the tables)
        }
        if (dl) {
            Fe* ev = sc + (size_t)3 * n;
            if (k > 0) ZG_TRY(ntt_batch_to_dev(ctx, sc + (size_t)2 * n, ev, n, 1, k, host_domain_omega(k), nullptr));
            else ZG_HIP(hipMemcpyAsync(ev, sc + (size_t)2 * n, sizeof(Fe), hipMemcpyDeviceToDevice, st));
            BasesGuard bl;
            ZG_TRY(bases_register_dev(ctx, dl, n, 0, &bl.b));
            MsmJob j;
            j.bases = bl.b; j.split = 1;
            j.scalars = ev; j.stride = n;
            j.batch = 1; j.n = n;
            j.out = d_sums + 3;
            ZG_TRY(msm_dev(ctx, j));
            ZG_HIP(hipStreamSynchronize(st));
        }
        for (size_t v = v0; v < v1; v++)
            ZG_HIP(hipMemcpyAsync(&sums[v], d_sums + v, sizeof(XYZZ), hipMemcpyDeviceToHost, st));
        if (dl) ZG_HIP(hipMemcpyAsync(&sums[3], d_sums + 3, sizeof(XYZZ), hipMemcpyDeviceToHost, st));
        ZG_HIP(hipStreamSynchronize(st));
    }
    if (k > 0) {
        const Affine ps[2] = {xyzz_to_affine(sums[1]), affine_neg(xyzz_to_affine(sums[0]))};
        const zg_g2_affine qs[2] = {*g2, *s_g2};
        // (A = B = identity would pass any s_g2: with weights nobody chose and no identity in g, probability ~2^-254)
        if (!pairing_product_is_one(ps, qs, 2)) bits |= ZG_SRS_POWERS;
    }
    if (g_lagrange) {
        const Affine c = xyzz_to_affine(sums[2]), d = xyzz_to_affine(sums[3]);
        if (!fe_eq(c.x, d.x) || !fe_eq(c.y, d.y)) bits |= ZG_SRS_LAGRANGE;
    }
    *failed = bits;
    *verdict = bits == 0;
    if (bits)
        set_error("zg_params_check:%s%s", (bits & ZG_SRS_POWERS) ? " g is no sequence of powers under s_g2" : "",
                  (bits & ZG_SRS_LAGRANGE) ? " g_lagrange is not the Lagrange basis of g" : "");
    return ZG_OK;
}

extern "C" int zg_params_new_dev(zg_ctx* ctx, uint32_t k, const zg_fr* s, void* d_g, void* d_g_lagrange) {
    ZG_REQUIRE(ctx && s && d_g && d_g_lagrange, ZG_ERR_INVALID_ARG, "zg_params_new_dev: null argument");
    ZG_REQUIRE(k <= 24, ZG_ERR_UNSUPPORTED, "zg_params_new_dev: k=%u > 24", k);
    ZG_ENTER(ctx);
    Fe sv;
    memcpy(&sv, s, 32);
    uint32_t n = 1u << k;
    Fe omega = host_domain_omega(k);
    Fe mult = Fr::mul(Fr::sub(Fr::pow_u64(sv, n), Fr::one()), Fr::inv(Fr::from_u64(n)));
    ZG_LAUNCH(ctx, "srs", 0, srs_kernel, dim3((n + 63) / 64), dim3(64), 0, (Affine*)d_g, (Affine*)d_g_lagrange,
              sv, omega, mult, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

extern "C" int zg_params_new(zg_ctx* ctx, uint32_t k, const zg_fr* s, zg_g1_affine* g, zg_g1_affine* g_lagrange) {
    ZG_REQUIRE(ctx && s && g && g_lagrange, ZG_ERR_INVALID_ARG, "zg_params_new: null argument");
    ZG_REQUIRE(k <= 24, ZG_ERR_UNSUPPORTED, "zg_params_new: k=%u > 24", k);
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    size_t n = (size_t)1 << k;
    Affine* dg = ws.get<Affine>(n);
    Affine* dl = ws.get<Affine>(n);
    if (ws.failed) return ZG_ERR_OOM;
    ZG_TRY(zg_params_new_dev(ctx, k, s, dg, dl));
    ZG_HIP(hipMemcpyAsync(g, dg, n * sizeof(Affine), hipMemcpyDeviceToHost, ctx->stream));
    ZG_HIP(hipMemcpyAsync(g_lagrange, dl, n * sizeof(Affine), hipMemcpyDeviceToHost, ctx->stream));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    return ZG_OK;
}
