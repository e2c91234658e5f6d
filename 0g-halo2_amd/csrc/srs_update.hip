// One contribution to an updatable KZG reference string, and its check.
//
// zg_params_new makes an SRS from a scalar its caller knows.  An SRS nobody knows the scalar of is made in steps: each
// party multiplies the string it was given by a secret t of its own,
//     g'[i] = t^i g[i],   s_g2' = t s_g2,   g2 unchanged      (the string of s becomes the string of s t)
// and publishes (t g[0], t g2) beside it.  The result is sound if ONE party forgot its t.  The step is n independent
// variable-base multiplications (g1_mul.hip) by powers made on the device; g_lagrange follows through the G1 transform
// of g1_fft.hip and never visits the host; the two G2 products and the pairings of the check run on the host
// (pairing.hip).  upstream has no counterpart: halo2_proofs v2023_04_20 only has ParamsKZG::setup (one party).
#include "poly.h"

namespace zg {

int g1_mul_each_dev(zg_ctx* ctx, const Affine* d_points, const Fe* d_scalars, size_t n, Affine* d_out);
int g1_lagrange_dev(zg_ctx* ctx, uint32_t k, const Affine* d_g, Affine* d_gl);
bool pairing_product_is_one(const Affine* p, const zg_g2_affine* q, size_t n);
const char* g2_point_fault(const zg_g2_affine& q);
const char* g2_mul_host(const zg_g2_affine& q, const Fe& t, zg_g2_affine* out);

namespace {

// out[i] = t^i, i < n
__global__ void srs_powers_kernel(Fe* __restrict__ out, Fe t, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = Fr::pow_u64(t, i);
}

template <class P>
bool limbs_below(const Fe& v) {
    for (int i = 7; i >= 0; i--) {
        if (v.l[i] < P::p(i)) return true;
        if (v.l[i] > P::p(i)) return false;
    }
    return false;
}

// a secret a contribution may use: limbs below r, not zero
bool update_scalar_ok(const zg_fr* t, Fe* out) {
    memcpy(out, t, sizeof(Fe));
    return limbs_below<FrParams>(*out) && !fe_is_zero(*out);
}

// canonical coordinates, on the curve, not the identity
bool g1_point_ok(const Affine& p) {
    return limbs_below<FqParams>(p.x) && limbs_below<FqParams>(p.y) && !affine_is_identity(p) && affine_on_curve(p);
}

// d_pw: room for n + 1 scalars; leaves t^0 .. t^n there and the updated points in d_g_out.  The caller zeroes d_pw.
int update_points_dev(zg_ctx* ctx, uint32_t k, const Fe& t, const Affine* d_g, Affine* d_g_out, Affine* d_gl_out, Fe* d_pw) {
    const uint32_t n = 1u << k;
    ZG_LAUNCH(ctx, "srs_powers", (double)(n + 1) * 32, srs_powers_kernel, dim3((n + 1 + 63) / 64), dim3(64), 0, d_pw, t, n + 1);
    ZG_HIP(hipGetLastError());
    ZG_TRY(g1_mul_each_dev(ctx, d_g, d_pw, n, d_g_out));
    if (d_gl_out) ZG_TRY(g1_lagrange_dev(ctx, k, d_g_out, d_gl_out));
    return ZG_OK;
}

}  // namespace
}  // namespace zg

using namespace zg;

extern "C" int zg_params_update_dev(zg_ctx* ctx, uint32_t k, const zg_fr* t, const void* d_g, void* d_g_out,
                                    void* d_g_lagrange_out) {
    ZG_REQUIRE(ctx && t && d_g && d_g_out, ZG_ERR_INVALID_ARG, "zg_params_update_dev: null argument");
    ZG_REQUIRE(k <= 24, ZG_ERR_UNSUPPORTED, "zg_params_update_dev: k=%u > 24", k);
    ZG_REQUIRE(d_g_lagrange_out != d_g_out && d_g_lagrange_out != d_g, ZG_ERR_INVALID_ARG,
               "zg_params_update_dev: g_lagrange may not share the array of g");
    Fe tv;
    ZG_REQUIRE(update_scalar_ok(t, &tv), ZG_ERR_INVALID_ARG, "zg_params_update_dev: t is zero or its limbs are not below r");
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    const size_t n = (size_t)1 << k;
    Fe* pw = ws.get<Fe>(n + 1);
    if (ws.failed) return ZG_ERR_OOM;
    const int st = update_points_dev(ctx, k, tv, (const Affine*)d_g, (Affine*)d_g_out, (Affine*)d_g_lagrange_out, pw);
    // the powers of the secret leave the pooled block before another call can be handed it (best effort: the kernel
    // arguments, registers and LDS of the launches above are not reachable from here)
    ZG_HIP(hipMemsetAsync(pw, 0, (n + 1) * sizeof(Fe), ctx->stream));
    return st;
}

extern "C" int zg_params_update(zg_ctx* ctx, uint32_t k, const zg_fr* t, const zg_g1_affine* g, const zg_g2_affine* g2,
                                const zg_g2_affine* s_g2, zg_g1_affine* g_out, zg_g1_affine* g_lagrange_out,
                                zg_g2_affine* s_g2_out, zg_srs_contribution* record) {
    ZG_REQUIRE(ctx && t && g && g2 && s_g2 && g_out && s_g2_out && record, ZG_ERR_INVALID_ARG, "zg_params_update: null argument");
    ZG_REQUIRE(k <= 24, ZG_ERR_UNSUPPORTED, "zg_params_update: k=%u > 24", k);
    Fe tv;
    ZG_REQUIRE(update_scalar_ok(t, &tv), ZG_ERR_INVALID_ARG, "zg_params_update: t is zero or its limbs are not below r");
    // the G2 half first, into temporaries: a refused point leaves every output as it was
    zg_g2_affine new_s_g2, t_g2;
    const char* why = g2_mul_host(*s_g2, tv, &new_s_g2);
    ZG_REQUIRE(!why, ZG_ERR_INVALID_ARG, "zg_params_update: s_g2: %s", why);
    why = g2_mul_host(*g2, tv, &t_g2);
    ZG_REQUIRE(!why, ZG_ERR_INVALID_ARG, "zg_params_update: g2: %s", why);
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    const size_t n = (size_t)1 << k;
    Affine* dg = ws.get<Affine>(n);
    Affine* dl = g_lagrange_out ? ws.get<Affine>(n) : nullptr;
    Affine* d_rec = ws.get<Affine>(1);
    Fe* pw = ws.get<Fe>(n + 1);
    if (ws.failed) return ZG_ERR_OOM;
    hipStream_t st = ctx->stream;
    Affine t_g1;
    ZG_HIP(hipMemcpyAsync(dg, g, n * sizeof(Affine), hipMemcpyHostToDevice, st));
    int status = update_points_dev(ctx, k, tv, dg, dg, nullptr, pw);
    // t g[0]: pw[1] = t, and g[0] is its own update (t^0 = 1)
    if (status == ZG_OK) status = g1_mul_each_dev(ctx, dg, pw + 1, 1, d_rec);
    ZG_HIP(hipMemsetAsync(pw, 0, (n + 1) * sizeof(Fe), st));  // (best effort, see zg_params_update_dev)
    if (status == ZG_OK && dl) status = g1_lagrange_dev(ctx, k, dg, dl);
    if (status != ZG_OK) {
        (void)hipStreamSynchronize(st);  // the blocks go back to the pool idle
        return status;
    }
    ZG_HIP(hipMemcpyAsync(g_out, dg, n * sizeof(Affine), hipMemcpyDeviceToHost, st));
    if (dl) ZG_HIP(hipMemcpyAsync(g_lagrange_out, dl, n * sizeof(Affine), hipMemcpyDeviceToHost, st));
    ZG_HIP(hipMemcpyAsync(&t_g1, d_rec, sizeof(Affine), hipMemcpyDeviceToHost, st));
    ZG_HIP(hipStreamSynchronize(st));
    *s_g2_out = new_s_g2;
    memcpy(&record->t_g1, &t_g1, sizeof(Affine));
    record->t_g2 = t_g2;
    return ZG_OK;
}

extern "C" int zg_params_check_update(zg_ctx* ctx, uint32_t k, const zg_g1_affine prev_g01[2], const zg_g1_affine* g_next,
                                      const zg_g1_affine* g_lagrange_next, const zg_g2_affine* g2,
                                      const zg_g2_affine* s_g2_next, const zg_srs_contribution* record,
                                      const uint8_t key[32], int* verdict, uint32_t* failed) {
    ZG_REQUIRE(ctx && prev_g01 && g_next && g2 && s_g2_next && record && key && verdict && failed, ZG_ERR_INVALID_ARG,
               "zg_params_check_update: null argument");
    ZG_REQUIRE(k >= 1, ZG_ERR_INVALID_ARG, "zg_params_check_update: k = 0 has no g[1] to link the step by");
    *verdict = 0;
    *failed = 0;
    // (a) the new string is a structured reference string: zg_params_check itself, same bits
    int v = 0;
    uint32_t bits = 0;
    ZG_TRY(zg_params_check(ctx, k, g_next, g_lagrange_next, g2, s_g2_next, key, &v, &bits));
    Affine prev[2], next[2], t_g1;
    memcpy(prev, prev_g01, sizeof prev);
    memcpy(next, g_next, sizeof next);
    memcpy(&t_g1, &record->t_g1, sizeof t_g1);
    // (b) the step kept the base point
    if (memcmp(&prev[0], &next[0], sizeof(Affine)) != 0) bits |= ZG_SRS_UPDATE_BASE;
    // (c) the step multiplied by the t of the record: e(t_g1, g2) = e(prev g[0], t_g2) ties the two halves of the record
    // to ONE t, and e(g_next[1], g2) = e(prev g[1], t_g2) says that g_next[1] is t times prev g[1]
    const char* why = nullptr;
    if (const char* w2 = g2_point_fault(record->t_g2)) why = w2;
    else if (g2_point_fault(*g2)) why = "g2 is no point to pair against";
    else if (!g1_point_ok(t_g1)) why = "t_g1 is non-canonical, off the curve or the identity";
    else if (!g1_point_ok(prev[0]) || !g1_point_ok(prev[1]) || !g1_point_ok(next[1]))
        why = "g[0] or g[1] is non-canonical, off the curve or the identity";
    else {
        const zg_g2_affine qs[2] = {*g2, record->t_g2};
        const Affine rec[2] = {t_g1, affine_neg(prev[0])};
        const Affine lnk[2] = {next[1], affine_neg(prev[1])};
        if (!pairing_product_is_one(rec, qs, 2)) why = "t_g1 and t_g2 are not the same multiple of g[0] and g2";
        else if (!pairing_product_is_one(lnk, qs, 2)) why = "g_next[1] is not t times the previous g[1]";
    }
    if (why) bits |= ZG_SRS_UPDATE_LINK;
    *failed = bits;
    *verdict = bits == 0;
    if (bits & ZG_SRS_UPDATE_BASE) set_error("zg_params_check_update: g_next[0] is not the previous g[0]");
    else if (why) set_error("zg_params_check_update: %s", why);
    return ZG_OK;
}
