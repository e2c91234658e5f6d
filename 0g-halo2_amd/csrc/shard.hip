// Point-range shards of the SRS: every rank commits against its slice of the base sets, the partial commitments of all
// ranks are exchanged and summed -- by a function of the caller's (zg_prover_set_shard) or over a communicator of the
// collective library (zg_prover_set_shard_rccl).
#include <dlfcn.h>

#include "prover.h"

using namespace zg;

// Host: out[i] = normalised sum over ranks r of the extended-Jacobian (X, Y, ZZ, ZZZ; 128 B) partial parts[r * count + i]
// -- the additions that follow the all-gather of a sharded commitment phase.
extern "C" int zg_xyzz_sum_ranks(const void* parts, size_t world, size_t count, zg_g1* out) {
    ZG_REQUIRE(out && (parts || count == 0) && world >= 1, ZG_ERR_INVALID_ARG, "zg_xyzz_sum_ranks: bad argument");
    const XYZZ* all = reinterpret_cast<const XYZZ*>(parts);
    std::vector<XYZZ> sum(count);
    for (size_t i = 0; i < count; i++) {
        XYZZ acc = all[i];
        for (size_t r = 1; r < world; r++) acc = xyzz_add(acc, all[r * count + i]);
        sum[i] = acc;
    }
    xyzz_batch_normalise(sum.data(), count, out);
    return ZG_OK;
}

namespace {

// RCCL is bound at run time (dlopen): the library has no link-time dependency on it, and only a prover that was given a
// communicator ever asks for it.
typedef int (*rccl_all_gather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static rccl_all_gather_fn rccl_all_gather() {
    static rccl_all_gather_fn fn = []() -> rccl_all_gather_fn {
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        return h ? (rccl_all_gather_fn)dlsym(h, "ncclAllGather") : nullptr;
    }();
    return fn;
}

// out[i] = sum over ranks r of parts[r * count + i] (extended Jacobian), one lane per commitment: world - 1 additions
__global__ void xyzz_sum_ranks_kernel(const XYZZ* __restrict__ parts, uint32_t world, uint32_t count, XYZZ* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    XYZZ acc = parts[i];
    for (uint32_t r = 1; r < world; r++) acc = xyzz_add(acc, parts[(size_t)r * count + i]);
    out[i] = acc;
}

// what both ways of declaring a shard ask of it (who: the entry's name)
int shard_args_ok(const char* who, const zg_prover* p, uint32_t rank, uint32_t world, size_t first_point, bool fn_missing) {
    ZG_REQUIRE(world >= 1 && rank < world, ZG_ERR_INVALID_ARG, "%s: rank %u of %u", who, rank, world);
    ZG_REQUIRE(world == 1 || !p->phased(), ZG_ERR_UNSUPPORTED, "%s: a circuit with challenges or advice phases is not proved on a point-range shard", who);
    ZG_REQUIRE(world == 1 || p->pk->NS == 0, ZG_ERR_UNSUPPORTED, "%s: a circuit with shuffles is not proved on a point-range shard", who);
    ZG_REQUIRE(!fn_missing, ZG_ERR_INVALID_ARG, "%s: no exchange function", who);
    ZG_REQUIRE(first_point + p->g->n <= p->pk->n, ZG_ERR_INVALID_ARG, "%s: points [%zu, %zu) of %u", who, first_point,
               first_point + p->g->n, p->pk->n);
    ZG_REQUIRE(world > 1 || p->g->n == p->pk->n, ZG_ERR_INVALID_ARG, "%s: a lone prover needs all 2^k points", who);
    return ZG_OK;
}
// ... and what it leaves in the prover: the rank's point range and ONE way of exchanging the partial sums
void shard_set(zg_prover* p, uint32_t rank, uint32_t world, size_t first_point, zg_exchange_fn fn, void* user, void* nccl_comm) {
    p->rank = rank;
    p->world = world;
    p->shard_lo = (uint32_t)first_point;
    p->shard_n = (uint32_t)p->g->n;
    p->exchange = fn;
    p->exchange_user = user;
    p->rccl_comm = nccl_comm;
}

}  // namespace

int zg::shard_gather_sum(zg_prover* p, size_t count, XYZZ* out) {
    rccl_all_gather_fn gather = rccl_all_gather();
    ZG_REQUIRE(gather != nullptr, ZG_ERR_UNSUPPORTED, "zg_prover: librccl.so could not be loaded");
    const int st = gather(p->xyzz, p->gathered, count * sizeof(XYZZ), /* ncclUint8 */ 1, p->rccl_comm, p->ctx->stream);
    ZG_REQUIRE(st == 0, ZG_ERR_HIP, "zg_prover: ncclAllGather failed with %d", st);
    ZG_LAUNCH(p->ctx, "xyzz_sum_ranks", (double)p->world * count * sizeof(XYZZ), xyzz_sum_ranks_kernel,
              dim3((uint32_t)((count + 63) / 64)), dim3(64), 0, p->gathered, p->world, (uint32_t)count, out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

extern "C" {

int zg_prover_set_shard(zg_prover* p, uint32_t rank, uint32_t world, size_t first_point, zg_exchange_fn fn, void* user) {
    ZG_REQUIRE(p, ZG_ERR_INVALID_ARG, "zg_prover_set_shard: null prover");
    ZG_ENTER(p->ctx);
    ZG_TRY(shard_args_ok("zg_prover_set_shard", p, rank, world, first_point, world != 1 && fn == nullptr));
    shard_set(p, rank, world, first_point, fn, user, nullptr);
    return ZG_OK;
}

int zg_xyzz_sum_ranks_dev(zg_ctx* ctx, const void* d_parts, size_t world, size_t count, void* d_out) {
    ZG_REQUIRE(ctx && d_out && (d_parts || count == 0) && world >= 1 && count < (1ull << 31), ZG_ERR_INVALID_ARG,
               "zg_xyzz_sum_ranks_dev: bad argument");
    if (count == 0) return ZG_OK;
    ZG_ENTER(ctx);
    ZG_LAUNCH(ctx, "xyzz_sum_ranks", (double)world * count * sizeof(XYZZ), xyzz_sum_ranks_kernel, dim3((uint32_t)((count + 63) / 64)),
              dim3(64), 0, (const XYZZ*)d_parts, (uint32_t)world, (uint32_t)count, (XYZZ*)d_out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int zg_prover_set_shard_rccl(zg_prover* p, uint32_t rank, uint32_t world, size_t first_point, void* nccl_comm) {
    ZG_REQUIRE(p && nccl_comm, ZG_ERR_INVALID_ARG, "zg_prover_set_shard_rccl: null argument");
    ZG_ENTER(p->ctx);
    ZG_TRY(shard_args_ok("zg_prover_set_shard_rccl", p, rank, world, first_point, false));
    ZG_REQUIRE(rccl_all_gather() != nullptr, ZG_ERR_UNSUPPORTED, "zg_prover_set_shard_rccl: librccl.so could not be loaded");
    if (p->gathered) (void)hipFree(p->gathered);
    p->gathered = nullptr;
    ZG_HIP(hipMalloc((void**)&p->gathered, (size_t)world * p->maxv * p->cap * sizeof(XYZZ)));
    p->gathered_cap = (size_t)p->cap;
    shard_set(p, rank, world, first_point, nullptr, nullptr, nccl_comm);
    return ZG_OK;
}

}  // extern "C"
