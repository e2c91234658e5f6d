// The cleartext model on the device: Wnn::predict (/root/reference/src/wnn.rs:78-173) for a batch of images, and the
// compute-accuracy loop (src/main.rs:186-213, argmax: src/utils.rs:35-45).  Integer arithmetic throughout: the scores are
// the reference's, bit for bit.
//
// Resident tables (built once, at zg_wnn_create):
//   bloom  one word per (filter, entry) whose bit c is bloom_filters[c][f][e] -- for a given filter and hash index EVERY class
//          reads the same entry, only the filter index depends on the image; u32 words up to 32 classes, u64 beyond
//   enc    one u32 per permuted input bit, permutation and thermometer threshold folded together: (pixel << 9) | threshold,
//          stored [t][f] (bit t of filter f) so that lanes = filters read consecutive words
// Mapping: one wave per image, WNN_WAVES images per workgroup, each wave stages its image in LDS; lane l owns filters
// l, l + 64, ...: it packs its filter index, hashes it, ANDs the `hashes` table words into the mask of responding classes;
// class c's score is the popcount of the wave's ballot of bit c, kept by lane c and written with one plain store.
#include "common.h"
#include "div64.h"

using namespace zg;

namespace {

constexpr uint32_t WNN_WAVES = 4;            // images per workgroup
constexpr uint32_t WNN_MAX_PIXELS = 16384;   // WNN_WAVES images of this size fill the 64 KB of LDS a launch gets unasked
constexpr uint32_t WNN_THR_BITS = 9;         // a threshold is 0..256

struct WnnShape {
    uint32_t classes, pixels, filters, n, hashes;  // hashes: the indices that can differ from 0 (see zg_wnn_create)
    uint32_t entries, lds_stride;
    Div64 p, e;
};

template <typename Word>
__global__ __launch_bounds__(WNN_WAVES * 64) void wnn_predict_kernel(const Word* __restrict__ bloom, const uint32_t* __restrict__ enc,
                                                                      const uint8_t* __restrict__ images, uint64_t* __restrict__ scores,
                                                                      size_t count, WnnShape s) {
    extern __shared__ uint8_t lds[];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t image = (size_t)blockIdx.x * WNN_WAVES + wave;
    const bool active = image < count;
    uint8_t* px = lds + wave * s.lds_stride;
    if (active) {
        // (a wave's slice of LDS starts at a multiple of 16; an image of the batch starts wherever count * pixels puts it)
        const uint8_t* src = images + image * s.pixels;
        const uint32_t words = ((uintptr_t)src & 3) == 0 ? s.pixels / 4 : 0;
        for (uint32_t i = lane; i < words; i += 64) ((uint32_t*)px)[i] = ((const uint32_t*)src)[i];
        for (uint32_t i = words * 4 + lane; i < s.pixels; i += 64) px[i] = src[i];
    }
    __syncthreads();
    if (!active) return;  // (whole waves leave: the ballots below see full waves)

    uint32_t score = 0;   // lane c: class c
    for (uint32_t base = 0; base < s.filters; base += 64) {
        const bool owns = base + lane < s.filters;
        const uint32_t f = owns ? base + lane : 0;
        // encode_image: bit t of filter f is permuted bit f * n + t, little-endian
        uint64_t x = 0;
        for (uint32_t t = 0; t < s.n; t++) {
            const uint32_t e = enc[(size_t)t * s.filters + f];
            const uint32_t bit = (uint32_t)px[e >> WNN_THR_BITS] >= (e & ((1u << WNN_THR_BITS) - 1));
            x |= (uint64_t)bit << t;
        }
        // mish_mash_hash: x^3 mod p as exact integers -- x mod p first, then two exact modular products
        uint64_t q;
        const uint64_t xr = div_mod(x, s.p, &q);
        uint64_t h = mul_mod(mul_mod(xr, xr, s.p), xr, s.p);
        // bloom_filter_lookup: index i = (h / entries^i) mod entries, each below `entries` by construction
        const Word* row = bloom + (size_t)f * s.entries;
        Word mask = ~(Word)0;
        for (uint32_t i = 0; i < s.hashes; i++) {
            const uint64_t idx = div_mod(h, s.e, &q);
            h = q;
            mask &= row[idx];
        }
        if (!owns) mask = 0;
        for (uint32_t c = 0; c < s.classes; c++) {
            const uint32_t responding = (uint32_t)__popcll(__ballot((int)((mask >> c) & 1)));
            if (lane == c) score += responding;
        }
    }
    if (lane < s.classes) scores[image * s.classes + lane] = score;
}

// utils.rs:35-45 argmax: the first index of the strict maximum, 0 when every score is 0
__global__ __launch_bounds__(256) void wnn_accuracy_kernel(const uint64_t* __restrict__ scores, const uint32_t* __restrict__ labels,
                                                           size_t count, uint32_t classes, uint32_t* __restrict__ predictions,
                                                           unsigned long long* __restrict__ correct,
                                                           unsigned long long* __restrict__ confusion) {
    const size_t image = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = image < count;
    uint32_t index = 0, label = 0;
    if (active) {
        uint64_t max = 0;
        for (uint32_t c = 0; c < classes; c++) {
            const uint64_t v = scores[image * classes + c];
            if (v > max) { max = v; index = c; }
        }
        label = labels[image];  // < classes: checked by the host
        predictions[image] = index;
        atomicAdd(&confusion[(size_t)label * classes + index], 1ull);
    }
    const uint32_t hits = (uint32_t)__popcll(__ballot(active && index == label));
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(correct, (unsigned long long)hits);
}

}  // namespace

struct zg_wnn {
    zg_ctx* ctx = nullptr;
    WnnShape shape{};
    void* bloom = nullptr;      // [filters][entries] u32 (classes <= 32) or u64
    uint32_t* enc = nullptr;    // [n][filters]
};

namespace {

int predict_launch(zg_wnn* m, const uint8_t* d_images, size_t count, uint64_t* d_scores) {
    zg_ctx* ctx = m->ctx;
    const WnnShape& s = m->shape;
    const dim3 grid((uint32_t)((count + WNN_WAVES - 1) / WNN_WAVES)), block(WNN_WAVES * 64);
    const size_t lds = (size_t)WNN_WAVES * s.lds_stride;
    // algorithmic bytes: the images in, the scores out (the tables stay in cache across the batch)
    const double bytes = (double)count * ((double)s.pixels + 8.0 * s.classes);
    if (s.classes <= 32)
        ZG_LAUNCH(ctx, "wnn_predict", bytes, wnn_predict_kernel<uint32_t>, grid, block, lds, (const uint32_t*)m->bloom, m->enc, d_images,
                  d_scores, count, s);
    else
        ZG_LAUNCH(ctx, "wnn_predict", bytes, wnn_predict_kernel<uint64_t>, grid, block, lds, (const uint64_t*)m->bloom, m->enc, d_images,
                  d_scores, count, s);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

constexpr size_t WNN_MAX_COUNT = (size_t)1 << 31;  // (the grid is count / WNN_WAVES workgroups)

}  // namespace

extern "C" {

int zg_wnn_create(zg_ctx* ctx, uint32_t num_classes, uint32_t width, uint32_t height, uint32_t bits_per_input,
                  uint32_t num_filter_inputs, uint32_t num_filter_entries, uint32_t num_filter_hashes, uint64_t p,
                  const uint8_t* bloom_filters, const uint64_t* input_permutation, const uint16_t* thresholds, zg_wnn** out) {
    ZG_REQUIRE(ctx != nullptr, ZG_ERR_INVALID_ARG, "zg_wnn_create: ctx is null");
    ZG_REQUIRE(out != nullptr, ZG_ERR_INVALID_ARG, "zg_wnn_create: out is null");
    ZG_REQUIRE(bloom_filters != nullptr, ZG_ERR_INVALID_ARG, "zg_wnn_create: bloom_filters is null");
    ZG_REQUIRE(input_permutation != nullptr, ZG_ERR_INVALID_ARG, "zg_wnn_create: input_permutation is null");
    ZG_REQUIRE(thresholds != nullptr, ZG_ERR_INVALID_ARG, "zg_wnn_create: thresholds is null");
    ZG_REQUIRE(num_classes && width && height && bits_per_input && num_filter_entries && num_filter_hashes && p, ZG_ERR_INVALID_ARG,
               "zg_wnn_create: a zero among classes %u, width %u, height %u, bits_per_input %u, entries %u, hashes %u, p %llu", num_classes,
               width, height, bits_per_input, num_filter_entries, num_filter_hashes, (unsigned long long)p);
    ZG_REQUIRE(num_filter_inputs >= 1 && num_filter_inputs <= 64, ZG_ERR_INVALID_ARG,
               "zg_wnn_create: %u inputs per filter (a filter index is 1..64 bits)", num_filter_inputs);
    ZG_REQUIRE(num_classes <= 64, ZG_ERR_UNSUPPORTED, "zg_wnn_create: %u classes (64 at most: one table word holds every class)", num_classes);
    const uint64_t pixels = (uint64_t)width * height;
    ZG_REQUIRE(pixels <= WNN_MAX_PIXELS, ZG_ERR_UNSUPPORTED, "zg_wnn_create: images of %u x %u pixels (%u at most: the image is staged in LDS)",
               width, height, WNN_MAX_PIXELS);
    const uint64_t bits = pixels * bits_per_input;
    ZG_REQUIRE(bits < (1ull << 31), ZG_ERR_UNSUPPORTED, "zg_wnn_create: %llu input bits", (unsigned long long)bits);
    const uint64_t filters = bits / num_filter_inputs;  // chunks_exact: a trailing partial chunk is dropped
    ZG_REQUIRE(filters >= 1, ZG_ERR_INVALID_ARG, "zg_wnn_create: %llu input bits make no filter of %u inputs", (unsigned long long)bits,
               num_filter_inputs);
    for (uint64_t t = 0; t < bits; t++)
        ZG_REQUIRE(input_permutation[t] < bits, ZG_ERR_INVALID_ARG, "zg_wnn_create: input_permutation[%llu] = %llu of %llu bits",
                   (unsigned long long)t, (unsigned long long)input_permutation[t], (unsigned long long)bits);
    for (uint64_t t = 0; t < bits; t++)
        ZG_REQUIRE(thresholds[t] <= 256, ZG_ERR_INVALID_ARG, "zg_wnn_create: threshold %llu is %u (0..256)", (unsigned long long)t, thresholds[t]);
    ZG_ENTER(ctx);

    const uint32_t n = num_filter_inputs;
    const uint64_t words = filters * num_filter_entries;
    ZG_REQUIRE(words < (1ull << 32), ZG_ERR_UNSUPPORTED, "zg_wnn_create: a table of %llu x %u entries (2^32 at most)",
               (unsigned long long)filters, num_filter_entries);
    const bool wide = num_classes > 32;
    std::vector<uint32_t> enc;
    std::vector<uint32_t> bloom32;
    std::vector<uint64_t> bloom64;
    zg_wnn* m = nullptr;
    try {
        enc.resize((size_t)n * filters);
        if (wide) bloom64.resize(words); else bloom32.resize(words);
        m = new zg_wnn();
    } catch (const std::exception&) {  // (nothing throws across the ABI)
        set_error("zg_wnn_create: no host memory for a table of %llu words", (unsigned long long)words);
        return ZG_ERR_OOM;
    }
    for (uint64_t f = 0; f < filters; f++)
        for (uint32_t t = 0; t < n; t++) {
            const uint64_t src = input_permutation[f * n + t];  // thermometer bit (b, i, j) = b * W * H + i * H + j
            const uint64_t b = src / pixels, pixel = src % pixels;
            enc[(size_t)t * filters + f] = (uint32_t)(pixel << WNN_THR_BITS) | thresholds[pixel * bits_per_input + b];
        }
    for (uint32_t c = 0; c < num_classes; c++) {
        const uint8_t* src = bloom_filters + (size_t)c * words;
        if (wide) { for (uint64_t i = 0; i < words; i++) bloom64[i] |= (uint64_t)(src[i] != 0) << c; }
        else { for (uint64_t i = 0; i < words; i++) bloom32[i] |= (uint32_t)(src[i] != 0) << c; }
    }

    m->ctx = ctx;
    WnnShape& s = m->shape;
    s.classes = num_classes; s.pixels = (uint32_t)pixels; s.filters = (uint32_t)filters; s.n = n;
    s.entries = num_filter_entries;
    s.lds_stride = ((uint32_t)pixels + 15) & ~15u;
    s.p = make_div(p);
    s.e = make_div(num_filter_entries);
    // h < 2^64 is 0 after 64 divisions by entries >= 2, and with one entry every index is 0: the indices past those are 0,
    // which the AND has seen already -- the same function for any num_filter_hashes, in a bounded loop
    s.hashes = num_filter_entries == 1 ? 1 : (num_filter_hashes < 65 ? num_filter_hashes : 65);
    const size_t bloom_bytes = (size_t)words * (wide ? 8 : 4), enc_bytes = enc.size() * 4;
    if (hipMalloc(&m->bloom, bloom_bytes) != hipSuccess || hipMalloc((void**)&m->enc, enc_bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("zg_wnn_create: no device memory for the tables (%zu + %zu bytes)", bloom_bytes, enc_bytes);
        zg_wnn_destroy(m);
        return ZG_ERR_OOM;
    }
    if (hipMemcpy(m->bloom, wide ? (const void*)bloom64.data() : (const void*)bloom32.data(), bloom_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->enc, enc.data(), enc_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("zg_wnn_create: the upload of the tables failed: %s", hipGetErrorString(hipGetLastError()));
        zg_wnn_destroy(m);
        return ZG_ERR_HIP;
    }
    *out = m;
    return ZG_OK;
}

void zg_wnn_destroy(zg_wnn* m) {
    if (!m) return;
    {
        std::lock_guard<std::recursive_mutex> lock(m->ctx->mu);
        (void)hipSetDevice(m->ctx->device);
        (void)hipStreamSynchronize(m->ctx->stream);
        if (m->bloom) (void)hipFree(m->bloom);
        if (m->enc) (void)hipFree(m->enc);
    }
    delete m;
}

int zg_wnn_predict_dev(zg_wnn* m, const void* d_images, size_t count, void* d_scores) {
    ZG_REQUIRE(m != nullptr, ZG_ERR_INVALID_ARG, "zg_wnn_predict_dev: model is null");
    if (count == 0) return ZG_OK;
    ZG_REQUIRE(d_images && d_scores, ZG_ERR_INVALID_ARG, "zg_wnn_predict_dev: null argument");
    ZG_REQUIRE(count <= WNN_MAX_COUNT, ZG_ERR_UNSUPPORTED, "zg_wnn_predict_dev: %zu images in one call", count);
    ZG_ENTER(m->ctx);
    return predict_launch(m, (const uint8_t*)d_images, count, (uint64_t*)d_scores);
}

int zg_wnn_predict(zg_wnn* m, const uint8_t* images, size_t count, uint64_t* scores) {
    ZG_REQUIRE(m != nullptr, ZG_ERR_INVALID_ARG, "zg_wnn_predict: model is null");
    if (count == 0) return ZG_OK;
    ZG_REQUIRE(images && scores, ZG_ERR_INVALID_ARG, "zg_wnn_predict: null argument");
    ZG_REQUIRE(count <= WNN_MAX_COUNT, ZG_ERR_UNSUPPORTED, "zg_wnn_predict: %zu images in one call", count);
    zg_ctx* ctx = m->ctx;
    ZG_ENTER(ctx);
    const WnnShape& s = m->shape;
    WsScope ws(ctx);
    uint8_t* d_images = ws.get<uint8_t>(count * s.pixels);
    uint64_t* d_scores = ws.get<uint64_t>(count * s.classes);
    if (ws.failed) return ZG_ERR_OOM;
    ZG_HIP(hipMemcpyAsync(d_images, images, count * s.pixels, hipMemcpyHostToDevice, ctx->stream));
    ZG_TRY(predict_launch(m, d_images, count, d_scores));
    ZG_HIP(hipMemcpyAsync(scores, d_scores, count * s.classes * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    return ZG_OK;
}

int zg_wnn_accuracy(zg_wnn* m, const uint8_t* images, const uint32_t* labels, size_t count, uint32_t* predictions, uint64_t* correct,
                    uint64_t* confusion) {
    ZG_REQUIRE(m != nullptr, ZG_ERR_INVALID_ARG, "zg_wnn_accuracy: model is null");
    ZG_REQUIRE(correct != nullptr && (count == 0 || (images && labels)), ZG_ERR_INVALID_ARG, "zg_wnn_accuracy: null argument");
    ZG_REQUIRE(count <= WNN_MAX_COUNT, ZG_ERR_UNSUPPORTED, "zg_wnn_accuracy: %zu images in one call", count);
    const WnnShape& s = m->shape;
    for (size_t i = 0; i < count; i++)
        ZG_REQUIRE(labels[i] < s.classes, ZG_ERR_INVALID_ARG, "zg_wnn_accuracy: label %zu is %u of %u classes", i, labels[i], s.classes);
    const size_t cells = (size_t)s.classes * s.classes;
    *correct = 0;
    if (confusion) memset(confusion, 0, cells * sizeof(uint64_t));
    if (count == 0) return ZG_OK;
    zg_ctx* ctx = m->ctx;
    ZG_ENTER(ctx);
    WsScope ws(ctx);
    uint8_t* d_images = ws.get<uint8_t>(count * s.pixels);
    uint64_t* d_scores = ws.get<uint64_t>(count * s.classes);
    uint32_t* d_labels = ws.get<uint32_t>(count);
    uint32_t* d_pred = ws.get<uint32_t>(count);
    unsigned long long* d_counts = ws.get<unsigned long long>(1 + cells);  // correct, then the confusion matrix
    if (ws.failed) return ZG_ERR_OOM;
    ZG_HIP(hipMemcpyAsync(d_images, images, count * s.pixels, hipMemcpyHostToDevice, ctx->stream));
    ZG_HIP(hipMemcpyAsync(d_labels, labels, count * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    ZG_HIP(hipMemsetAsync(d_counts, 0, (1 + cells) * sizeof(unsigned long long), ctx->stream));
    ZG_TRY(predict_launch(m, d_images, count, d_scores));
    ZG_LAUNCH(ctx, "wnn_accuracy", (double)count * (8.0 * s.classes + 8.0), wnn_accuracy_kernel, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0,
              d_scores, d_labels, count, s.classes, d_pred, d_counts, d_counts + 1);
    ZG_HIP(hipGetLastError());
    std::vector<unsigned long long> counts(1 + cells);
    ZG_HIP(hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (predictions) ZG_HIP(hipMemcpyAsync(predictions, d_pred, count * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    ZG_HIP(hipStreamSynchronize(ctx->stream));
    *correct = counts[0];
    if (confusion)
        for (size_t i = 0; i < cells; i++) confusion[i] = counts[1 + i];
    return ZG_OK;
}

}  // extern "C"
