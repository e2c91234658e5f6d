// Test program (not product code): runs the primitives of csrc/field9.h and the device path of csrc/field.h on operands
// read from a file and writes back, raw, what they returned.  It holds no expected values and no case generator: the
// cases and the judge are Python integers (tests/field9_ref.py, tests/field9_cases.py).
//
// Usage: field9_probe device|host IN OUT
//   IN : records of 76 int32: op, field (0 = Fq, 1 = Fr), arg, 0, then eight operand slots of nine int32 (raw F9 limbs; the
//        8 x 32-bit ops use the first eight words of a slot; a point takes four slots: x, y, zz, zzz).
//   OUT: per record twelve result slots of nine int32 (pre-filled with 0x5a5a5a5a), then inf, wm, the is_zero_mod_p bits, 0.
// What an op reads and writes is stated at its case in run_op / the lane kernels below.  "device" launches one kernel per
// op over all records of that op; "host" runs the ops below OP_LANES (plain C++: no DPP, no fences) on the CPU.
// Every HIP status is checked; the first error ends the program with a non-zero exit.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../0g-halo2_amd/csrc/field9.h"

using namespace zg;

struct RecIn {
    int32_t op, field, arg, pad;
    F9 s[8];
};
struct RecOut {
    F9 s[12];
    int32_t inf, wm, zero, pad;
};
static_assert(sizeof(RecIn) == 304 && sizeof(RecOut) == 448, "record layout");

enum Op : int32_t {
    OP_UNPACK = 1,     // slot i: Fe -> f9_unpack
    OP_PACK = 2,       // slot i: Fe -> f9_pack(f9_unpack)
    OP_NORM = 3,       // slot i -> f9_norm
    OP_MUL = 4,        // (s0, s1), (s2, s3), (s4, s5), (s6, s7) -> out 0..3
    OP_SQR = 5,        // slot i -> sqr
    OP_MUL2_ADD = 6,   // (s0..s3), (s4..s7) -> out 0, 1
    OP_MUL2_SUB = 7,
    OP_DOT = 8,        // arg terms, term t = s[2 (t % 4)] * s[2 (t % 4) + 1]: triples then single terms, a carry() after each
    OP_CANON = 9,      // slot i -> canon
    OP_ISZERO = 10,    // slot i -> bit i of `zero`
    OP_REDUCE_PACK = 11,  // slot i -> Fe
    OP_MUL_SMALL = 12,    // slot i, c = arg
    OP_MUL2_SPLIT = 13,   // as OP_MUL2_SUB, by mulq twice and sub_fused
    OP_FE_MUL = 20,    // pairs as OP_MUL, 8 x 32-bit words
    OP_FE_SQR = 21,
    OP_FE_ADD = 22,
    OP_FE_SUB = 23,
    OP_FE_NEG = 24,    // slot i
    OP_FE_DBL = 25,
    OP_FE_FROM_RAW = 26,
    OP_FE_TO_RAW = 27,
    OP_MADD = 30,      // acc = s0..s3, inf = arg, qx = s4, qy = s5 -> out 0..3, inf
    OP_FROM_PAIR = 31, // x1, y1, x2, y2 = s0..s3 -> out 0..3 (all-zero where inf is set), inf
    OP_DBL = 32,       // s0..s3 -> out 0..3
    OP_ADD = 33,       // s0..s3 + s4..s7 -> out 0..3
    OP_TO_XYZZ = 34,   // s0..s3, inf = arg -> four Fe in out 0..3
    OP_LANES = 40,
    OP_XADDL1 = 40,    // s0..s3 + s4..s7 by xaddl<L> + xstore<L > 1> -> out 0..3; xyzz9_add of the same -> out 4..7;
    OP_XADDL2 = 41,    //   wm: four bits per lane of the group
    OP_XADDL4 = 42,
    OP_XADD1 = 43,     // the same through xadd<false>, xadd<true>, xadd4 called by name
    OP_XADD2 = 44,
    OP_XADD4 = 45,
    OP_XMADD_PAIR = 50,  // eight consecutive records are one chain of a lane pair, starting from inf: step = += (s0, s1);
                         //   out 0..3 the pair's x, y, zz, zzz (lane A's m, lane B's m, lane A's z and w), out 8 lane B's z (zzz again),
                         //   out 4..7 xyzz9_madd on one lane of the same chain;
                         //   inf: bit 0 lane A, bit 1 lane B, bit 2 the one-lane chain
};

template <class P>
ZG_HD void limb_op(const RecIn& in, RecOut& out) {
    switch (in.op) {
        case OP_NORM:
            for (int i = 0; i < 8; i++) out.s[i] = f9_norm(in.s[i]);
            break;
        case OP_MUL:
            for (int i = 0; i < 4; i++) out.s[i] = Field9<P>::mul(in.s[2 * i], in.s[2 * i + 1]);
            break;
        case OP_SQR:
            for (int i = 0; i < 8; i++) out.s[i] = Field9<P>::sqr(in.s[i]);
            break;
        case OP_MUL2_ADD:
            for (int i = 0; i < 2; i++)
                out.s[i] = Field9<P>::template mul2<false>(in.s[4 * i], in.s[4 * i + 1], in.s[4 * i + 2], in.s[4 * i + 3]);
            break;
        case OP_MUL2_SUB:
            for (int i = 0; i < 2; i++)
                out.s[i] = Field9<P>::template mul2<true>(in.s[4 * i], in.s[4 * i + 1], in.s[4 * i + 2], in.s[4 * i + 3]);
            break;
        case OP_MUL2_SPLIT:
            for (int i = 0; i < 2; i++) {
                F9 qh, qk;
                const F9 h = Field9<P>::mulq(in.s[4 * i], in.s[4 * i + 1], qh), k = Field9<P>::mulq(in.s[4 * i + 2], in.s[4 * i + 3], qk);
                out.s[i] = Field9<P>::sub_fused(h, qh, k, qk);
            }
            break;
        case OP_DOT: {
            Dot9<P> acc;
            acc.zero();
            int t = 0;
            for (; t + 3 <= in.arg; t += 3) {
                for (int u = t; u < t + 3; u++) acc.mac(in.s[2 * (u & 3)], in.s[2 * (u & 3) + 1]);
                acc.carry();
            }
            for (; t < in.arg; t++) {
                acc.mac(in.s[2 * (t & 3)], in.s[2 * (t & 3) + 1]);
                acc.carry();
            }
            out.s[0] = acc.reduce();
            break;
        }
        case OP_CANON:
            for (int i = 0; i < 8; i++) out.s[i] = Field9<P>::canon(in.s[i]);
            break;
        case OP_ISZERO: {
            int32_t z = 0;
            for (int i = 0; i < 8; i++) z |= Field9<P>::is_zero_mod_p(in.s[i]) ? (1 << i) : 0;
            out.zero = z;
            break;
        }
        case OP_REDUCE_PACK:
            for (int i = 0; i < 8; i++) {
                const Fe r = f9_reduce_pack<P>(in.s[i]);
                for (int w = 0; w < 8; w++) out.s[i].l[w] = (int32_t)r.l[w];
            }
            break;
        case OP_MUL_SMALL:
            for (int i = 0; i < 8; i++) out.s[i] = f9_mul_small<P>(in.s[i], in.arg);
            break;
        default:
            break;
    }
}

ZG_HD Fe slot_fe(const F9& s) {
    Fe r;
    for (int w = 0; w < 8; w++) r.l[w] = (uint32_t)s.l[w];
    return r;
}
ZG_HD void fe_slot(F9& s, const Fe& v) {
    for (int w = 0; w < 8; w++) s.l[w] = (int32_t)v.l[w];
}

template <class F>
ZG_HD void fe_op(const RecIn& in, RecOut& out) {
    if (in.op >= OP_FE_MUL && in.op <= OP_FE_SUB && in.op != OP_FE_SQR) {
        for (int i = 0; i < 4; i++) {
            const Fe a = slot_fe(in.s[2 * i]), b = slot_fe(in.s[2 * i + 1]);
            fe_slot(out.s[i], in.op == OP_FE_MUL ? F::mul(a, b) : in.op == OP_FE_ADD ? F::add(a, b) : F::sub(a, b));
        }
        return;
    }
    for (int i = 0; i < 8; i++) {
        const Fe a = slot_fe(in.s[i]);
        Fe r = a;
        switch (in.op) {
            case OP_FE_SQR: r = F::sqr(a); break;
            case OP_FE_NEG: r = F::neg(a); break;
            case OP_FE_DBL: r = F::dbl(a); break;
            case OP_FE_FROM_RAW: r = F::from_raw(a); break;
            case OP_FE_TO_RAW: r = F::to_raw(a); break;
            default: break;
        }
        fe_slot(out.s[i], r);
    }
}

ZG_HD XYZZ9 slots_point(const F9* s) {
    XYZZ9 p;
    p.x = s[0];
    p.y = s[1];
    p.zz = s[2];
    p.zzz = s[3];
    return p;
}
ZG_HD void point_slots(F9* s, const XYZZ9& p) {
    s[0] = p.x;
    s[1] = p.y;
    s[2] = p.zz;
    s[3] = p.zzz;
}

// every op below OP_LANES: the same function on the device (one thread per record) and on the host
ZG_HD void run_op(const RecIn& in, RecOut& out) {
    const int op = in.op;
    if (op == OP_UNPACK) {
        for (int i = 0; i < 8; i++) out.s[i] = f9_unpack(slot_fe(in.s[i]));
    } else if (op == OP_PACK) {
        for (int i = 0; i < 8; i++) fe_slot(out.s[i], f9_pack(f9_unpack(slot_fe(in.s[i]))));
    } else if (op < OP_FE_MUL) {
        if (in.field) limb_op<Fr9Params>(in, out);
        else limb_op<Fq9Params>(in, out);
    } else if (op < OP_MADD) {
        if (in.field) fe_op<Fr>(in, out);
        else fe_op<Fq>(in, out);
    } else if (op == OP_MADD) {
        XYZZ9 a = slots_point(in.s);
        bool inf = in.arg != 0;
        xyzz9_madd(a, inf, in.s[4], in.s[5]);
        point_slots(out.s, a);
        out.inf = inf ? 1 : 0;
    } else if (op == OP_FROM_PAIR) {
        XYZZ9 o = xyzz9_identity();
        bool inf = false;
        xyzz9_from_pair(in.s[0], in.s[1], in.s[2], in.s[3], o, inf);
        point_slots(out.s, o);
        out.inf = inf ? 1 : 0;
    } else if (op == OP_DBL) {
        point_slots(out.s, xyzz9_dbl(slots_point(in.s)));
    } else if (op == OP_ADD) {
        point_slots(out.s, xyzz9_add(slots_point(in.s), slots_point(in.s + 4)));
    } else if (op == OP_TO_XYZZ) {
        const XYZZ r = xyzz9_to_xyzz(slots_point(in.s), in.arg != 0);
        fe_slot(out.s[0], r.x);
        fe_slot(out.s[1], r.y);
        fe_slot(out.s[2], r.zz);
        fe_slot(out.s[3], r.zzz);
    }
}

// records [first, first + n) all carry the same op
__global__ void op_kernel(const RecIn* in, RecOut* out, int first, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RecOut o = out[first + i];
    run_op(in[first + i], o);
    out[first + i] = o;
}

// L lanes per record (a whole wave = 64 / L neighbouring records); the sum goes through xstore into the sentinel-filled
// result, then the group's first lane alone adds the same operands with xyzz9_add
template <int L, bool BY_NAME>
__global__ void xadd_kernel(const RecIn* in, RecOut* out, int first, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = t / L;
    if (g >= n) return;
    const uint32_t role = (uint32_t)(t % L);
    const RecIn* ri = in + first + g;
    RecOut* ro = out + first + g;
    const XYZZ9* pa = reinterpret_cast<const XYZZ9*>(&ri->s[0]);
    const XYZZ9* pb = reinterpret_cast<const XYZZ9*>(&ri->s[4]);
    XSum s;
    if constexpr (!BY_NAME) s = xaddl<L>(pa, pb, role);
    else if constexpr (L == 4) s = xadd4(pa, pb, role);
    else s = xadd<L == 2>(pa, pb, role);
    xstore<(L > 1)>(reinterpret_cast<XYZZ9*>(&ro->s[0]), s);
    atomicOr(&ro->wm, (int32_t)(s.wm << (4 * role)));
    if (role == 0) st_xyzz9(reinterpret_cast<XYZZ9*>(&ro->s[4]), xyzz9_add(ld_xyzz9(pa), ld_xyzz9(pb)));
}

// lanes 2c and 2c + 1 run chain c (records first + 8 c ...) with xmadd_pair; after every step the pair's point is put
// together from both lanes, and both lanes also run the same chain with xyzz9_madd (lane A writes it)
__global__ void xmadd_pair_kernel(const RecIn* in, RecOut* out, int first, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = t / 2;
    if (c * 8 >= n) return;
    const bool A = (t & 1) == 0;
    PairAcc acc;
    acc.m = acc.z = acc.w = xyzz9_identity().x;
    XYZZ9 one = xyzz9_identity();
    bool inf = true, inf1 = true;
    for (int step = 0; step < 8 && c * 8 + step < n; step++) {
        const RecIn* ri = in + first + c * 8 + step;
        RecOut* ro = out + first + c * 8 + step;
        const F9 qx = ld_f9(&ri->s[0]), qy = ld_f9(&ri->s[1]);
        xmadd_pair(acc, inf, qx, qy, A);
        xyzz9_madd(one, inf1, qx, qy);
        if (A) {
            st_f9(&ro->s[0], acc.m);
            st_f9(&ro->s[2], acc.z);
            st_f9(&ro->s[3], acc.w);
            st_xyzz9(reinterpret_cast<XYZZ9*>(&ro->s[4]), one);
        } else {
            st_f9(&ro->s[1], acc.m);
            st_f9(&ro->s[8], acc.z);
        }
        atomicOr(&ro->inf, (inf ? (A ? 1 : 2) : 0) | (A && inf1 ? 4 : 0));
    }
}

#define HIP_OK(call)                                                                       \
    do {                                                                                   \
        const hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "FAIL %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 2;                                                                      \
        }                                                                                  \
    } while (0)

static int run_device(const std::vector<RecIn>& in, std::vector<RecOut>& out) {
    const size_t n = in.size();
    RecIn* din = nullptr;
    RecOut* dout = nullptr;
    HIP_OK(hipSetDevice(0));
    HIP_OK(hipMalloc(&din, n * sizeof(RecIn)));
    HIP_OK(hipMalloc(&dout, n * sizeof(RecOut)));
    HIP_OK(hipMemcpy(din, in.data(), n * sizeof(RecIn), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dout, out.data(), n * sizeof(RecOut), hipMemcpyHostToDevice));
    for (size_t first = 0; first < n;) {  // one launch per run of records with the same op
        const int op = in[first].op;
        size_t end = first;
        while (end < n && in[end].op == op) end++;
        const int cnt = (int)(end - first), f = (int)first;
        auto blocks = [](long threads) { return dim3((unsigned)((threads + 63) / 64)); };
        switch (op) {
            case OP_XADDL1: hipLaunchKernelGGL((xadd_kernel<1, false>), blocks(cnt), dim3(64), 0, 0, din, dout, f, cnt); break;
            case OP_XADDL2: hipLaunchKernelGGL((xadd_kernel<2, false>), blocks(2L * cnt), dim3(64), 0, 0, din, dout, f, cnt); break;
            case OP_XADDL4: hipLaunchKernelGGL((xadd_kernel<4, false>), blocks(4L * cnt), dim3(64), 0, 0, din, dout, f, cnt); break;
            case OP_XADD1: hipLaunchKernelGGL((xadd_kernel<1, true>), blocks(cnt), dim3(64), 0, 0, din, dout, f, cnt); break;
            case OP_XADD2: hipLaunchKernelGGL((xadd_kernel<2, true>), blocks(2L * cnt), dim3(64), 0, 0, din, dout, f, cnt); break;
            case OP_XADD4: hipLaunchKernelGGL((xadd_kernel<4, true>), blocks(4L * cnt), dim3(64), 0, 0, din, dout, f, cnt); break;
            case OP_XMADD_PAIR:
                hipLaunchKernelGGL(xmadd_pair_kernel, blocks(2L * ((cnt + 7) / 8)), dim3(64), 0, 0, din, dout, f, cnt);
                break;
            default:
                if (op < OP_UNPACK || op >= OP_LANES) {
                    fprintf(stderr, "FAIL unknown op %d at record %zu\n", op, first);
                    return 2;
                }
                hipLaunchKernelGGL(op_kernel, blocks(cnt), dim3(64), 0, 0, din, dout, f, cnt);
        }
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        first = end;
    }
    HIP_OK(hipMemcpy(out.data(), dout, n * sizeof(RecOut), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(din));
    HIP_OK(hipFree(dout));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4 || (strcmp(argv[1], "device") && strcmp(argv[1], "host"))) {
        fprintf(stderr, "usage: field9_probe device|host IN OUT\n");
        return 2;
    }
    const bool device = !strcmp(argv[1], "device");
    FILE* fi = fopen(argv[2], "rb");
    if (!fi) { fprintf(stderr, "FAIL cannot read %s\n", argv[2]); return 2; }
    fseek(fi, 0, SEEK_END);
    const long bytes = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (long)sizeof(RecIn)) { fprintf(stderr, "FAIL %s: %ld bytes is no whole number of records\n", argv[2], bytes); return 2; }
    std::vector<RecIn> in((size_t)bytes / sizeof(RecIn));
    if (fread(in.data(), sizeof(RecIn), in.size(), fi) != in.size()) { fprintf(stderr, "FAIL short read\n"); return 2; }
    fclose(fi);
    std::vector<RecOut> out(in.size());
    memset(out.data(), 0x5a, out.size() * sizeof(RecOut));
    for (auto& o : out) o.inf = o.wm = o.zero = o.pad = 0;
    if (device) {
        const int rc = run_device(in, out);
        if (rc) return rc;
    } else {
        for (size_t i = 0; i < in.size(); i++) {
            if (in[i].op < OP_UNPACK || in[i].op >= OP_LANES) { fprintf(stderr, "FAIL op %d at record %zu is not a host op\n", in[i].op, i); return 2; }
            run_op(in[i], out[i]);
        }
    }
    FILE* fo = fopen(argv[3], "wb");
    if (!fo || fwrite(out.data(), sizeof(RecOut), out.size(), fo) != out.size() || fclose(fo)) { fprintf(stderr, "FAIL cannot write %s\n", argv[3]); return 2; }
    printf("%zu records %s\n", in.size(), device ? "device" : "host");
    return 0;
}
