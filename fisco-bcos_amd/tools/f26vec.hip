// f26vec.hip -- vectors for the two 10 x 26-bit fields as the device runs them (fe26.h: secp256k1, fp26.h:
// SM2 in Montgomery form, R = 2^286), for tests/test_gpu_f26.py.  On the device fe26_mul / fe26_sqr /
// fp26_mul / fp26_sqr are the generated inline-asm blocks of fe_asm.h, which no host build runs.
//
// stdin: one case per line, "<field> <op> <a> <b>": field k1 | p2, a and b ten raw hex limbs joined by
// commas (limb 0 first; any representation within the op's magnitude contract, canonical or not).  Ops:
//   mul sqr add weak norm is_zero to_mont from_mont inv      (to_mont / from_mont / inv: p2 only)
//   sub<K> neg<K> mul_int<C>, written sub9, neg2, mul_int4   (the K and C of the dispatch below)
//   sqrt_cand sqrt_split0 sqrt_split1                        (k1 only; split<CUT> = head<CUT> then tail<CUT>)
// stdout: one line per case, the raw result limbs exactly as the op leaves them (nothing is normalised
// that the op does not normalise itself), or 0 / 1 for is_zero, or "na" for an op this build cannot run.
// One thread per case, two launches (the square-root chains have their own kernel); every HIP call is
// checked, the first error ends the program with a nonzero status and nothing is launched after it.
//
// Host leg: the same file compiled by a C++ compiler (g++ -x c++ -DFE26_CHECK) runs the kernels' bodies
// (run_k1 / run_p2 / run_sqrt) as a loop over the cases on the C++ fallbacks, with every magnitude
// contract and limb bound asserted; `inv` (safegcd, device-only) prints "na" there.
// tests/test_f26vec_host.py feeds it the GPU test's case file.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "../csrc/ecc_device.h"  // fp26_inv (verify_sm2_26.h) with the safegcd it calls
#define VEC_OUTLINE __host__ __device__ __noinline__ static
#else
#include "../csrc/fp26.h"
#define VEC_OUTLINE static
#endif

using namespace bcosgpu;

enum Op : int {
    OP_MUL, OP_SQR, OP_ADD, OP_WEAK, OP_NORM, OP_IS_ZERO, OP_SUB, OP_NEG, OP_MUL_INT, OP_TO_MONT, OP_FROM_MONT,
    OP_INV, OP_SQRT_CAND, OP_SQRT_SPLIT0, OP_SQRT_SPLIT1
};
struct Case {
    int field, op, k;  // field 0 k1, 1 p2; k: the K of sub / neg, the C of mul_int
    uint32_t a[10], b[10];
};
struct Res {
    uint32_t v[10];
    int flag;  // is_zero's answer; -1 where the op is not available
};

// smallest magnitude that holds the limbs (what FE26_CHECK tracks; unused otherwise)
static int magnitude(const uint32_t* v) {
    uint64_t m = 1;
    for (int i = 0; i < 10; ++i) {
        const int sh = i == 9 ? 22 : 26;
        const uint64_t need = (static_cast<uint64_t>(v[i]) + (1ull << sh) - 1) >> sh;
        if (need > m) m = need;
    }
    return static_cast<int>(m);
}

template <class E>
F26_HD void load(E& e, const uint32_t* v, int m) {
#pragma unroll
    for (int i = 0; i < 10; ++i) e.v[i] = v[i];
    F26_SETM(e, m);
    (void)m;
}

// the K of fe26_sub<K> / fp26_sub<K> and the C of mul_int<C> that ec26.h, ecp26.h, ec26_trio.h,
// ecp26_trio.h, recover26.h, verify_sm2_26.h, ecc_device.h and the kernels instantiate (neg: K = 2 only);
// tests/f26_cases.py keeps the same lists
#define K1_SUB(X) X(2) X(3) X(4) X(6) X(7) X(9) X(10) X(11)
#define K1_MUL_INT(X) X(2) X(3) X(4) X(8) X(16)
#define P2_SUB(X) X(2) X(3) X(4) X(8) X(9) X(12) X(13)
#define P2_MUL_INT(X) X(2) X(3) X(4) X(8) X(12)

F26_HD void run_k1(const Case& c, int ma, int mb, Res& o) {
    fe26 a, b, r;
    load(a, c.a, ma);
    load(b, c.b, mb);
    fe26_zero(r);
    o.flag = 0;
    switch (c.op) {
        case OP_MUL: fe26_mul(r, a, b); break;
        case OP_SQR: fe26_sqr(r, a); break;
        case OP_ADD: fe26_add(r, a, b); break;
        case OP_WEAK: fe26_copy(r, a); fe26_normalize_weak(r); break;
        case OP_NORM: fe26_copy(r, a); fe26_normalize(r); break;
        case OP_IS_ZERO: o.flag = fe26_is_zero(a) ? 1 : 0; break;
        case OP_SUB:
            switch (c.k) {
#define X(K) case K: fe26_sub<K>(r, a, b); break;
                K1_SUB(X)
#undef X
                default: o.flag = -1;
            }
            break;
        case OP_NEG:
            if (c.k == 2) fe26_neg<2>(r, a);
            else o.flag = -1;
            break;
        case OP_MUL_INT:
            switch (c.k) {
#define X(C) case C: fe26_mul_int<C>(r, a); break;
                K1_MUL_INT(X)
#undef X
                default: o.flag = -1;
            }
            break;
        default: o.flag = -1;
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) o.v[i] = r.v[i];
}

F26_HD void run_p2(const Case& c, int ma, int mb, Res& o) {
    fp26 a, b, r;
    load(a, c.a, ma);
    load(b, c.b, mb);
    fp26_zero(r);
    o.flag = 0;
    switch (c.op) {
        case OP_MUL: fp26_mul(r, a, b); break;
        case OP_SQR: fp26_sqr(r, a); break;
        case OP_ADD: fp26_add(r, a, b); break;
        case OP_WEAK: fp26_copy(r, a); fp26_normalize_weak(r); break;
        case OP_NORM: fp26_copy(r, a); fp26_normalize(r); break;
        case OP_IS_ZERO: o.flag = fp26_is_zero(a) ? 1 : 0; break;
        case OP_TO_MONT: fp26_to_mont(r, a); break;
        case OP_FROM_MONT: fp26_from_mont(r, a); break;
        case OP_INV:
#if defined(__HIP_DEVICE_COMPILE__)
            fp26_inv(r, a);
#else
            o.flag = -1;
#endif
            break;
        case OP_SUB:
            switch (c.k) {
#define X(K) case K: fp26_sub<K>(r, a, b); break;
                P2_SUB(X)
#undef X
                default: o.flag = -1;
            }
            break;
        case OP_NEG:
            if (c.k == 2) fp26_neg<2>(r, a);
            else o.flag = -1;
            break;
        case OP_MUL_INT:
            switch (c.k) {
#define X(C) case C: fp26_mul_int<C>(r, a); break;
                P2_MUL_INT(X)
#undef X
                default: o.flag = -1;
            }
            break;
        default: o.flag = -1;
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) o.v[i] = r.v[i];
}

// the square-root chains (k1): a kernel of their own, each chain out of line, so that neither kernel
// carries several hundred inlined products
template <int CUT>
VEC_OUTLINE void sqrt_split(fe26& r, const fe26& a) {
    fe26 st[fe26_sqrt_live<CUT>()];
    fe26_sqrt_head<CUT>(st, a);
    fe26_sqrt_tail<CUT>(r, st);
}
VEC_OUTLINE void sqrt_whole(fe26& r, const fe26& a) { fe26_sqrt_cand(r, a); }

F26_HD void run_sqrt(const Case& c, int ma, Res& o) {
    fe26 a, r;
    load(a, c.a, ma);
    fe26_zero(r);
    o.flag = 0;
    if (c.op == OP_SQRT_CAND) sqrt_whole(r, a);
    else if (c.op == OP_SQRT_SPLIT0) sqrt_split<0>(r, a);
    else if (c.op == OP_SQRT_SPLIT1) sqrt_split<1>(r, a);
    else o.flag = -1;
#pragma unroll
    for (int i = 0; i < 10; ++i) o.v[i] = r.v[i];
}

static bool is_sqrt(int op) { return op == OP_SQRT_CAND || op == OP_SQRT_SPLIT0 || op == OP_SQRT_SPLIT1; }

#if defined(__HIPCC__)
__global__ void k_ops(const Case* cs, const int* idx, int n, Res* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const Case c = cs[idx[t]];
    Res o;
    if (c.field == 0) run_k1(c, 1, 1, o);
    else run_p2(c, 1, 1, o);
    out[idx[t]] = o;
}
__global__ void k_sqrt(const Case* cs, const int* idx, int n, Res* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const Case c = cs[idx[t]];
    Res o;
    run_sqrt(c, 1, o);
    out[idx[t]] = o;
}

#define HIP_OK(call)                                                                        \
    do {                                                                                    \
        const hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                             \
            fprintf(stderr, "f26vec: %s: %s\n", #call, hipGetErrorString(e_));              \
            return false;                                                                   \
        }                                                                                   \
    } while (0)

static bool run_all(const std::vector<Case>& cs, std::vector<Res>& out) {
    const int n = static_cast<int>(cs.size());
    std::vector<int> plain, roots;
    for (int i = 0; i < n; ++i) (is_sqrt(cs[i].op) ? roots : plain).push_back(i);
    Case* dcs = nullptr;
    Res* dout = nullptr;
    int* didx = nullptr;
    HIP_OK(hipMalloc(&dcs, n * sizeof(Case)));
    HIP_OK(hipMalloc(&dout, n * sizeof(Res)));
    HIP_OK(hipMalloc(&didx, n * sizeof(int)));
    HIP_OK(hipMemcpy(dcs, cs.data(), n * sizeof(Case), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xff, n * sizeof(Res)));
    if (!plain.empty()) {
        const int m = static_cast<int>(plain.size());
        HIP_OK(hipMemcpy(didx, plain.data(), m * sizeof(int), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_ops, dim3((m + 255) / 256), dim3(256), 0, 0, dcs, didx, m, dout);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
    }
    if (!roots.empty()) {
        const int m = static_cast<int>(roots.size());
        HIP_OK(hipMemcpy(didx, roots.data(), m * sizeof(int), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_sqrt, dim3((m + 63) / 64), dim3(64), 0, 0, dcs, didx, m, dout);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
    }
    HIP_OK(hipMemcpy(out.data(), dout, n * sizeof(Res), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(dcs));
    HIP_OK(hipFree(dout));
    HIP_OK(hipFree(didx));
    return true;
}
#else
static bool run_all(const std::vector<Case>& cs, std::vector<Res>& out) {
    for (size_t i = 0; i < cs.size(); ++i) {
        const Case& c = cs[i];
        const int ma = magnitude(c.a), mb = magnitude(c.b);
        if (is_sqrt(c.op)) run_sqrt(c, ma, out[i]);
        else if (c.field == 0) run_k1(c, ma, mb, out[i]);
        else run_p2(c, ma, mb, out[i]);
    }
    return true;
}
#endif

static bool parse_limbs(const char* s, uint32_t* v) {
    for (int i = 0; i < 10; ++i) {
        char* end = nullptr;
        const unsigned long long x = strtoull(s, &end, 16);
        if (end == s || x > 0xffffffffull) return false;
        v[i] = static_cast<uint32_t>(x);
        if (i < 9) {
            if (*end != ',') return false;
            s = end + 1;
        } else if (*end != 0) {
            return false;
        }
    }
    return true;
}

static bool parse_op(const std::string& o, int field, Case& c) {
    static const struct { const char* name; int op, field; } kPlain[] = {
        {"mul", OP_MUL, -1}, {"sqr", OP_SQR, -1}, {"add", OP_ADD, -1}, {"weak", OP_WEAK, -1}, {"norm", OP_NORM, -1},
        {"is_zero", OP_IS_ZERO, -1}, {"to_mont", OP_TO_MONT, 1}, {"from_mont", OP_FROM_MONT, 1}, {"inv", OP_INV, 1},
        {"sqrt_cand", OP_SQRT_CAND, 0}, {"sqrt_split0", OP_SQRT_SPLIT0, 0}, {"sqrt_split1", OP_SQRT_SPLIT1, 0}};
    c.k = 0;
    for (const auto& p : kPlain)
        if (o == p.name) {
            c.op = p.op;
            return p.field < 0 || p.field == field;
        }
    static const struct { const char* prefix; int op; } kParam[] = {{"mul_int", OP_MUL_INT}, {"sub", OP_SUB}, {"neg", OP_NEG}};
    for (const auto& p : kParam) {
        const size_t len = strlen(p.prefix);
        if (o.compare(0, len, p.prefix) == 0 && o.size() > len) {
            c.op = p.op;
            c.k = atoi(o.c_str() + len);
            return c.k > 0;
        }
    }
    return false;
}

int main() {
    std::vector<Case> cs;
    char field[8], op[24], a[128], b[128];
    while (scanf("%7s %23s %127s %127s", field, op, a, b) == 4) {
        Case c;
        c.field = strcmp(field, "k1") == 0 ? 0 : strcmp(field, "p2") == 0 ? 1 : -1;
        if (c.field < 0 || !parse_op(op, c.field, c) || !parse_limbs(a, c.a) || !parse_limbs(b, c.b)) {
            fprintf(stderr, "f26vec: bad case line %zu: %s %s\n", cs.size() + 1, field, op);
            return 2;
        }
        cs.push_back(c);
    }
    if (cs.empty()) return 0;
    std::vector<Res> out(cs.size());
    if (!run_all(cs, out)) return 1;
    for (size_t i = 0; i < cs.size(); ++i) {
        if (out[i].flag < 0) {
            if (cs[i].op != OP_INV) {
                fprintf(stderr, "f26vec: case %zu: no such instantiation: %d\n", i + 1, cs[i].k);
                return 2;
            }
            printf("na\n");
        } else if (cs[i].op == OP_IS_ZERO) {
            printf("%d\n", out[i].flag);
        } else {
            for (int j = 0; j < 10; ++j) printf("%x%c", out[i].v[j], j == 9 ? '\n' : ',');
        }
    }
    return 0;
}
