// fetest.hip -- field-arithmetic vectors for tests/test_gpu_field.py: reads lines "op a b" (hex,
// 256-bit, op in add/sub/mul/sqr/norm/shl1/shl2/shl3/mul3) from stdin, evaluates them with FieldK1 on the GPU (one
// vector per lane), prints the canonical result per line.  Covers the rare carry/borrow tails of
// the k1_add/k1_sub asm that random inputs almost never reach.
//
// A field selector in front of the op, "p2:mul", "n1:inv", "n2:gcd_var", picks one of the 8 x 32-bit
// Montgomery fields instead (FieldP2 with the multiplication-free redc_sm2p, FieldN1, FieldN2; no selector
// or "k1:" is FieldK1).  Their ops: mul sqr add sub neg from_plain to_plain inv (Mont<>::inv's Fermat chains,
// FieldP2::inv for p2), the safegcd inversions of modinv.h on a plain residue with the field's ModInfo30
// (gcd gcd_pipe gcd_var, also for k1) and on a Montgomery residue (minv minv_pipe minv_var:
// mont_inv_safegcd<P, 0 | 1 | 2>).  Operands are < m as those contracts say; the result is printed as the op
// leaves it, with no normalisation after it.  These run in a second launch.  Every HIP call is checked: the
// first error ends the program with a nonzero status and nothing is launched after it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../csrc/modinv.h"

using namespace bcosgpu;

__global__ void k(const uint32_t* in, const int* op, const int* idx, int n, uint32_t* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = idx[t];
    fe a, b, r;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        a.v[w] = in[16 * i + w];
        b.v[w] = in[16 * i + 8 + w];
    }
    switch (op[i]) {
        case 0: FieldK1::add(r, a, b); break;
        case 1: FieldK1::sub(r, a, b); break;
        case 2: FieldK1::mul(r, a, b); break;
        case 3: FieldK1::sqr(r, a); break;
        case 5: FieldK1::shl<1>(r, a); break;
        case 6: FieldK1::shl<2>(r, a); break;
        case 7: FieldK1::shl<3>(r, a); break;
        case 8: FieldK1::mul3(r, a); break;
        default: fe_copy(r, a); break;
    }
    FieldK1::normalize(r);
#pragma unroll
    for (int w = 0; w < 8; ++w) out[8 * i + w] = r.v[w];
}

enum MOp : int { M_MUL, M_SQR, M_ADD, M_SUB, M_NEG, M_FROM_PLAIN, M_TO_PLAIN, M_INV, M_GCD, M_GCD_PIPE, M_GCD_VAR,
                 M_MINV, M_MINV_PIPE, M_MINV_VAR, M_COUNT };

template <class F, class P>
__device__ __noinline__ void mont_op(int op, fe& r, const fe& a, const fe& b, const ModInfo30& mi, const uint32_t* r3) {
    switch (op) {
        case M_MUL: F::mul(r, a, b); break;
        case M_SQR: F::sqr(r, a); break;
        case M_ADD: F::add(r, a, b); break;
        case M_SUB: F::sub(r, a, b); break;
        case M_NEG: F::neg(r, a); break;
        case M_FROM_PLAIN: F::from_plain(r, a); break;
        case M_TO_PLAIN: F::to_plain(r, a); break;
        case M_INV: F::inv(r, a); break;
        case M_GCD: modinv_safegcd(r, a, mi); break;
        case M_GCD_PIPE: modinv_safegcd_pipe(r, a, mi); break;
        case M_GCD_VAR: modinv_safegcd_var(r, a, mi); break;
        case M_MINV: mont_inv_safegcd<P, 0>(r, a, mi, r3); break;
        case M_MINV_PIPE: mont_inv_safegcd<P, 1>(r, a, mi, r3); break;
        case M_MINV_VAR: mont_inv_safegcd<P, 2>(r, a, mi, r3); break;
        default: fe_zero(r); break;
    }
}

// the Montgomery fields and the inversions: op[i] = 64 * field (0 k1, 1 p2, 2 n1, 3 n2) + MOp, one case per
// lane through idx, the result stored as the op returns it
__global__ void km(const uint32_t* in, const int* op, const int* idx, int n, uint32_t* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = idx[t];
    fe a, b, r;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        a.v[w] = in[16 * i + w];
        b.v[w] = in[16 * i + 8 + w];
    }
    const int f = op[i] >> 6, o = op[i] & 63;
    if (f == 1) mont_op<FieldP2, ParamP2>(o, r, a, b, kMod30P2, kR3P2);
    else if (f == 2) mont_op<FieldN1, ParamN1>(o, r, a, b, kMod30N1, kR3N1);
    else if (f == 3) mont_op<FieldN2, ParamN2>(o, r, a, b, kMod30N2, kR3N2);
    else if (o == M_GCD) modinv_safegcd(r, a, kMod30K1P);
    else if (o == M_GCD_PIPE) modinv_safegcd_pipe(r, a, kMod30K1P);
    else if (o == M_GCD_VAR) modinv_safegcd_var(r, a, kMod30K1P);
    else fe_zero(r);
#pragma unroll
    for (int w = 0; w < 8; ++w) out[8 * i + w] = r.v[w];
}

// "field:op" -> 64 * field + MOp, or -1
static int parse_mont(const std::string& o) {
    static const char* kFields[] = {"k1", "p2", "n1", "n2"};
    static const char* kOps[M_COUNT] = {"mul", "sqr", "add", "sub", "neg", "from_plain", "to_plain", "inv", "gcd",
                                        "gcd_pipe", "gcd_var", "minv", "minv_pipe", "minv_var"};
    const size_t colon = o.find(':');
    for (int f = 0; f < 4; ++f)
        for (int k = 0; k < M_COUNT; ++k)
            if (o.compare(0, colon, kFields[f]) == 0 && o.compare(colon + 1, std::string::npos, kOps[k]) == 0)
                return (f == 0 && (k < M_GCD || k > M_GCD_VAR)) ? -1 : 64 * f + k;
    return -1;
}

#define HIP_OK(call)                                                              \
    do {                                                                          \
        const hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "fetest: %s: %s\n", #call, hipGetErrorString(e_));    \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static void parse(const char* h, uint32_t* w) {
    char buf[65];
    const size_t len = strlen(h) < 64 ? strlen(h) : 64;
    memset(buf, '0', 64);
    memcpy(buf + 64 - len, h + strlen(h) - len, len);
    buf[64] = 0;
    for (int q = 0; q < 8; ++q) {
        char part[9];
        memcpy(part, buf + 8 * (7 - q), 8);
        part[8] = 0;
        w[q] = static_cast<uint32_t>(strtoul(part, nullptr, 16));
    }
}

int main() {
    std::vector<uint32_t> in;
    std::vector<int> ops, k1idx, midx;
    char op[24], a[80], b[80];
    while (scanf("%23s %79s %79s", op, a, b) == 3) {
        uint32_t w[16];
        parse(a, w);
        parse(b, w + 8);
        in.insert(in.end(), w, w + 16);
        std::string o(op);
        const int i = static_cast<int>(ops.size());
        if (o.compare(0, 3, "k1:") == 0 && parse_mont(o) < 0) o = o.substr(3);
        if (o.find(':') != std::string::npos) {
            const int code = parse_mont(o);
            if (code < 0) {
                fprintf(stderr, "fetest: line %d: no such field or op: %s\n", i + 1, op);
                return 2;
            }
            ops.push_back(code);
            midx.push_back(i);
            continue;
        }
        const int code = o == "add" ? 0 : o == "sub" ? 1 : o == "mul" ? 2 : o == "sqr" ? 3 : o == "norm" ? 4 : o == "shl1" ? 5
                         : o == "shl2" ? 6 : o == "shl3" ? 7 : o == "mul3" ? 8 : -1;
        if (code < 0) {
            fprintf(stderr, "fetest: line %d: no such op: %s\n", i + 1, op);
            return 2;
        }
        ops.push_back(code);
        k1idx.push_back(i);
    }
    const int n = static_cast<int>(ops.size());
    if (!n) return 0;
    uint32_t *din, *dout;
    int *dop, *didx;
    HIP_OK(hipMalloc(&din, in.size() * 4));
    HIP_OK(hipMalloc(&dout, n * 32));
    HIP_OK(hipMalloc(&dop, n * 4));
    HIP_OK(hipMalloc(&didx, n * 4));
    HIP_OK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dop, ops.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0, n * 32));
    if (!k1idx.empty()) {
        const int m = static_cast<int>(k1idx.size());
        HIP_OK(hipMemcpy(didx, k1idx.data(), m * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k, dim3((m + 255) / 256), dim3(256), 0, 0, din, dop, didx, m, dout);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
    }
    if (!midx.empty()) {
        const int m = static_cast<int>(midx.size());
        HIP_OK(hipMemcpy(didx, midx.data(), m * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(km, dim3((m + 63) / 64), dim3(64), 0, 0, din, dop, didx, m, dout);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
    }
    std::vector<uint32_t> out(8 * n);
    HIP_OK(hipMemcpy(out.data(), dout, n * 32, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        for (int q = 7; q >= 0; --q) printf("%08x", out[8 * i + q]);
        printf("\n");
    }
    return 0;
}
