// rowvec.hip -- vectors for the row-spread fields (fe_row.h: secp256k1 and SM2, one limb per lane of a
// 16-lane DPP row) and the row helpers of ec_row.h, for tests/test_gpu_row_field.py.  The code is
// device-only (DPP moves, permlane swaps), so this is its only unit test.
//
// stdin: one ROW per line, "<op> <a> <b>", a and b ten raw hex limbs joined by commas (lanes 0..9; lanes
// 10..15 are loaded with 0 as the contract requires).  Four consecutive lines are the four rows of one
// wave and must name the same op (a wave runs one op: the DPP moves need every lane enabled); the test
// chooses what the neighbouring rows hold.  The line count must be a multiple of four.  Ops:
//   mul sqr mul_sm2 sqr_sm2 add                           per row
//   sub<K> neg<K> sub_sm2<K> neg_sm2<K> mul_int<C>        per row; K, C as dispatched below
//   from_fe26 from_words                                  per row; from_words takes eight words in a[0..7]
//   gather4_0..3 gather01_0 gather01_1 gather0            what every row receives from row j
//   sel4                                                  sel4(L, a, b, a + b, a ^ b)
//   to_fe26 is_zero is_zero_sm2                           of ROW 0's element, the answer seen by every row
// stdout: one line per row: the sixteen lane values as the op leaves them; for to_fe26 the ten fe26 limbs
// that the row's lane 0 holds; for the zero tests 0 / 1.  One launch, one wave per block; every HIP call is
// checked and the first error ends the program with a nonzero status.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../csrc/ecc_device.h"  // ec_row.h's table loaders use its fe, Booth digits and shifts
#include "../csrc/ec_row.h"

using namespace bcosgpu;

enum Op : int {
    OP_MUL, OP_SQR, OP_MUL_SM2, OP_SQR_SM2, OP_ADD, OP_SUB, OP_NEG, OP_SUB_SM2, OP_NEG_SM2, OP_MUL_INT, OP_FROM_FE26,
    OP_FROM_WORDS, OP_GATHER4, OP_GATHER01, OP_GATHER0, OP_SEL4, OP_TO_FE26, OP_IS_ZERO, OP_IS_ZERO_SM2
};
struct Row {
    int op, k;  // k: the K of sub / neg, the C of mul_int, the j of gather4_j / gather01_j
    uint32_t a[10], b[10];
};
struct Out {
    uint32_t v[16];
};

// the K and C that ec_row.h and ecc_row.hip instantiate; tests/row_vectors.py keeps the same lists
#define ROW_SUB(X) X(2) X(3) X(7) X(9) X(10) X(11)
#define ROW_MUL_INT(X) X(2) X(3) X(4) X(8)

__global__ void __launch_bounds__(64) k_rows(const Row* rows, Out* out) {
    __shared__ uint32_t slot[16];
    const int lane = threadIdx.x;
    const frow::Lane L(lane);
    const frow::Sm2Lane C(L);
    const Row& me = rows[4 * blockIdx.x + L.row];
    const int op = __builtin_amdgcn_readfirstlane(me.op), kk = __builtin_amdgcn_readfirstlane(me.k);
    const uint32_t a = L.k < 10 ? me.a[L.k] : 0u, b = L.k < 10 ? me.b[L.k] : 0u;
    uint32_t r = 0;
    bool whole = false;  // the answer is an fe26 / a flag per row, not a lane value
    fe26 t;
    fe26_zero(t);
    uint32_t flag = 0;
    switch (op) {
        case OP_MUL: r = frow::mul(a, b, L); break;
        case OP_SQR: r = frow::sqr(a, L); break;
        case OP_MUL_SM2: r = frow::mul_sm2(a, b, L, C); break;
        case OP_SQR_SM2: r = frow::mul_sm2(a, a, L, C); break;
        case OP_ADD: r = frow::add(a, b); break;
        case OP_SUB:
            switch (kk) {
#define X(K) case K: r = frow::sub<K>(a, b, L); break;
                ROW_SUB(X)
#undef X
            }
            break;
        case OP_SUB_SM2:
            switch (kk) {
#define X(K) case K: r = frow::sub_sm2<K>(a, b, C); break;
                ROW_SUB(X)
#undef X
            }
            break;
        case OP_NEG: r = frow::neg<2>(a, L); break;
        case OP_NEG_SM2: r = frow::neg_sm2<2>(a, C); break;
        case OP_MUL_INT:
            switch (kk) {
#define X(K) case K: r = frow::mul_int<K>(a); break;
                ROW_MUL_INT(X)
#undef X
            }
            break;
        case OP_FROM_FE26: {
            fe26 x;
#pragma unroll
            for (int q = 0; q < 10; ++q) x.v[q] = me.a[q];
            r = frow::from_fe26(x, L);
            break;
        }
        case OP_FROM_WORDS: r = frow::from_words(me.a, L); break;
        case OP_GATHER4: {
            const frow::Rows4 g = frow::gather4(a);
            r = kk == 0 ? g.v[0] : kk == 1 ? g.v[1] : kk == 2 ? g.v[2] : g.v[3];
            break;
        }
        case OP_GATHER01: {
            uint32_t p0, p1;
            frow::gather01(a, p0, p1);
            r = kk == 0 ? p0 : p1;
            break;
        }
        case OP_GATHER0: r = frow::gather0(a); break;
        case OP_SEL4: r = frow::sel4(L, a, b, a + b, a ^ b); break;
        case OP_TO_FE26: frow::to_fe26(t, a, slot, L); whole = true; break;
        case OP_IS_ZERO: flag = frow::is_zero(a, slot, L) ? 1u : 0u; whole = true; break;
        case OP_IS_ZERO_SM2: flag = frow::is_zero_sm2(a, slot, L) ? 1u : 0u; whole = true; break;
    }
    Out& o = out[4 * blockIdx.x + L.row];
    if (!whole) {
        o.v[L.k] = r;
    } else if (L.k == 0) {
#pragma unroll
        for (int q = 0; q < 10; ++q) o.v[q] = t.v[q];
        o.v[10] = flag;
    }
}

#define HIP_OK(call)                                                           \
    do {                                                                       \
        const hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) {                                                \
            fprintf(stderr, "rowvec: %s: %s\n", #call, hipGetErrorString(e_)); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

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

static bool in_list(int k, std::initializer_list<int> l) {
    for (int x : l)
        if (x == k) return true;
    return false;
}

static bool parse_op(const std::string& o, Row& r) {
    static const struct { const char* name; int op; } kPlain[] = {
        {"mul", OP_MUL}, {"sqr", OP_SQR}, {"mul_sm2", OP_MUL_SM2}, {"sqr_sm2", OP_SQR_SM2}, {"add", OP_ADD},
        {"from_fe26", OP_FROM_FE26}, {"from_words", OP_FROM_WORDS}, {"gather0", OP_GATHER0}, {"sel4", OP_SEL4},
        {"to_fe26", OP_TO_FE26}, {"is_zero", OP_IS_ZERO}, {"is_zero_sm2", OP_IS_ZERO_SM2}};
    r.k = 0;
    for (const auto& p : kPlain)
        if (o == p.name) {
            r.op = p.op;
            return true;
        }
    static const struct { const char* prefix; int op; } kParam[] = {
        {"sub_sm2", OP_SUB_SM2}, {"neg_sm2", OP_NEG_SM2}, {"mul_int", OP_MUL_INT}, {"sub", OP_SUB}, {"neg", OP_NEG},
        {"gather4_", OP_GATHER4}, {"gather01_", OP_GATHER01}};
    for (const auto& p : kParam) {
        const size_t len = strlen(p.prefix);
        if (o.compare(0, len, p.prefix) != 0 || o.size() <= len || o.find_first_not_of("0123456789", len) != std::string::npos)
            continue;
        r.op = p.op;
        r.k = atoi(o.c_str() + len);
        switch (p.op) {
            case OP_SUB: case OP_SUB_SM2: return in_list(r.k, {2, 3, 7, 9, 10, 11});
            case OP_NEG: case OP_NEG_SM2: return r.k == 2;
            case OP_MUL_INT: return in_list(r.k, {2, 3, 4, 8});
            case OP_GATHER4: return r.k < 4;
            default: return r.k < 2;
        }
    }
    return false;
}

int main() {
    std::vector<Row> rows;
    char op[24], a[128], b[128];
    while (scanf("%23s %127s %127s", op, a, b) == 3) {
        Row r;
        if (!parse_op(op, r) || !parse_limbs(a, r.a) || !parse_limbs(b, r.b)) {
            fprintf(stderr, "rowvec: bad line %zu: %s\n", rows.size() + 1, op);
            return 2;
        }
        if (rows.size() % 4 != 0 && (rows.back().op != r.op || rows.back().k != r.k)) {
            fprintf(stderr, "rowvec: line %zu: the four rows of a wave must name one op\n", rows.size() + 1);
            return 2;
        }
        rows.push_back(r);
    }
    if (rows.size() % 4 != 0) {
        fprintf(stderr, "rowvec: %zu rows: not whole waves\n", rows.size());
        return 2;
    }
    if (rows.empty()) return 0;
    const size_t n = rows.size();
    Row* drows = nullptr;
    Out* dout = nullptr;
    HIP_OK(hipMalloc(&drows, n * sizeof(Row)));
    HIP_OK(hipMalloc(&dout, n * sizeof(Out)));
    HIP_OK(hipMemcpy(drows, rows.data(), n * sizeof(Row), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xff, n * sizeof(Out)));
    hipLaunchKernelGGL(k_rows, dim3(static_cast<unsigned>(n / 4)), dim3(64), 0, 0, drows, dout);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<Out> out(n);
    HIP_OK(hipMemcpy(out.data(), dout, n * sizeof(Out), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(drows));
    HIP_OK(hipFree(dout));
    for (size_t i = 0; i < n; ++i) {
        const int o = rows[i].op;
        if (o == OP_IS_ZERO || o == OP_IS_ZERO_SM2) {
            printf("%x\n", out[i].v[10]);
        } else {
            const int cnt = o == OP_TO_FE26 ? 10 : 16;
            for (int j = 0; j < cnt; ++j) printf("%x%c", out[i].v[j], j == cnt - 1 ? '\n' : ',');
        }
    }
    return 0;
}
