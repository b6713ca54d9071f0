// triovec.hip -- the lane-trio point operations on a real wave, for tests/test_gpu_trio_ops.py: secp256k1's
// (ec26_trio.h) in lib/triovec, and SM2's (ecp26_trio.h) in lib/triovec_sm2, the same file built with
// -DTRIOVEC_SM2 and the flags of the translation unit those ship in (see the Makefile).  The CPU suite runs
// the trio code as 16 host threads (tests/cpp/trio_test.cpp), where trio::any votes over one row,
// TrioLane's wave masks are 0 (so trio::csel's v_cndmask_b32_dpp path never runs) and dpp_fence is empty;
// here a wave is 4 rows x 5 trios (lanes 3t..3t+2 of a row) plus the phantom lane 15 of each row, __any
// votes over all 64 lanes, and the test chooses which trio of which row meets an exceptional case.
//
// stdin: eight lines "table <x> <y>" first: the affine points 1R..8R of the signed table that trio_window
// and trio_chain_start look up (ten hex limbs each, joined by commas; read and unused by the SM2 build);
// then one TRIO per line,
//   "<op> <k> <X> <Y> <Z> <inf> <X2> <Y2> <Z2> <inf2> <E1> <E2> <E3>"
// with raw limbs: the first operand (Jacobian), the second (affine x, y or Jacobian), and three more
// elements whose meaning the op gives.  Twenty consecutive lines are one wave (row-major: trios 0..4 of
// row 0, then row 1, ...) and name one op; the line count must be a multiple of 80 (blocks of 256 threads,
// four waves).  secp256k1 ops:
//   dbl dbl_zz madd (trio_madd<true>) add
//   madd_zz       E1 = ZZ = Z^2 of the first operand
//   window        k = the digit d in -8..8 (trio_dbln<0..3>, trio_maddq_zz with keep = (d == 0))
//   chain_start   k = the scalar's top word
//   scale         trio_scale_xz with K = E1, then trio_scale_y with l = E2
//   add_z         trio_add_z; the answer is E
// SM2 ops (coordinates in fp26's Montgomery form):
//   dbl_sm2 madd_sm2 (trio_madd_sm2<true>)
//   dbl_sm2_d     E1 = D = Z^2
//   madd_sm2_d    E1 = D
//   add_sm2_jd    E1 = D, the entry (X2, Y2, Z2) with ZZ = E2, ZZZ = E3
// stdout: one line per trio, after trio_to_jac / trio_to_jac_sm2 (window: trio_acc_to first):
// "X Y Z inf E", E = lane 0's ZZ of dbl_zz, lane 0's D of the _d ops, lane 2's Z3 of add_z, else zeros.
// One launch, blocks of 256 threads; every HIP call is checked and the first error ends the program with
// a nonzero status.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../csrc/ecp26_trio.h"

using namespace bcosgpu;

enum Op : int {
    OP_DBL, OP_DBL_ZZ, OP_MADD, OP_MADD_ZZ, OP_ADD, OP_WINDOW, OP_CHAIN_START, OP_SCALE, OP_ADD_Z,
    OP_DBL_SM2, OP_DBL_SM2_D, OP_MADD_SM2_D, OP_ADD_SM2_JD, OP_MADD_SM2, OP_COUNT
};
static const char* kOps[OP_COUNT] = {"dbl", "dbl_zz", "madd", "madd_zz", "add", "window", "chain_start", "scale", "add_z",
                                     "dbl_sm2", "dbl_sm2_d", "madd_sm2_d", "add_sm2_jd", "madd_sm2"};
#ifdef TRIOVEC_SM2
static bool op_here(int op) { return op >= OP_DBL_SM2; }
#else
static bool op_here(int op) { return op < OP_DBL_SM2; }
#endif

struct Trio {
    int op, inf, inf2;
    uint32_t k;
    uint32_t p[3][10], q[3][10], e[3][10];
};
struct Out {
    uint32_t v[4][10];  // X, Y, Z, extra
    int inf;
};
struct Table {
    uint32_t e[8][2][10];
};

template <class E>
__device__ __forceinline__ void load(E& r, const uint32_t* v) {
#pragma unroll
    for (int i = 0; i < 10; ++i) r.v[i] = v[i];
}

#ifndef TRIOVEC_SM2
// the operand as a TrioPt: S1 = (X | Y | Y), X and Z on lane 2 only (lanes 0 and 1 hold zeros there: the
// header calls them don't-care, and a read from the wrong lane then shows)
__device__ __forceinline__ void load_pt(TrioPt& P, const uint32_t (*c)[10], bool inf, const TrioLane& T) {
    fe26 X, Y, Z, z;
    load(X, c[0]);
    load(Y, c[1]);
    load(Z, c[2]);
    fe26_zero(z);
    trio::sel(P.S1, T.r0, X, Y);
    trio::sel(P.Xs, T.r2, X, z);
    trio::sel(P.Zs, T.r2, Z, z);
    P.inf = inf;
}
// the signed table point +-|d| R (d = 0: any entry), y negated for d < 0 (m 2)
struct TabEntry {
    const Table* tab;
    __device__ __forceinline__ void operator()(Aff26& S, int d) const {
        const int m = ((d < 0 ? -d : d) - 1) & 7;
        load(S.x, tab->e[m][0]);
        load(S.y, tab->e[m][1]);
        fe26 ny;
        fe26_neg<2>(ny, S.y);
        fe26_cmov(S.y, ny, d < 0);
    }
};

__device__ __forceinline__ void run(int op, const Trio& me, const Table* tab, const TrioLane& T, uint32_t (&X)[10],
                                    uint32_t (&Y)[10], uint32_t (&Z)[10], uint32_t (&E)[10], bool& inf, bool& e_lane2) {
    TrioPt P, Q, R;
    load_pt(P, me.p, me.inf != 0, T);
    load_pt(Q, me.q, me.inf2 != 0, T);
    Aff26 A;
    load(A.x, me.q[0]);
    load(A.y, me.q[1]);
    fe26 extra, e1, e2;
    fe26_zero(extra);
    load(e1, me.e[0]);
    load(e2, me.e[1]);
    const TabEntry entry{tab};
    switch (op) {
        case OP_DBL: trio_dbl(P, T); R = P; break;
        case OP_DBL_ZZ: trio_dbl_zz(P, extra, T); R = P; break;
        case OP_MADD: trio_madd<true>(R, P, A, T); break;
        case OP_MADD_ZZ: trio_madd_zz(R, P, e1, A, T); break;
        case OP_ADD: trio_add(R, P, Q, T); break;
        case OP_WINDOW: {
            TrioAcc acc;
            trio_acc_from(acc, P);
            trio_window(acc, static_cast<int>(me.k), entry, T);
            trio_acc_to(R, acc, T);
            break;
        }
        case OP_CHAIN_START: trio_chain_start(R, me.k, entry, T); break;
        case OP_SCALE:
            trio_scale_xz(R, P, e1, T);
            trio_scale_y(R, e2, T);
            break;
        case OP_ADD_Z:
            trio_add_z(extra, P, Q, T);
            R = P;
            e_lane2 = true;
            break;
        default: trio_set_inf(R); break;
    }
    Jac26 J;
    trio_to_jac(J, R, T);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        X[i] = J.X.v[i];
        Y[i] = J.Y.v[i];
        Z[i] = J.Z.v[i];
        E[i] = extra.v[i];
    }
    inf = J.inf;
}
#else
// the operand as a TrioPtP: P1 = (Z | Y | Y), Q1 = (Z | Y | Z), Xr = (X | X | 0)
__device__ __forceinline__ void load_pt(TrioPtP& P, const uint32_t (*c)[10], bool inf, const TrioLane& T) {
    fp26 X, Y, Z, z;
    load(X, c[0]);
    load(Y, c[1]);
    load(Z, c[2]);
    fp26_zero(z);
    trio::sel(P.P1, T.r0, Z, Y);
    trio::sel(P.Q1, T.r1, Y, Z);
    trio::sel(P.Xr, T.r2, z, X);
    P.inf = inf;
}

__device__ __forceinline__ void run(int op, const Trio& me, const Table*, const TrioLane& T, uint32_t (&X)[10],
                                    uint32_t (&Y)[10], uint32_t (&Z)[10], uint32_t (&E)[10], bool& inf, bool&) {
    TrioPtP P, R;
    load_pt(P, me.p, me.inf != 0, T);
    AffP26 A;
    load(A.x, me.q[0]);
    load(A.y, me.q[1]);
    fp26 extra, d, z;
    fp26_zero(extra);
    fp26_zero(z);
    load(d, me.e[0]);
    trio::sel(d, T.r0, d, z);  // D lives on lane 0
    switch (op) {
        case OP_DBL_SM2: trio_dbl_sm2(P, T); R = P; break;
        case OP_DBL_SM2_D:
            trio_dbl_sm2_d(P, d, T);
            R = P;
            fp26_copy(extra, d);
            break;
        case OP_MADD_SM2_D: trio_madd_sm2_d(R, extra, P, d, A, T); break;
        case OP_ADD_SM2_JD: {
            JacEntP26 Q;
            load(Q.X, me.q[0]);
            load(Q.Y, me.q[1]);
            load(Q.Z, me.q[2]);
            load(Q.ZZ, me.e[1]);
            load(Q.ZZZ, me.e[2]);
            trio_add_sm2_jd(R, extra, P, d, Q, T);
            break;
        }
        case OP_MADD_SM2: trio_madd_sm2<true>(R, P, A, T); break;
        default: trio_set_inf_sm2(R); break;
    }
    JacP26 J;
    trio_to_jac_sm2(J, R, T);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        X[i] = J.X.v[i];
        Y[i] = J.Y.v[i];
        Z[i] = J.Z.v[i];
        E[i] = extra.v[i];
    }
    inf = J.inf;
}
#endif

__global__ void __launch_bounds__(256) k_trios(const Trio* trios, const Table* tab, Out* out) {
    const int lane = threadIdx.x & 63, row = lane >> 4, pos = lane & 15;
    const int wave = 4 * blockIdx.x + (threadIdx.x >> 6);
    const TrioLane T(lane);
    // the phantom lane rides with trio 4's inputs; its results are not stored
    const int slot = pos == 15 ? 4 : pos / 3;
    const Trio& me = trios[20 * wave + 5 * row + slot];
    const int op = __builtin_amdgcn_readfirstlane(me.op);
    uint32_t X[10], Y[10], Z[10], E[10];
    bool inf = false, e_lane2 = false;
    run(op, me, tab, T, X, Y, Z, E, inf, e_lane2);
    Out& o = out[20 * wave + 5 * row + slot];
    if (T.r0 && pos != 15) {
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            o.v[0][i] = X[i];
            o.v[1][i] = Y[i];
            o.v[2][i] = Z[i];
        }
        o.inf = inf ? 1 : 0;
    }
    if ((e_lane2 ? T.r2 : T.r0) && pos != 15) {
#pragma unroll
        for (int i = 0; i < 10; ++i) o.v[3][i] = E[i];
    }
}

#define HIP_OK(call)                                                            \
    do {                                                                        \
        const hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) {                                                 \
            fprintf(stderr, "triovec: %s: %s\n", #call, hipGetErrorString(e_)); \
            return 1;                                                           \
        }                                                                       \
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

int main() {
    Table tab;
    char w[13][128];
    for (int i = 0; i < 8; ++i) {
        if (scanf("%127s %127s %127s", w[0], w[1], w[2]) != 3 || strcmp(w[0], "table") != 0 ||
            !parse_limbs(w[1], tab.e[i][0]) || !parse_limbs(w[2], tab.e[i][1])) {
            fprintf(stderr, "triovec: table line %d\n", i + 1);
            return 2;
        }
    }
    std::vector<Trio> trios;
    while (scanf("%127s %127s %127s %127s %127s %127s %127s %127s %127s %127s %127s %127s %127s", w[0], w[1], w[2], w[3],
                 w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12]) == 13) {
        Trio t;
        t.op = -1;
        for (int i = 0; i < OP_COUNT; ++i)
            if (strcmp(w[0], kOps[i]) == 0 && op_here(i)) t.op = i;
        t.k = static_cast<uint32_t>(strtoll(w[1], nullptr, 0));
        t.inf = atoi(w[5]);
        t.inf2 = atoi(w[9]);
        if (t.op < 0 || !parse_limbs(w[2], t.p[0]) || !parse_limbs(w[3], t.p[1]) || !parse_limbs(w[4], t.p[2]) ||
            !parse_limbs(w[6], t.q[0]) || !parse_limbs(w[7], t.q[1]) || !parse_limbs(w[8], t.q[2]) ||
            !parse_limbs(w[10], t.e[0]) || !parse_limbs(w[11], t.e[1]) || !parse_limbs(w[12], t.e[2])) {
            fprintf(stderr, "triovec: bad line %zu (or an op of the other build): %s\n", trios.size() + 1, w[0]);
            return 2;
        }
        if (trios.size() % 20 != 0 && trios.back().op != t.op) {
            fprintf(stderr, "triovec: line %zu: the twenty trios of a wave must name one op\n", trios.size() + 1);
            return 2;
        }
        trios.push_back(t);
    }
    if (trios.size() % 80 != 0) {
        fprintf(stderr, "triovec: %zu trios: not whole blocks of four waves\n", trios.size());
        return 2;
    }
    if (trios.empty()) return 0;
    const size_t n = trios.size();
    Trio* dt = nullptr;
    Table* dtab = nullptr;
    Out* dout = nullptr;
    HIP_OK(hipMalloc(&dt, n * sizeof(Trio)));
    HIP_OK(hipMalloc(&dtab, sizeof(Table)));
    HIP_OK(hipMalloc(&dout, n * sizeof(Out)));
    HIP_OK(hipMemcpy(dt, trios.data(), n * sizeof(Trio), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dtab, &tab, sizeof(Table), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xff, n * sizeof(Out)));
    hipLaunchKernelGGL(k_trios, dim3(static_cast<unsigned>(n / 80)), dim3(256), 0, 0, dt, dtab, dout);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<Out> out(n);
    HIP_OK(hipMemcpy(out.data(), dout, n * sizeof(Out), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(dt));
    HIP_OK(hipFree(dtab));
    HIP_OK(hipFree(dout));
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 4; ++c) {
            for (int j = 0; j < 10; ++j) printf("%x%c", out[i].v[c][j], j == 9 ? ' ' : ',');
            if (c == 2) printf("%d ", out[i].inf);
        }
        printf("\n");
    }
    return 0;
}
