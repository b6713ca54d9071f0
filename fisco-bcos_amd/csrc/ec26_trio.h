// ec26_trio.h -- secp256k1 point doubling and mixed addition split over a lane TRIO: three adjacent
// lanes of one wave (positions 3t, 3t + 1, 3t + 2 of a 16-lane DPP row; position 15 is a phantom
// role-0 lane whose results are never used) cooperate on ONE point, each lane computing one of the
// independent field multiplications of a dependency level.  Operands are routed between the lanes of
// a trio by DPP row shifts (row_shr / row_shl by 1 or 2) and per-role selects, so a level costs one
// multiplication of latency and no barrier and no LDS round trip -- the wave-pair split of
// coop26_dbl / coop26_madd (ecc_coop.hip) paid a __syncthreads and an LDS write + read per level.
//
// Every lane executes the same instruction stream (a wave has one program counter): a level is one
// fe26_mul / fe26_sqr whose operands are chosen per role, so the split must give all roles the same
// operation at each level.  The formulas are CurveK1x's (ec26.h) with the same magnitudes:
//
//   dbl (3 levels):  L1  A = X^2          | B = Y^2            | B = Y^2   (redundant)
//                    L2  F = (3A)^2       | C = B^2            | XB = X B
//                    L3  --               | E (D - X3)         | Y Z       (lane 1 gathers E, F, XB)
//                    D = 4 XB, X3 = F - 2D, Y3 = E (D - X3) - 8C, Z3 = 2 Y Z
//   madd (5 levels): L1  Z^2              | y2 Z               | Z^2
//                    L2  U2 = x2 Z^2      | S2 = y2 Z Z^2      | U2
//                    L3  HH = H^2         | rr^2               | Z H       (H = U2 - X, rr = S2 - Y)
//                    L4  J = H I          | --                 | V = X I   (I = 4 HH)
//                    L5  rr (V - X3)      | Y J                | --
//                    X3 = 4 rr^2 - J - 2V, Y3 = 2 (rr (V - X3) - Y J), Z3 = 2 Z H
//
// A point lives in the trio as TrioPt: S1 = (X | Y | Y) (the first doubling level's operand), Xs = X
// and Zs = Z on lane 2 (lanes 0 and 1 hold don't-care values there), inf on every lane.  Magnitudes:
// dbl -> (10, 10, 2), madd -> (9, 6, 2), as CurveK1x.
#pragma once
#include <type_traits>
#include "ec26.h"

#ifndef TRIO_DUMP  // tools/triobench.hip defines it to dump the addition's per-level values
#define TRIO_DUMP(slot, a) ((void)0)
#endif

namespace bcosgpu {

struct TrioPt {
    fe26 S1, Xs, Zs;
    bool inf;
};

// lane role inside its trio, the three role predicates and (device) their wave masks for
// v_cndmask_b32_dpp (n* = complements)
struct TrioLane {
    bool r0, r1, r2;
    uint64_t m0, m1, m2, n0, n1, n2;
    F26_HD explicit TrioLane(int lane) {
        const int role = (lane & 15) % 3;
        r0 = role == 0;
        r1 = role == 1;
        r2 = role == 2;
#if defined(__HIP_DEVICE_COMPILE__)
        m0 = __builtin_amdgcn_ballot_w64(r0);
        m1 = __builtin_amdgcn_ballot_w64(r1);
        m2 = __builtin_amdgcn_ballot_w64(r2);
#else
        m0 = m1 = m2 = 0;
#endif
        n0 = ~m0;
        n1 = ~m1;
        n2 = ~m2;
    }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// host emulation of a DPP row (tests/cpp/trio_test.cpp runs the 16 lanes of a row as threads)
uint32_t trio_emu_dpp(uint32_t x, int ctrl);
bool trio_emu_any(bool b);
#endif

namespace trio {
// DPP fetches inside a 16-lane row: L1 / L2 = the value of lane i - 1 / i - 2 (row_shr), R1 / R2 = of
// lane i + 1 / i + 2 (row_shl); out-of-row sources read 0 (bound_ctrl), which only phantom lanes see
template <int CTRL>
F26_HD uint32_t dpp(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(x), CTRL, 0xf, 0xf, true));
#else
    return trio_emu_dpp(x, CTRL);
#endif
}
F26_HD bool any(bool b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(b);
#else
    return trio_emu_any(b);
#endif
}
constexpr int kL1 = 0x111, kL2 = 0x112, kR1 = 0x101, kR2 = 0x102;

// the magnitude of a fetched element travels with it in the checking build (a phantom lane's zero
// reads as magnitude 1)
#ifdef FE26_CHECK
template <int CTRL>
F26_HD int mdpp(int m) {
    const int r = static_cast<int>(dpp<CTRL>(static_cast<uint32_t>(m)));
    return r ? r : 1;
}
#endif

template <int CTRL, class E>
F26_HD void fdpp(E& r, const E& a) {
#pragma unroll
    for (int i = 0; i < 10; ++i) r.v[i] = dpp<CTRL>(a.v[i]);
    F26_SETM(r, mdpp<CTRL>(a.m));
}
// A DPP read needs two wait states after the VALU write of its source VGPR (gfx9 rule).  The compiler
// pads its own code, but not the boundary after an inline-asm block (fe26_mul_asm / fe26_sqr_asm end
// with VALU writes of their result limbs; fp26_mul_asm / fp26_sqr_asm likewise), so every product a
// lane may fetch goes through these: the
// s_nop names the limbs as in/out operands, so any later DPP read of them is ordered after it.
template <class E>
F26_HD void dpp_fence(E& r) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_nop 1"
                 : "+v"(r.v[0]), "+v"(r.v[1]), "+v"(r.v[2]), "+v"(r.v[3]), "+v"(r.v[4]), "+v"(r.v[5]),
                   "+v"(r.v[6]), "+v"(r.v[7]), "+v"(r.v[8]), "+v"(r.v[9]));
#else
    (void)r;
#endif
}
F26_HD void mul(fe26& r, const fe26& a, const fe26& b) {
    fe26_mul(r, a, b);
    dpp_fence(r);
}
F26_HD void sqr(fe26& r, const fe26& a) {
    fe26_sqr(r, a);
    dpp_fence(r);
}
template <class E>
F26_HD void sel(E& r, bool c, const E& a, const E& b) {
#pragma unroll
    for (int i = 0; i < 10; ++i) r.v[i] = c ? a.v[i] : b.v[i];
    F26_SETM(r, c ? a.m : b.m);
}
// c ? a : (d ? DPP<C1>(b) : DPP<C2>(b))
template <int C1, int C2, class E>
F26_HD void sel_dpp2(E& r, bool c, const E& a, bool d, const E& b) {
#ifdef FE26_CHECK
    const int m1 = mdpp<C1>(b.m), m2 = mdpp<C2>(b.m);
#endif
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t x = dpp<C1>(b.v[i]), y = dpp<C2>(b.v[i]);
        r.v[i] = c ? a.v[i] : (d ? x : y);
    }
    F26_SETM(r, c ? a.m : d ? m1 : m2);
}
// r = c ? a : DPP<CTRL>(b) in one v_cndmask_b32_dpp per limb (the DPP combiner is off, so the fold
// is written out): VCC = cm, the wave mask of c; s_nop 1 gives the DPP source its two wait states
// after a VALU write (SALU -> VALU reads of VCC need none).  Five limbs per block (operand limit).
// The mask is an input bound to VCC itself (a register variable): the compiler copies cm there in front
// of a block only where VCC does not hold it already, so blocks of one role that follow each other share
// one s_mov_b64 (the three role masks and their complements are kernel-long SGPR pairs).  The ten limbs'
// second block carries no s_nop of its own: the first block's covers it unless the compiler puts a VALU
// write of a limb of b between the two, which tools/hazard_check.py (tests/test_hazards.py) would find in
// the built code.
#define TRIO_CSEL_INS(D, S0, S1, CTL) "v_cndmask_b32_dpp %" #D ", %" #S0 ", %" #S1 ", vcc " CTL \
    " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define TRIO_CSEL5(NOP, CTL, r, a, b, o, cm)                                                            \
    asm volatile(NOP TRIO_CSEL_INS(0, 10, 5, CTL) TRIO_CSEL_INS(1, 11, 6, CTL)                         \
                 TRIO_CSEL_INS(2, 12, 7, CTL) TRIO_CSEL_INS(3, 13, 8, CTL) TRIO_CSEL_INS(4, 14, 9, CTL)      \
                 : "=&v"((r).v[o]), "=&v"((r).v[o + 1]), "=&v"((r).v[o + 2]), "=&v"((r).v[o + 3]),       \
                   "=&v"((r).v[o + 4])                                                                  \
                 : "v"((a).v[o]), "v"((a).v[o + 1]), "v"((a).v[o + 2]), "v"((a).v[o + 3]), "v"((a).v[o + 4]), \
                   "v"((b).v[o]), "v"((b).v[o + 1]), "v"((b).v[o + 2]), "v"((b).v[o + 3]), "v"((b).v[o + 4]), \
                   "s"(cm))
#define TRIO_CSEL10(CTL, r, a, b, cm)                    \
    register uint64_t vcc_cm asm("vcc") = (cm);          \
    TRIO_CSEL5("s_nop 1\n\t", CTL, r, a, b, 0, vcc_cm); \
    TRIO_CSEL5("", CTL, r, a, b, 5, vcc_cm)
template <int CTRL, class E>
F26_HD void csel(E& r, bool c, uint64_t cm, const E& a, const E& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)c;
    E t;
    if constexpr (CTRL == kL1) {
        TRIO_CSEL10("row_shr:1", t, a, b, cm);
    } else if constexpr (CTRL == kL2) {
        TRIO_CSEL10("row_shr:2", t, a, b, cm);
    } else if constexpr (CTRL == kR1) {
        TRIO_CSEL10("row_shl:1", t, a, b, cm);
    } else {
        static_assert(CTRL == kR2, "csel: row shift by 1 or 2");
        TRIO_CSEL10("row_shl:2", t, a, b, cm);
    }
    r = t;
#else
    (void)cm;
#ifdef FE26_CHECK
    const int mb = mdpp<CTRL>(b.m);
#endif
    E t;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t x = dpp<CTRL>(b.v[i]);
        t.v[i] = c ? a.v[i] : x;
    }
    F26_SETM(t, c ? a.m : mb);
    r = t;
#endif
}
F26_HD uint32_t bdpp_from(uint32_t f, const TrioLane& T, int src) {
    // the value of f held by role src of this lane's trio
    const uint32_t l1 = dpp<kL1>(f), l2 = dpp<kL2>(f), r1 = dpp<kR1>(f), r2 = dpp<kR2>(f);
    if (src == 0) return T.r0 ? f : T.r1 ? l1 : l2;
    if (src == 1) return T.r1 ? f : T.r0 ? r1 : l1;
    return T.r2 ? f : T.r1 ? r1 : r2;
}
}  // namespace trio

F26_HD void trio_from_aff(TrioPt& P, const Aff26& Q, const TrioLane& T) {
    trio::sel(P.S1, T.r0, Q.x, Q.y);
    fe26_copy(P.Xs, Q.x);
    fe26_one(P.Zs);
    P.inf = false;
}
F26_HD void trio_set_inf(TrioPt& P) {
    fe26_zero(P.S1);
    fe26_zero(P.Xs);
    fe26_zero(P.Zs);
    P.inf = true;
}
F26_HD void trio_cmov(TrioPt& P, const TrioPt& Q, bool c) {
    fe26_cmov(P.S1, Q.S1, c);
    fe26_cmov(P.Xs, Q.Xs, c);
    fe26_cmov(P.Zs, Q.Zs, c);
    P.inf = c ? Q.inf : P.inf;
}
// the full Jacobian point on every lane of the trio (X from lane 0, Y from lane 1, Z from lane 2)
F26_HD void trio_to_jac(Jac26& J, const TrioPt& P, const TrioLane& T) {
    using namespace trio;
    sel_dpp2<kL1, kL2>(J.X, T.r0, P.S1, T.r1, P.S1);   // lane 1 <- lane 0, lane 2 <- lane 0
    sel_dpp2<kR1, kL1>(J.Y, T.r1, P.S1, T.r0, P.S1);   // lane 0 <- lane 1, lane 2 <- lane 1
    sel_dpp2<kR1, kR2>(J.Z, T.r2, P.Zs, T.r1, P.Zs);   // lane 1 <- lane 2, lane 0 <- lane 2
    J.inf = P.inf;
}

// P <- 2P  (X, Y <= 10, Z <= 16 -> (10, 10, 2))
F26_HD void trio_dbl(TrioPt& P, const TrioLane& T) {
    using namespace trio;
    fe26 o1, T2, S2, o2, F, XB, D, X3, W, P3, Q3, o3, C8, Y3, t;
    sqr(o1, P.S1);                                       // (A | B | B)                 m 1
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t x3 = (o1.v[i] << 1) + o1.v[i];  // one v_lshl_add_u32
        T2.v[i] = T.r0 ? x3 : o1.v[i];                  // (3A | B | B)               m <= 3
    }
    F26_SETM(T2, T.r0 ? 3 : 1);
    sel(S2, T.r2, P.Xs, T2);                             // (3A | B | X)                m <= 10
    mul(o2, S2, T2);                                     // (F | C | XB)
    fdpp<kL1>(F, o2);                                    // lane 1: F                   m 1
    fdpp<kR1>(XB, o2);                                   // lane 1: X B                 m 1
    fe26_mul_int<4>(D, XB);                              // D = 4 X B                   m 4
    fe26_mul_int<2>(t, D);                               //                             m 8
    fe26_sub<9>(X3, F, t);                               // X3 = F - 2D                 m 10
    fe26_sub<11>(W, D, X3);                              // D - X3                      m 15
    csel<kL1>(P3, T.r2, T.m2, P.S1, T2);                 // lane 1: E = 3A (lane 0), lane 2: Y
    sel(Q3, T.r2, P.Zs, W);                              // lane 1: D - X3, lane 2: Z
    mul(o3, P3, Q3);                                     // (- | E (D - X3) | Y Z)
    fe26_mul_int<8>(C8, o2);                             // lane 1: 8C                  m 8
    fe26_sub<9>(Y3, o3, C8);                             // lane 1: Y3                  m 10
    fe26_mul_int<2>(P.Zs, o3);                           // lane 2: Z3 = 2 Y Z          m 2
    // next state: S1 = (X3 | Y3 | Y3) from lane 1, Xs = X3 on lane 2
    csel<kL1>(t, T.r1, T.m1, Y3, Y3);                    // lanes 1, 2: Y3 of lane 1
    csel<kR1>(P.S1, !T.r0, T.n0, t, X3);                 // lane 0: X3 of lane 1
    fdpp<kL1>(P.Xs, X3);                                 // lane 2 <- X3 of lane 1
}

// R <- P + Q, Q affine (x, y <= 2) and never infinity; P: X, Y <= 10, Z <= 16 -> (9, 6, 2).  The
// exceptional cases are those of CurveK1x::madd: P = Q doubles (computed on lane 2, which holds all of
// P), P = -Q gives infinity, P = infinity gives Q.  EXC = false drops the P = +-Q tests for callers
// that exclude those cases (trio_glv_chain in ecc_coop.hip states why a GLV chain does).
template <bool EXC = true>
F26_HD void trio_madd(TrioPt& R, const TrioPt& P, const Aff26& Q, const TrioLane& T) {
    using namespace trio;
    fe26 Zb, P1, o1, P2, Q2, o2, Xl, h, P3, o3, HHx, I, P4, o4, R2, V, X3, W, P5, Q5, o5, Y3, t;
    sel_dpp2<kR1, kR2>(Zb, T.r2, P.Zs, T.r1, P.Zs);     // Z on every lane
    sel(P1, T.r1, Q.y, Zb);
    mul(o1, P1, Zb);                                     // (Z1Z1 | y2 Z | Z1Z1)
    TRIO_DUMP(0, o1);
    sel(P2, T.r1, o1, Q.x);
    fdpp<kR1>(Q2, o1);
    sel(Q2, T.r1, Q2, o1);                               // lane 1: Z1Z1 of lane 2
    mul(o2, P2, Q2);                                     // (U2 | S2 | U2)
    TRIO_DUMP(1, o2);
    sel(Xl, T.r2, P.Xs, P.S1);                           // (X | Y | X)                 m <= 10
    fe26_sub<11>(h, o2, Xl);                             // (H | rr | H)                m 12
    sel(P3, T.r2, Zb, h);
    mul(o3, P3, h);                                      // (HH | rr^2 | Z H)
    TRIO_DUMP(2, h);
    TRIO_DUMP(3, o3);
    fdpp<kL2>(HHx, o3);
    sel(HHx, T.r2, HHx, o3);                             // lanes 0, 2: HH
    fe26_mul_int<4>(I, HHx);                             // I = 4 HH                    m 4
    sel(P4, T.r2, P.Xs, h);
    mul(o4, P4, I);                                      // (J | - | V)
    TRIO_DUMP(4, o4);
    // lane 0: X3 = 4 rr^2 - J - 2V and V - X3
    fdpp<kR1>(R2, o3);
    fe26_mul_int<4>(R2, R2);                             // 4 rr^2                      m 4
    fdpp<kR2>(V, o4);                                    // V of lane 2                 m 1
    fe26_sub<2>(X3, R2, o4);                             //                             m 6
    fe26_mul_int<2>(t, V);                               //                             m 2
    fe26_sub<3>(X3, X3, t);                              // X3                          m 9
    fe26_sub<10>(W, V, X3);                              // V - X3                      m 11
    fdpp<kR1>(P5, h);
    sel(P5, T.r0, P5, P.S1);                             // lane 0: rr (lane 1), lane 1: Y   m 12
    fdpp<kL1>(Q5, o4);
    sel(Q5, T.r0, W, Q5);                                // lane 0: V - X3, lane 1: J of lane 0
    mul(o5, P5, Q5);                                     // (rr (V - X3) | Y J | -)
    TRIO_DUMP(5, o5);
    TRIO_DUMP(6, X3);
    fdpp<kR1>(t, o5);
    fe26_sub<2>(Y3, o5, t);                              //                             m 3
    fe26_mul_int<2>(Y3, Y3);                             // lane 0: Y3                  m 6
    TRIO_DUMP(7, Y3);
    TrioPt O;
    sel_dpp2<kL1, kL2>(O.S1, T.r0, X3, T.r1, Y3);      // (X3 | Y3 | Y3) from lane 0
    fdpp<kL2>(O.Xs, X3);                                 // lane 2 <- X3 of lane 0
    fe26_mul_int<2>(O.Zs, o3);                           // lane 2: Z3 = 2 Z H          m 2
    O.inf = false;
    if constexpr (EXC) {  // exceptional cases (flags shared across the trio)
        const uint32_t zf = fe26_is_zero(h) ? 1u : 0u;
        const bool hz = bdpp_from(zf, T, 0) != 0u && !P.inf;
        const bool rz = bdpp_from(zf, T, 1) != 0u;
        if (any(hz && rz)) {                             // P == Q: double on lane 2 (rare)
            Jac26 A, D;
            fe26_copy(A.X, P.Xs);
            fe26_copy(A.Y, P.S1);
            fe26_copy(A.Z, P.Zs);
            A.inf = P.inf;
            CurveK1x::dbl(D, A);
            TrioPt Dt;
            sel_dpp2<kR2, kR1>(Dt.S1, T.r2, D.Y, T.r0, D.X);  // lane 0 <- X, lane 1 <- Y of lane 2
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const uint32_t y = dpp<kR1>(D.Y.v[i]);
                Dt.S1.v[i] = T.r1 ? y : Dt.S1.v[i];
            }
            F26_SETM(Dt.S1, 10);
            fe26_copy(Dt.Xs, D.X);
            fe26_copy(Dt.Zs, D.Z);
            Dt.inf = false;
            trio_cmov(O, Dt, hz && rz);
        }
        if (hz && !rz) O.inf = true;                     // P == -Q
    }
    if (P.inf) trio_from_aff(O, Q, T);
    R = O;
}

// P <- 2P as trio_dbl, and ZZ = Z3^2 on lane 0 for the mixed addition that follows (trio_madd_zz): the
// first level's redundant lane-2 square becomes Z^2 (lane 2's B comes from lane 1), and the third
// level's idle lane 0 computes B Z^2, so Z3^2 = (2 Y Z)^2 = 4 B Z^2 costs no product level.
// (X, Y <= 10, Z <= 16 -> (10, 10, 2), ZZ m 4)
F26_HD void trio_dbl_zz(TrioPt& P, fe26& ZZ, const TrioLane& T) {
    using namespace trio;
    fe26 S0, o1, T2, S2, o2, F, XB, D, X3, W, P3, Q3, o3, C8, Y3, t;
    sel(S0, T.r2, P.Zs, P.S1);                           // (X | Y | Z)
    sqr(o1, S0);                                         // (A | B | Z^2)                m 1
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t x3 = (o1.v[i] << 1) + o1.v[i];  // one v_lshl_add_u32
        T2.v[i] = T.r0 ? x3 : o1.v[i];                  // (3A | B | Z^2)
    }
    F26_SETM(T2, T.r0 ? 3 : 1);
    csel<kL1>(T2, !T.r2, T.n2, T2, o1);                  // lane 2: B of lane 1 -> (3A | B | B)
    sel(S2, T.r2, P.Xs, T2);                             // (3A | B | X)                 m <= 10
    mul(o2, S2, T2);                                     // (F | C | XB)
    fdpp<kL1>(F, o2);                                    // lane 1: F                    m 1
    fdpp<kR1>(XB, o2);                                   // lane 1: X B                  m 1
    fe26_mul_int<4>(D, XB);                              // D = 4 X B                    m 4
    fe26_mul_int<2>(t, D);                               //                              m 8
    fe26_sub<9>(X3, F, t);                               // X3 = F - 2D                  m 10
    fe26_sub<11>(W, D, X3);                              // D - X3                       m 15
    csel<kL1>(P3, T.r2, T.m2, P.S1, T2);                 // lane 1: E = 3A (lane 0), lane 2: Y
    csel<kR1>(P3, !T.r0, T.n0, P3, o1);                  // lane 0: B (lane 1)
    sel(Q3, T.r2, P.Zs, W);                              // lane 1: D - X3, lane 2: Z
    csel<kR2>(Q3, !T.r0, T.n0, Q3, o1);                  // lane 0: Z^2 (lane 2)
    mul(o3, P3, Q3);                                     // (B Z^2 | E (D - X3) | Y Z)
    fe26_mul_int<4>(ZZ, o3);                             // lane 0: Z3^2 = 4 B Z^2       m 4
    fe26_mul_int<8>(C8, o2);                             // lane 1: 8C                   m 8
    fe26_sub<9>(Y3, o3, C8);                             // lane 1: Y3                   m 10
    fe26_mul_int<2>(P.Zs, o3);                           // lane 2: Z3 = 2 Y Z           m 2
    csel<kL1>(t, T.r1, T.m1, Y3, Y3);                    // lanes 1, 2: Y3 of lane 1
    csel<kR1>(P.S1, !T.r0, T.n0, t, X3);                 // lane 0: X3 of lane 1
    fdpp<kL1>(P.Xs, X3);                                 // lane 2 <- X3 of lane 1
}

// R <- P + Q, Q affine, given ZZ = Z1^2 on lane 0 (trio_dbl_zz): CurveK1x::madd in 4 product levels
// instead of 5 (the Z1^2 level is gone), without the P = +-Q tests (the GLV chain's additions, see
// trio_glv_chain in ecc_coop.hip); P = infinity gives Q.  X, Y <= 10, Z <= 16, ZZ <= 4; Q <= 2
// -> (9, 6, 2).
//   L1  U2 = x2 ZZ       | T = y2 Z        | --
//   L2  HH = H^2         | S2 = T ZZ       | Z H          (H = U2 - X on lane 0)
//   L3  J = H I          | rr^2            | V = X I      (I = 4 HH, rr = S2 - Y on lane 1)
//   L4  rr (V - X3)      | Y J             | --           (X3 = 4 rr^2 - J - 2V on lane 0)
F26_HD void trio_madd_zz(TrioPt& R, const TrioPt& P, const fe26& ZZ, const Aff26& Q, const TrioLane& T) {
    using namespace trio;
    fe26 P1, Q1, o1, h, P2, Q2, a, b, o2, I, rr, P3, Q3, o3, R2, V, X3, W, P4, Q4, o4, Y3, t;
    sel(P1, T.r1, Q.y, Q.x);                             // (x2 | y2 | x2)
    csel<kR1>(Q1, T.r0, T.m0, ZZ, P.Zs);                 // (ZZ | Z of lane 2 | -)
    mul(o1, P1, Q1);                                     // (U2 | T | -)
    fe26_sub<11>(h, o1, P.S1);                           // lane 0: H = U2 - X           m 12
    sel(P2, T.r1, o1, P.Zs);
    sel(P2, T.r0, h, P2);                                // (H | T | Z)
    fdpp<kL1>(a, ZZ);                                    // lane 1: ZZ
    fdpp<kL2>(b, h);                                     // lane 2: H
    sel(Q2, T.r1, a, b);
    sel(Q2, T.r0, h, Q2);                                // (H | ZZ | H)
    mul(o2, P2, Q2);                                     // (HH | S2 | Z H)
    fe26_mul_int<4>(I, o2);                              // lane 0: I = 4 HH             m 4
    fe26_sub<11>(rr, o2, P.S1);                          // lane 1: rr = S2 - Y          m 12
    sel(P3, T.r1, rr, P.Xs);
    sel(P3, T.r0, h, P3);                                // (H | rr | X)
    fdpp<kL2>(b, I);                                     // lane 2: I
    sel(Q3, T.r1, rr, b);
    sel(Q3, T.r0, I, Q3);                                // (I | rr | I)
    mul(o3, P3, Q3);                                     // (J | rr^2 | V)
    // lane 0: X3 = 4 rr^2 - J - 2V and V - X3
    fdpp<kR1>(R2, o3);
    fe26_mul_int<4>(R2, R2);                             // 4 rr^2                       m 4
    fdpp<kR2>(V, o3);                                    // V of lane 2                  m 1
    fe26_sub<2>(X3, R2, o3);                             //                              m 6
    fe26_mul_int<2>(t, V);                               //                              m 2
    fe26_sub<3>(X3, X3, t);                              // X3                           m 9
    fe26_sub<10>(W, V, X3);                              // V - X3                       m 11
    csel<kR1>(P4, !T.r0, T.n0, P.S1, rr);                // lane 0: rr (lane 1), lane 1: Y   m 12
    csel<kL1>(Q4, T.r0, T.m0, W, o3);                    // lane 0: V - X3, lane 1: J of lane 0
    mul(o4, P4, Q4);                                     // (rr (V - X3) | Y J | -)
    fdpp<kR1>(t, o4);
    fe26_sub<2>(Y3, o4, t);                              //                              m 3
    fe26_mul_int<2>(Y3, Y3);                             // lane 0: Y3                   m 6
    TrioPt O;
    sel_dpp2<kL1, kL2>(O.S1, T.r0, X3, T.r1, Y3);      // (X3 | Y3 | Y3) from lane 0
    fdpp<kL2>(O.Xs, X3);                                 // lane 2 <- X3 of lane 0
    fe26_mul_int<2>(O.Zs, o2);                           // lane 2: Z3 = 2 Z H           m 2
    O.inf = false;
    if (P.inf) trio_from_aff(O, Q, T);
    R = O;
}

// The start of a radix-16 Booth chain over a 128-bit scalar k (top = its highest word): the two top
// digits, d32 = bit 127 and d31 = (bits 124..127) + (bit 123) - 16 d32, weigh 16 d32 + d31 = t =
// (top nibble) + (bit 123) in [0, 16] together.  With t = 2a + b, a = t >> 1 <= 8, b = t & 1:
// acc <- 2 (a R) + b R, the table's a R taken as the accumulator (a = 0: infinity), one doubling and one
// 4-level addition -- 7 product levels where a 5-level addition onto infinity, four doublings and an
// addition took 21.  entry(S, d) gives the signed table point S = +-d R, d in [1, 8] (x, y <= 2; for
// d = 0 any entry).  No P = +-Q case: 2a = +-b only for a = 0, the infinity flag.  -> (10, 10, 2) as a
// window's end (the doubling's bound; the addition's (9, 6, 2) lies inside it), infinity for t = 0; the
// chain goes on at digit 30.
template <class Entry>
F26_HD void trio_chain_start(TrioPt& acc, uint32_t top, const Entry& entry, const TrioLane& T) {
    const uint32_t t = (top >> 28) + ((top >> 27) & 1u);
    const int a = static_cast<int>(t >> 1), b = static_cast<int>(t & 1u);
    Aff26 S;
    TrioPt R;
    fe26 zz;
    entry(S, a);
    trio_from_aff(R, S, T);
    trio_set_inf(acc);
    trio_cmov(acc, R, a != 0);
    trio_dbl_zz(acc, zz, T);
    entry(S, 1);
    trio_madd_zz(R, acc, zz, S, T);
    trio_cmov(acc, R, b != 0);
}

// ------------------------------------------------------------------ the lean window
// A window of a radix-16 chain (four doublings and the addition of a signed table point) with fewer
// routing and small-constant instructions between the same 16 product levels.  What changes against
// trio_dbl x 3, trio_dbl_zz, trio_madd_zz:
//   * the state is TrioAcc: S1 = (X | Y | Y) and Zs = Z on lane 2.  X is not kept on lane 2 between
//     operations: the lane that multiplies by X fetches it from lane 0's S1 inside the select that builds
//     its operand (one v_cndmask_b32_dpp per limb where a DPP move and a select stood);
//   * a doubling returns -2P = (X3, -Y3, Z3) (Z3 up to a power of two that the window settles once): -Y3 = E (X3 - D) + 8C is an addition (one v_lshl_add_u32 per
//     limb) where Y3 = E (D - X3) - 8C adds a multiple of p and subtracts.  The next doubling squares Y and
//     takes Z3 = 2 Y Z on the negated point, so four doublings give +16P; Z3^2 = 4 B Z^2 does not see the sign;
//   * the second level's operand is (3A | 2B | 2B), one v_lshl_add_u32 with a per-lane shift and no select:
//     the level then returns (F | 4C | 2XB), from which X3 = F - 4 (2XB), X3 - D = X3 - 2 (2XB) and
//     8C = 2 (4C) follow without the temporaries D and 2D, all under one added multiple of p;
//   * the addition is the unscaled one, Z3 = Z H, X3 = rr^2 - H^3 - 2 X H^2, Y3 = rr (X H^2 - X3) - Y H^3
//     (another representative of the same point: no 4 HH, 4 rr^2, 2 (...)), with rr and T = y2 Z on lane 2,
//     which holds Y and Z, and Z H on the last level's idle lane;
//   * an infinite accumulator sits behind a wave-uniform branch, and the digit-0 case is one select per
//     limb of S1 and Zs.
struct TrioAcc {
    fe26 S1, Zs;
    bool inf;
};
F26_HD void trio_acc_from(TrioAcc& A, const TrioPt& P) {
    fe26_copy(A.S1, P.S1);
    fe26_copy(A.Zs, P.Zs);
    A.inf = P.inf;
}
F26_HD void trio_acc_to(TrioPt& P, const TrioAcc& A, const TrioLane&) {
    fe26_copy(P.S1, A.S1);
    trio::fdpp<trio::kL2>(P.Xs, A.S1);                   // lane 2 <- X of lane 0
    fe26_copy(P.Zs, A.Zs);
    P.inf = A.inf;
}

// The window's doubling number STEP = 0..3: P <- -2P, and the last one (STEP 3) also gives ZZ = Z3^2 on lane 0
// (m 1) as trio_dbl_zz does.  X, Y, Z <= 16 -> (9, 3, .).
//   L1  A = X^2          | B = Y^2            | B   (STEP 3: Z^2, and 2B comes from lane 1)
//   L2  F = (3A)^2       | 4C = (2B)^2        | x = X 2B             (X from lane 0)
//   L3  -- (3: B Z^2)    | E (X3 - D)         | Y Z                  (E = 3A from lane 0)
//   lane 1: G = F + 8p, X3 = G - 4x, X3 - D = X3 - 2x (limb by limb 8 p_i >= 6 x_i: x is a product, m 1),
//   -Y3 = E (X3 - D) + 2 (4C).
// Z3 = 2 Y Z is not doubled at every step: between the steps Zs holds a power of two times Z, and one shift per
// window stands where four doublings of Z and the scaling of Z^2 stood:
//   step 0  Zs = Z       -> Y Z = Z3 / 2                                (m 1)
//   step 1  Zs = Z / 2   -> Y Z / 2 = Z3 / 4                            (m 1)
//   step 2  Zs = Z / 4   -> 16 (Y Z / 4) = 2 Z3                         (m 16)
//   step 3  Zs = 2 Z     -> Y (2 Z) = Z3 (m 1), and ZZ = B (2 Z)^2 = 4 B Z^2 = Z3^2.
// Only X and Y of steps 0..2 are a point's coordinates with that Zs; trio_window runs the four in order.
template <int STEP>
F26_HD void trio_dbln(TrioAcc& P, fe26& ZZ, const TrioLane& T) {
    using namespace trio;
    static_assert(STEP >= 0 && STEP <= 3, "a window has four doublings");
    constexpr bool WZZ = STEP == 3;
    fe26 S0, o1, T2, S2, o2, F, x, X3, Wn, P3, Q3, o3, Y3, t;
    if constexpr (WZZ) {
        sel(S0, T.r2, P.Zs, P.S1);                       // (X | Y | 2 Z)
        sqr(o1, S0);                                     // (A | B | 4 Z^2)              m 1
    } else {
        sqr(o1, P.S1);                                   // (A | B | B)                  m 1
    }
    const uint32_t sh = T.r0 ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < 10; ++i) T2.v[i] = (o1.v[i] << sh) + o1.v[i];  // one v_lshl_add_u32
    F26_SETM(T2, T.r0 ? 3 : 2);                          // (3A | 2B | 2B)               m <= 3
    if constexpr (WZZ) csel<kL1>(T2, !T.r2, T.n2, T2, T2);  // lane 2: 2B of lane 1
    csel<kL2>(S2, !T.r2, T.n2, T2, P.S1);                // (3A | 2B | X of lane 0)      m <= 16
    mul(o2, S2, T2);                                     // (F | 4C | x)
    fdpp<kL1>(F, o2);                                    // lane 1: F                    m 1
    fdpp<kR1>(x, o2);                                    // lane 1: x = 2 X B            m 1
    F26_REQ(F.m <= 1 && x.m <= 1);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t g = F.v[i] + 8u * f26::plimb(i);
        X3.v[i] = g - (x.v[i] << 2);                     // X3 = F - 2D                  m 9
        Wn.v[i] = X3.v[i] - (x.v[i] << 1);               // X3 - D                       m 9
    }
    F26_SETM(X3, 9);
    F26_SETM(Wn, 9);
    F26_CHK(X3);
    F26_CHK(Wn);
    csel<kL1>(P3, T.r2, T.m2, P.S1, T2);                 // lane 1: E = 3A (lane 0), lane 2: Y
    sel(Q3, T.r2, P.Zs, Wn);                             // lane 1: X3 - D, lane 2: Zs
    if constexpr (WZZ) {
        csel<kR1>(P3, !T.r0, T.n0, P3, o1);              // lane 0: B (lane 1)
        csel<kR2>(Q3, !T.r0, T.n0, Q3, o1);              // lane 0: 4 Z^2 (lane 2)
    }
    mul(o3, P3, Q3);                                     // (- or Z3^2 | E (X3 - D) | Y Zs)
    if constexpr (WZZ) fe26_copy(ZZ, o3);                // lane 0: Z3^2                 m 1
#pragma unroll
    for (int i = 0; i < 10; ++i) Y3.v[i] = (o2.v[i] << 1) + o3.v[i];  // lane 1: -Y3 = o3 + 8C
    F26_SETM(Y3, 3);
    F26_CHK(Y3);
    if constexpr (STEP == 2) fe26_mul_int<16>(P.Zs, o3); // lane 2: 2 Z3                 m 16
    else fe26_copy(P.Zs, o3);                            // lane 2: Z3 / 2, Z3 / 4, Z3   m 1
    csel<kL1>(t, T.r1, T.m1, Y3, Y3);                    // lanes 1, 2: -Y3 of lane 1
    csel<kR1>(P.S1, !T.r0, T.n0, t, X3);                 // lane 0: X3 of lane 1
}

// P <- keep ? P : P + Q, Q affine (x, y <= 2) and never infinity, given ZZ = Z^2 on lane 0 (trio_dbln<3>);
// P = infinity gives Q.  The unscaled mixed addition in the same 4 product levels as trio_madd_zz:
//   L1  U2 = x2 ZZ       | --                 | T = y2 Z
//   L2  HH = H^2         | --                 | S2 = T ZZ            (H = U2 - X on lane 0)
//   L3  J = H HH         | V = X HH           | rr^2                 (rr = S2 - Y on lane 2)
//   L4  rr (V - X3)      | Y J                | Z3 = Z H             (X3 = rr^2 - J - 2V on lane 0)
//   lane 1: Y3 = rr (V - X3) - Y J.
// No P = +-Q test: the argument of trio_glv_chain (ecc_coop.hip) bounds the multiples |K| >= 16 of the
// accumulator and |d| <= 8 of the table point, and is the same for -P as for P; here the accumulator is
// +16 K R in any case, the window's four doublings having restored the sign.
// X, Y <= 10, Z <= 16, ZZ <= 4; Q <= 2 -> (5, 3, 1), or P unchanged.
F26_HD void trio_maddq_zz(TrioAcc& P, const fe26& ZZ, const Aff26& Q, bool keep, const TrioLane& T) {
    using namespace trio;
    fe26 A1, B1, o1, h, A2, B2, o2, rr, t, u, A3, B3, o3, R2, V, s, X3, W, A4, B4, o4, Y3, Z3;
    sel(A1, T.r0, Q.x, Q.y);                             // (x2 | - | y2)
    sel(B1, T.r0, ZZ, P.Zs);                             // (ZZ | - | Z)
    mul(o1, A1, B1);                                     // (U2 | - | T)
    fe26_sub<11>(h, o1, P.S1);                           // lane 0: H = U2 - X           m 12
    sel(A2, T.r0, h, o1);                                // (H | - | T)
    csel<kL2>(B2, !T.r2, T.n2, h, ZZ);                   // (H | - | ZZ of lane 0)
    mul(o2, A2, B2);                                     // (HH | - | S2)
    fe26_sub<11>(rr, o2, P.S1);                          // lane 2: rr = S2 - Y          m 12
    sel(t, T.r0, h, rr);
    csel<kL1>(A3, !T.r1, T.n1, t, P.S1);                 // (H | X of lane 0 | rr)
    sel(u, T.r0, o2, rr);
    csel<kL1>(B3, !T.r1, T.n1, u, o2);                   // (HH | HH of lane 0 | rr)
    mul(o3, A3, B3);                                     // (J | V | rr^2)
    // lane 0: X3 = rr^2 - (J + 2V) and V - X3
    fdpp<kR2>(R2, o3);                                   // rr^2 of lane 2               m 1
    fdpp<kR1>(V, o3);                                    // V of lane 1                  m 1
    F26_REQ(V.m <= 1);
#pragma unroll
    for (int i = 0; i < 10; ++i) s.v[i] = (V.v[i] << 1) + o3.v[i];  // J + 2V           m 3
    F26_SETM(s, 3);
    fe26_sub<4>(X3, R2, s);                              // X3                           m 5
    fe26_sub<6>(W, V, X3);                               // V - X3                       m 7
    csel<kL1>(t, !T.r1, T.n1, W, o3);                    // lane 1: J of lane 0
    csel<kL2>(A4, !T.r2, T.n2, t, h);                    // (V - X3 | J | H of lane 0)
    sel(u, T.r2, P.Zs, P.S1);
    csel<kR2>(B4, !T.r0, T.n0, u, rr);                   // (rr of lane 2 | Y | Z)
    mul(o4, A4, B4);                                     // (rr (V - X3) | Y J | Z H)
    fdpp<kL1>(t, o4);
    fe26_sub<2>(Y3, t, o4);                              // lane 1: Y3                   m 3
    sel(s, T.r0, X3, Y3);
    csel<kL1>(s, !T.r2, T.n2, s, Y3);                    // (X3 | Y3 | Y3 of lane 1)
    fe26_copy(Z3, o4);                                   // lane 2: Z3                   m 1
    if (any(P.inf)) {                                    // infinity + Q = Q (no real signature past its
        fe26 one;                                        // first non-zero digit)
        sel(t, T.r0, Q.x, Q.y);
        fe26_one(one);
        fe26_cmov(s, t, P.inf);
        fe26_cmov(Z3, one, P.inf);
    }
    sel(P.S1, keep, P.S1, s);
    sel(P.Zs, keep, P.Zs, Z3);
    P.inf = keep && P.inf;
}

// One window of a radix-16 Booth chain: acc <- 16 acc + d S, d in [-8, 8]; entry(S, d) gives the signed
// table point as for trio_chain_start.  X, Y, Z <= 16 -> (9, 3, 1) (d = 0) or (5, 3, 1), inside the
// entry contract of the next window, of trio_add and of trio_scale_xz.
template <class Entry>
F26_HD void trio_window(TrioAcc& acc, int d, const Entry& entry, const TrioLane& T) {
    fe26 zz;
    trio_dbln<0>(acc, zz, T);
    trio_dbln<1>(acc, zz, T);
    trio_dbln<2>(acc, zz, T);
    trio_dbln<3>(acc, zz, T);                            // + Z^2 for the addition
    Aff26 S;
    entry(S, d);
    trio_maddq_zz(acc, zz, S, d == 0, T);
}

// R <- P + Q, both Jacobian in trio form (lane 2 holds all of each point at entry); CurveK1x::add's
// formulas, magnitudes and exceptional cases (P = Q doubles on lane 2, P = -Q gives infinity, an
// infinite operand gives the other), 16 products in 6 levels:
//   L1  Z1Z1 = Z1^2      | Z2Z2 = Z2^2     | A = Y1 Z2
//   L2  U2 = X2 Z1Z1     | U1 = X1 Z2Z2    | B = Y2 Z1
//   L3  S2 = B Z1Z1      | S1 = A Z2Z2     | I = (2H)^2          (H = U2 - U1 on lane 2)
//   L4  J = H I          | V = U1 I        | r^2                 (r = 2 (S2 - S1) on lane 2)
//   L5  r (V - X3)       | S1 J            | Z1 Z2               (X3 = r^2 - J - 2V on lane 0)
//   L6  --               | --              | Z1 Z2 H
//   X3 = r^2 - J - 2V, Y3 = r (V - X3) - 2 S1 J, Z3 = 2 Z1 Z2 H.  X, Y, Z <= 16 (both) -> (6, 4, 2).
F26_HD void trio_add(TrioPt& R, const TrioPt& P, const TrioPt& Q, const TrioLane& T) {
    using namespace trio;
    fe26 a, b, P1, Q1, o1, P2, Q2, o2, u2, u1, h, h2, P3, Q3, o3, s2, s1, rr, P4, Q4, o4, rv, X3, W, P5, Q5, o5,
        Y3, Z3, t;
    // L1: lane 0 Z1 Z1 (Z1 of lane 2), lane 1 Z2 Z2 (Z2 of lane 2), lane 2 Y1 Z2
    fdpp<kR2>(a, P.Zs);                                  // lane 0: Z1
    fdpp<kR1>(b, Q.Zs);                                  // lane 1: Z2
    sel(P1, T.r0, a, b);
    sel(P1, T.r2, P.S1, P1);
    sel(Q1, T.r2, Q.Zs, P1);
    mul(o1, P1, Q1);                                     // (Z1Z1 | Z2Z2 | A)            m 1
    // L2: lane 0 X2 Z1Z1, lane 1 X1 Z2Z2 (X1 of lane 0), lane 2 Y2 Z1
    fdpp<kL1>(a, P.S1);                                  // lane 1: X1
    sel(P2, T.r1, a, Q.S1);                              // (X2 | X1 | Y2)
    sel(Q2, T.r2, P.Zs, o1);                             // (Z1Z1 | Z2Z2 | Z1)
    mul(o2, P2, Q2);                                     // (U2 | U1 | B)
    // lane 2: H = U2 - U1, 2H
    fdpp<kL2>(u2, o2);                                   // lane 0's U2 at lane 2
    fdpp<kL1>(u1, o2);                                   // lane 1's U1 at lane 2
    fe26_sub<2>(h, u2, u1);                              // H                            m 3
    fe26_mul_int<2>(h2, h);                              // 2H                           m 6
    // L3: lane 0 B Z1Z1 (B of lane 2), lane 1 A Z2Z2 (A of lane 2), lane 2 (2H)^2
    fdpp<kR2>(a, o2);                                    // lane 0: B
    fdpp<kR1>(b, o1);                                    // lane 1: A
    sel(P3, T.r0, a, b);
    sel(P3, T.r2, h2, P3);
    sel(Q3, T.r2, h2, o1);
    mul(o3, P3, Q3);                                     // (S2 | S1 | I)
    // lane 2: r = 2 (S2 - S1)
    fdpp<kL2>(s2, o3);                                   // lane 0's S2 at lane 2
    fdpp<kL1>(s1, o3);                                   // lane 1's S1 at lane 2
    fe26_sub<2>(rr, s2, s1);                             //                              m 3
    fe26_mul_int<2>(rr, rr);                             // r                            m 6
    // L4: lane 0 J = H I, lane 1 V = U1 I, lane 2 r^2 (H and I of lane 2)
    fdpp<kR2>(a, h);                                     // lane 0: H
    sel(P4, T.r0, a, o2);                                // (H | U1 | -)
    sel(P4, T.r2, rr, P4);                               // (H | U1 | r)
    fdpp<kR2>(a, o3);                                    // lane 0: I
    fdpp<kR1>(b, o3);                                    // lane 1: I
    sel(Q4, T.r0, a, b);
    sel(Q4, T.r2, rr, Q4);                               // (I | I | r)
    mul(o4, P4, Q4);                                     // (J | V | r^2)
    // lane 0: X3 = r^2 - J - 2V (r^2 of lane 2, V of lane 1), V - X3
    fdpp<kR2>(rv, o4);                                   // lane 0: r^2
    fdpp<kR1>(b, o4);                                    // lane 0: V
    fe26_sub<2>(X3, rv, o4);                             //                              m 3
    fe26_mul_int<2>(t, b);                               //                              m 2
    fe26_sub<3>(X3, X3, t);                              // X3                           m 6
    fe26_sub<7>(W, b, X3);                               // V - X3                       m 8
    // L5: lane 0 r (V - X3) (r of lane 2), lane 1 S1 J (J of lane 0), lane 2 Z1 Z2
    fdpp<kR2>(a, rr);                                    // lane 0: r
    sel(P5, T.r0, a, o3);                                // (r | S1 | -)
    sel(P5, T.r2, P.Zs, P5);                             // (r | S1 | Z1)
    fdpp<kL1>(b, o4);                                    // lane 1: J
    sel(Q5, T.r0, W, b);
    sel(Q5, T.r2, Q.Zs, Q5);                             // (V - X3 | J | Z2)
    mul(o5, P5, Q5);                                     // (r (V - X3) | S1 J | Z1 Z2)
    // L6 (lane 2): Z3 = 2 Z1 Z2 H
    mul(Z3, o5, h);
    fe26_mul_int<2>(Z3, Z3);                             //                              m 2
    // lane 0: Y3 = r (V - X3) - 2 S1 J
    fdpp<kR1>(t, o5);                                    // lane 0: S1 J
    fe26_mul_int<2>(t, t);                               //                              m 2
    fe26_sub<3>(Y3, o5, t);                              // Y3                           m 4
    TrioPt O;
    sel_dpp2<kL1, kL2>(O.S1, T.r0, X3, T.r1, Y3);      // (X3 | Y3 | Y3) from lane 0
    fdpp<kL2>(O.Xs, X3);                                 // lane 2 <- X3 of lane 0
    fe26_copy(O.Zs, Z3);
    O.inf = false;
    // exceptional cases (flags of lane 2, shared across the trio)
    const uint32_t zf = (fe26_is_zero(h) ? 1u : 0u) | (fe26_is_zero(rr) ? 2u : 0u);
    const uint32_t f = bdpp_from(zf, T, 2);
    const bool hz = (f & 1u) != 0u && !P.inf && !Q.inf;
    const bool rz = (f & 2u) != 0u;
    if (any(hz && rz)) {                                 // P == Q: double P on lane 2 (rare)
        Jac26 A, D;
        fe26_copy(A.X, P.Xs);
        fe26_copy(A.Y, P.S1);
        fe26_copy(A.Z, P.Zs);
        A.inf = P.inf;
        CurveK1x::dbl(D, A);
        TrioPt Dt;
        sel_dpp2<kR2, kR1>(Dt.S1, T.r2, D.Y, T.r0, D.X);  // lane 0 <- X, lane 1 <- Y of lane 2
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const uint32_t y = dpp<kR1>(D.Y.v[i]);
            Dt.S1.v[i] = T.r1 ? y : Dt.S1.v[i];
        }
        F26_SETM(Dt.S1, 10);
        fe26_copy(Dt.Xs, D.X);
        fe26_copy(Dt.Zs, D.Z);
        Dt.inf = false;
        trio_cmov(O, Dt, hz && rz);
    }
    if (hz && !rz) O.inf = true;                         // P == -Q
    trio_cmov(O, Q, P.inf);                              // (element-wise: no struct select through memory)
    trio_cmov(O, P, !P.inf && Q.inf);
    R = O;
}

// The Jacobian representative (X K, Y K l, Z K) of the point (X, Y, Z l), for K = l^2: the scaling by l
// that leaves l in the Y coordinate only.  The lane-trio kernel maps its chains' sum from E_w to E this way
// (l = Zc y, K = Zc^2 w): X and Z are then free of the square root y.  In two steps, so that the first can
// run before y is known: trio_scale_xz gives X K and Z K (and Y K on lanes 1 and 2 of S1, not yet a
// coordinate), trio_scale_y multiplies that Y K by l.  S: X, Y, Z <= 16; K, l <= 2 -> (1, 1, 1).
F26_HD void trio_scale_xz(TrioPt& R, const TrioPt& S, const fe26& K, const TrioLane&) {
    using namespace trio;
    TrioPt O;
    mul(O.S1, S.S1, K);                                  // (X K | Y K | Y K)
    mul(O.Xs, S.Xs, K);
    mul(O.Zs, S.Zs, K);
    O.inf = S.inf;
    R = O;
}
F26_HD void trio_scale_y(TrioPt& R, const fe26& l, const TrioLane& T) {
    using namespace trio;
    fe26 t;
    mul(t, R.S1, l);
    sel(R.S1, T.r0, R.S1, t);                            // (X K | Y K l | Y K l)
}

// Z3 of trio_add(P, Q) alone (lane 2), from the X and Z coordinates only -- P.S1 and Q.S1 on lane 0, P.Zs
// and Q.Zs on lane 2 -- in 3 product levels, for a caller whose Y(Q) is not known yet (the lane-trio
// kernel's last addition, ecc_coop.hip):
//   L1  Z1Z1 = Z1^2      | Z2Z2 = Z2^2     | Z1 Z2
//   L2  U2 = X2 Z1Z1     | U1 = X1 Z2Z2    | --
//   L3  --               | --              | Z1 Z2 H             (H = U2 - U1 on lane 2)
// The same value as trio_add's Z3 in each of its cases: 2 Z1 Z2 H, Z(Q) for P = infinity, Z(P) for
// Q = infinity, and for H = 0 the Z of dbl(P) = 2 Y1 Z1 (P.S1 on lane 2 is Y1), which is trio_add's when
// P = Q; when P = -Q the sum is infinity and its Z is never read.  X, Z <= 16 (both) -> m <= 16.
F26_HD void trio_add_z(fe26& Z3, const TrioPt& P, const TrioPt& Q, const TrioLane& T) {
    using namespace trio;
    fe26 a, b, P1, Q1, o1, P2, o2, u2, u1, h, z;
    fdpp<kR2>(a, P.Zs);                                  // lane 0: Z1
    fdpp<kR1>(b, Q.Zs);                                  // lane 1: Z2
    sel(P1, T.r0, a, b);
    sel(P1, T.r2, P.Zs, P1);                             // (Z1 | Z2 | Z1)
    sel(Q1, T.r2, Q.Zs, P1);                             // (Z1 | Z2 | Z2)
    mul(o1, P1, Q1);                                     // (Z1Z1 | Z2Z2 | Z1 Z2)        m 1
    fdpp<kL1>(a, P.S1);                                  // lane 1: X1
    sel(P2, T.r1, a, Q.S1);                              // (X2 | X1 | -)
    mul(o2, P2, o1);                                     // (U2 | U1 | -)
    fdpp<kL2>(u2, o2);                                   // lane 0's U2 at lane 2
    fdpp<kL1>(u1, o2);                                   // lane 1's U1 at lane 2
    fe26_sub<2>(h, u2, u1);                              // H                            m 3
    mul(z, o1, h);                                       // lane 2: Z1 Z2 H
    fe26_mul_int<2>(Z3, z);                              //                              m 2
    const bool hz = T.r2 && fe26_is_zero(h) && !P.inf && !Q.inf;  // (lanes 0 and 1 hold no H)
    if (any(hz)) {                                       // P = +-Q (rare)
        fe26 d;
        fe26_mul(d, P.S1, P.Zs);                         // lane 2: Y1 Z1
        fe26_mul_int<2>(d, d);
        fe26_cmov(Z3, d, hz);
    }
    fe26_cmov(Z3, Q.Zs, P.inf);
    fe26_cmov(Z3, P.Zs, !P.inf && Q.inf);
}

// ------------------------------------------------------------------ the recovery kernel's table on three waves
// trio_table_shared: the co-Z table of P (1 P .. 8 P over one Z, beta x of each entry, that Z, and K = Zc^2 w)
// built by three waves of one workgroup, one lane per tx, each wave one ROLE.  Every stored word is what the
// one-wave build (trio_table_staged, below) stores: the multiples come from the same calls on the same
// inputs, and the rescale factors s_j = Zc / Z_j are the same field values (only the order of the products
// differs, and every stored value is canonical).
//   kTableLong    2P, 3P, 6P, 7P; then the suffix products suf_j = Z_j .. Z_7 (j = 7 .. 2); entries 1, 2, 3
//   kTablePrefix  no multiple; the prefix products pre_j = Z_1 .. Z_j (j = 1 .. 6) as the Z_j arrive, Zc, K;
//                 entries 0 and 7
//   kTableShort   4P, 5P, 8P from the long wave's 2P; entries 4, 5, 6
// LDS (a struct with the members of Trio26RecoverLds named here): the Jacobian multiple (j + 1) P waits in
// L.tab[j] (X, Y raw limbs, m 10) and L.tabphx[j] (Z, m 2) until entry j replaces it; pre_1 .. pre_5 wait in
// the rows of L.xg (free before phase D; pre_6 stays in the prefix wave's registers), suf_2 .. suf_7 in L.tsuf,
// raw limbs of magnitude <= 2.
// H is the hand-off: post(slot) is a release store of 1 by the wave, wait(slot) acquire loads until it reads
// non-zero (device: lds_flag_post / lds_flag_wait on L.spost; host test: std::atomic), stamp(k) a probe.
//   slot             posted by   after                          waited for by
//   kTfMul0 + j      long/short  the multiple (j + 1) P stored  prefix (all), long (7, 6, .. 2), short (1)
//   kTfPre           prefix      its last read of a Z_j; pre_j, zc  long, short
//   kTfSuf           long        its last read of a Z_j; suf_j  prefix, short
//   kTfDone[role]    each role   its last entry (prefix: and K) the chains
// An entry's stores overwrite row j, so they follow every other wave's last read of it: every entry 1 .. 7 is
// stored behind kTfPre and kTfSuf (a wave's own flag is its program order), and the short wave's read of 2P
// precedes its post of kTfMul0 + 7, which the long wave waits for.  Row 0 holds no multiple.  No wait has a
// cycle: the long wave's multiples wait for nothing, the short wave's for kTfMul0 + 1 only, kTfPre and kTfSuf
// for multiples only.  Control flow does not depend on the lane's values, so rejected and idle lanes run the
// same flag sequence.
constexpr int kTableLong = 0, kTablePrefix = 1, kTableShort = 2;
constexpr int kTfDone[3] = {1, 3, 4};  // Trio26RecoverLds::spost slots
constexpr int kTfPre = 7, kTfSuf = 8;
constexpr int kTfMul0 = 8;  // the multiples' slots are kTfMul0 + j, j = 1 .. 7 (slot 8 itself is kTfSuf's)
constexpr int kTfSlots = 16;

namespace trio_table {
// compile-time loop I .. N - 1 (the entries and flag slots are constants); ecc_device.h's Unroll is device-only,
// and this header compiles on the host
template <int I, int N>
struct Seq {
    template <class Fn>
    F26_HD static void run(Fn&& fn) {
        if constexpr (I < N) {
            fn(std::integral_constant<int, I>{});
            Seq<I + 1, N>::run(fn);
        }
    }
};
template <class LDS>
F26_HD void put(LDS& L, int j, const Jac26& J, int lane) {
#pragma unroll
    for (int q = 0; q < 10; ++q) {
        L.tab[j][q][lane] = J.X.v[q];
        L.tab[j][10 + q][lane] = J.Y.v[q];
        L.tabphx[j][q][lane] = J.Z.v[q];
    }
}
template <class LDS>
F26_HD void get_z(fe26& Z, const LDS& L, int j, int lane) {
#pragma unroll
    for (int q = 0; q < 10; ++q) Z.v[q] = L.tabphx[j][q][lane];
    F26_SETM(Z, 2);
}
template <class LDS>
F26_HD void get_xy(fe26& X, fe26& Y, const LDS& L, int j, int lane) {
#pragma unroll
    for (int q = 0; q < 10; ++q) {
        X.v[q] = L.tab[j][q][lane];
        Y.v[q] = L.tab[j][10 + q][lane];
    }
    F26_SETM(X, 10);
    F26_SETM(Y, 10);
}
// a product (m 1; pre_1 and suf_7 are a Z itself, m 2) parked as raw limbs: rows 10 i .. 10 i + 9 of `rows`
// (row number -> that row's 64 words)
template <class Rows>
F26_HD void park(const Rows& rows, int i, const fe26& a, int lane) {
#pragma unroll
    for (int q = 0; q < 10; ++q) rows(10 * i + q)[lane] = a.v[q];
}
template <class Rows>
F26_HD void unpark(fe26& a, const Rows& rows, int i, int lane) {
#pragma unroll
    for (int q = 0; q < 10; ++q) a.v[q] = rows(10 * i + q)[lane];
    F26_SETM(a, 2);
}
F26_HD void store_canonical(uint32_t (*dst)[64], const fe26& a, int lane) {
    fe26 t;
    fe26_copy(t, a);
    fe26_normalize(t);
#pragma unroll
    for (int q = 0; q < 10; ++q) dst[q][lane] = t.v[q];
}
// entry j from its multiple (X, Y) and s = Zc / Z_j: (X s^2, Y s^3) and beta X s^2, canonical limbs
template <class LDS>
F26_HD void entry(LDS& L, int j, const fe26& s, const fe26& X, const fe26& Y, const fe26& beta, int lane) {
    fe26 s2, s3, x, y, bx;
    fe26_sqr(s2, s);
    fe26_mul(s3, s2, s);
    fe26_mul(x, X, s2);
    fe26_mul(y, Y, s3);
    fe26_mul(bx, x, beta);
    store_canonical(L.tab[j], x, lane);
    store_canonical(L.tab[j] + 10, y, lane);
    store_canonical(L.tabphx[j], bx, lane);
}
}  // namespace trio_table

// The one-wave build, the reference of trio_table_shared (tests/cpp/trio_table_test.cpp; no kernel calls it):
// the multiples in the order of multiples8_26, parked in the table's own rows of column `lane`, then s_j from
// prefix products and a running suffix, the entries from the top down (coz_table26), beta x, Zc and K.
template <class LDS>
F26_HD void trio_table_staged(LDS& L, const Aff26& P, const fe26& w, const fe26& beta, int lane) {
    using namespace trio_table;
    {
        Jac26 A, B, N;  // T[j] = (j + 1) P
        CurveK1x::from_aff(B, P);
        CurveK1x::dbl(A, B);      // 2 P
        put(L, 1, A, lane);
        CurveK1x::madd(B, A, P);  // 3 P
        put(L, 2, B, lane);
        CurveK1x::dbl(N, A);      // 4 P
        put(L, 3, N, lane);
        CurveK1x::dbl(A, B);      // 6 P
        put(L, 5, A, lane);
        CurveK1x::madd(B, A, P);  // 7 P
        put(L, 6, B, lane);
        CurveK1x::madd(B, N, P);  // 5 P
        put(L, 4, B, lane);
        CurveK1x::dbl(A, N);      // 8 P
        put(L, 7, A, lane);
    }
    fe26 pre[7], suf, Zc, Zj, K;
    fe26_one(pre[0]);
    get_z(pre[1], L, 1, lane);
    Seq<2, 7>::run([&](auto J) {
        get_z(Zj, L, J, lane);
        fe26_mul(pre[J], pre[J - 1], Zj);
    });
    get_z(Zj, L, 7, lane);
    fe26_mul(Zc, pre[6], Zj);
    fe26_zero(suf);
    Seq<0, 8>::run([&](auto J) {
        constexpr int j = 7 - decltype(J)::value;
        fe26 sj, s2, s3, X, Y, bx;
        if constexpr (j == 0) {
            fe26_copy(X, P.x);
            fe26_copy(Y, P.y);
        } else {
            get_xy(X, Y, L, j, lane);
            get_z(Zj, L, j, lane);
        }
        if constexpr (j == 7) fe26_copy(sj, pre[6]);
        else if constexpr (j <= 1) fe26_copy(sj, suf);
        else fe26_mul(sj, pre[j - 1], suf);
        if constexpr (j == 7) fe26_copy(suf, Zj);
        else if constexpr (j >= 1) fe26_mul(suf, suf, Zj);
        fe26_sqr(s2, sj);
        fe26_mul(s3, s2, sj);
        fe26_mul(X, X, s2);
        fe26_mul(Y, Y, s3);
        fe26_mul(bx, X, beta);
        store_canonical(L.tab[j], X, lane);
        store_canonical(L.tab[j] + 10, Y, lane);
        store_canonical(L.tabphx[j], bx, lane);
    });
    {
        fe26 t;
        uint32_t z8[8];
        fe26_copy(t, Zc);
        fe26_normalize(t);
        fe26_to_words(z8, t);
#pragma unroll
        for (int q = 0; q < 8; ++q) L.zc[q][lane] = z8[q];
    }
    fe26_sqr(K, Zc);
    fe26_mul(K, K, w);
    store_canonical(L.kw, K, lane);
}

// P = R' (m 1 both), w of magnitude <= 2 (the prefix role's K), beta the GLV constant; see above.
template <int ROLE, class LDS, class H>
F26_HD void trio_table_shared(LDS& L, H& h, const Aff26& P, const fe26& w, const fe26& beta, int lane) {
    using namespace trio_table;
    constexpr int kXgRows = sizeof(L.xg[0]) / sizeof(L.xg[0][0]);
    static_assert(sizeof(L.xg) / sizeof(L.xg[0]) * kXgRows >= 50, "xg holds the five parked prefix products");
    static_assert(sizeof(L.tsuf) / sizeof(L.tsuf[0][0]) >= 60, "tsuf holds the six suffix products");
    const auto pre = [&](int r) -> uint32_t* { return L.xg[r / kXgRows][r % kXgRows]; };  // pre_j at place j - 1
    const auto suf = [&](int r) -> uint32_t* { return L.tsuf[r / 10][r % 10]; };          // suf_j at place j - 2
    fe26 X, Y, s, Zj;
    if constexpr (ROLE == kTableLong) {
        {
            Jac26 A, B;
            CurveK1x::from_aff(B, P);
            CurveK1x::dbl(A, B);      // 2 P
            put(L, 1, A, lane);
            h.post(kTfMul0 + 1);
            CurveK1x::madd(B, A, P);  // 3 P
            put(L, 2, B, lane);
            h.post(kTfMul0 + 2);
            CurveK1x::dbl(A, B);      // 6 P
            put(L, 5, A, lane);
            h.post(kTfMul0 + 5);
            CurveK1x::madd(B, A, P);  // 7 P
            put(L, 6, B, lane);
            h.post(kTfMul0 + 6);
        }
        h.stamp(10);
        fe26 run, keep[3];  // suf_2 .. suf_4 stay here for this wave's entries
        h.wait(kTfMul0 + 7);
        get_z(run, L, 7, lane);
        park(suf, 5, run, lane);
        Seq<0, 5>::run([&](auto I) {
            constexpr int j = 6 - decltype(I)::value;  // 6 .. 2
            h.wait(kTfMul0 + j);
            get_z(Zj, L, j, lane);
            fe26_mul(run, run, Zj);
            park(suf, j - 2, run, lane);
            if constexpr (j <= 4) fe26_copy(keep[j - 2], run);
        });
        h.post(kTfSuf);
        h.stamp(11);
        h.wait(kTfPre);
        get_xy(X, Y, L, 1, lane);
        entry(L, 1, keep[0], X, Y, beta, lane);
        Seq<2, 4>::run([&](auto J) {
            constexpr int j = decltype(J)::value;
            unpark(s, pre, j - 2, lane);
            fe26_mul(s, s, keep[j - 1]);
            get_xy(X, Y, L, j, lane);
            entry(L, j, s, X, Y, beta, lane);
        });
    } else if constexpr (ROLE == kTableShort) {
        {
            Jac26 A, B, N;
            h.wait(kTfMul0 + 1);
            get_xy(A.X, A.Y, L, 1, lane);
            get_z(A.Z, L, 1, lane);
            A.inf = false;            // 2 P of an affine P
            CurveK1x::dbl(N, A);      // 4 P
            put(L, 3, N, lane);
            h.post(kTfMul0 + 3);
            CurveK1x::madd(B, N, P);  // 5 P
            put(L, 4, B, lane);
            h.post(kTfMul0 + 4);
            CurveK1x::dbl(A, N);      // 8 P
            put(L, 7, A, lane);
            h.post(kTfMul0 + 7);
        }
        h.stamp(10);
        h.wait(kTfPre);
        h.wait(kTfSuf);
        Seq<4, 7>::run([&](auto J) {
            constexpr int j = decltype(J)::value;
            fe26 t;
            unpark(s, pre, j - 2, lane);
            unpark(t, suf, j - 1, lane);
            fe26_mul(s, s, t);
            get_xy(X, Y, L, j, lane);
            entry(L, j, s, X, Y, beta, lane);
        });
    } else {
        static_assert(ROLE == kTablePrefix, "three roles");
        fe26 run, Zc, K;
        h.wait(kTfMul0 + 1);
        get_z(run, L, 1, lane);
        park(pre, 0, run, lane);
        Seq<2, 7>::run([&](auto J) {
            constexpr int j = decltype(J)::value;
            h.wait(kTfMul0 + j);
            get_z(Zj, L, j, lane);
            fe26_mul(run, run, Zj);
            if constexpr (j < 6) park(pre, j - 1, run, lane);  // (pre_6 = s_7 is this wave's own)
        });
        h.wait(kTfMul0 + 7);
        get_z(Zj, L, 7, lane);
        fe26_mul(Zc, run, Zj);
        {
            fe26 t;
            uint32_t z8[8];
            fe26_copy(t, Zc);
            fe26_normalize(t);
            fe26_to_words(z8, t);
#pragma unroll
            for (int q = 0; q < 8; ++q) L.zc[q][lane] = z8[q];
        }
        h.post(kTfPre);
        h.stamp(10);
        fe26_sqr(K, Zc);
        fe26_mul(K, K, w);
        store_canonical(L.kw, K, lane);
        entry(L, 0, Zc, P.x, P.y, beta, lane);
        h.wait(kTfSuf);
        get_xy(X, Y, L, 7, lane);
        entry(L, 7, run, X, Y, beta, lane);  // s_7 = pre_6
    }
    h.post(kTfDone[ROLE]);
    h.stamp(6);
}

}  // namespace bcosgpu
