// modinv30.h -- the core of the safegcd inversion (modinv.h): 30 divsteps on the low words, the 2x2
// transition-matrix updates of (f, g) and (d, e) in signed 30-bit limbs, and the final normalisation.
// Host/device in the manner of fe26.h (F26_HD): no HIP header and no fe.h, so a host test can run it
// (tests/cpp/modinv_trio_test.cpp).  The fe <-> S30 conversions and the __constant__ moduli stay in modinv.h.
//
// Two forms: one value per lane (divsteps_30, update_fg_30, update_de_30: what every kernel but the
// recovery kernel's phase D uses), and one value per lane TRIO (divsteps_30_trio, update_trio_30,
// modinv_safegcd_trio, at the end of this file), which spreads a divstep's three identical recurrences
// and the two updates over the three lanes of ec26_trio.h's trios.
#pragma once
#include "ec26_trio.h"

namespace bcosgpu {

struct S30 {
    int32_t v[9];
};

struct ModInfo30 {
    int32_t m[9];    // modulus in signed-30 form
    uint32_t inv30;  // m^-1 mod 2^30
};

static constexpr int32_t kM30 = 0x3fffffff;

// 30 divsteps on the low bits of f, g; transition matrix (u, v, q, r) scaled by 2^30:
// u f0 + v g0 = f 2^30, q f0 + r g0 = g 2^30.  zeta = -(delta + 1/2).
F26_HD int32_t divsteps_30(int32_t zeta, uint32_t f, uint32_t g, int32_t t[4]) {
    uint32_t u = 1, v = 0, q = 0, r = 1;
#pragma unroll
    for (int i = 0; i < 30; ++i) {
        uint32_t c1 = static_cast<uint32_t>(zeta >> 31);  // zeta < 0
        const uint32_t c2 = 0u - (g & 1u);                 // g odd
        const uint32_t x = (f ^ c1) - c1, y = (u ^ c1) - c1, z = (v ^ c1) - c1;
        g += x & c2;
        q += y & c2;
        r += z & c2;
        c1 &= c2;
        zeta = (zeta ^ static_cast<int32_t>(c1)) - 1;
        f += g & c1;
        u += q & c1;
        v += r & c1;
        g >>= 1;
        u <<= 1;
        v <<= 1;
    }
    t[0] = static_cast<int32_t>(u);
    t[1] = static_cast<int32_t>(v);
    t[2] = static_cast<int32_t>(q);
    t[3] = static_cast<int32_t>(r);
    return zeta;
}

// (f, g) <- t (f, g) / 2^30 (exact)
F26_HD void update_fg_30(S30& f, S30& g, const int32_t t[4]) {
    const int64_t u = t[0], v = t[1], q = t[2], r = t[3];
    int64_t cf = u * f.v[0] + v * g.v[0];
    int64_t cg = q * f.v[0] + r * g.v[0];
    cf >>= 30;
    cg >>= 30;
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        cf += u * f.v[i] + v * g.v[i];
        cg += q * f.v[i] + r * g.v[i];
        f.v[i - 1] = static_cast<int32_t>(cf) & kM30;
        cf >>= 30;
        g.v[i - 1] = static_cast<int32_t>(cg) & kM30;
        cg >>= 30;
    }
    f.v[8] = static_cast<int32_t>(cf);
    g.v[8] = static_cast<int32_t>(cg);
}

// (d, e) <- (t (d, e) + m (md, me)) / 2^30, md/me chosen so the division is exact; keeps d, e in
// (-2m, m).
F26_HD void update_de_30(S30& d, S30& e, const int32_t t[4], const ModInfo30& mi) {
    const int32_t u = t[0], v = t[1], q = t[2], r = t[3];
    const int32_t sd = d.v[8] >> 31, se = e.v[8] >> 31;
    int32_t md = (u & sd) + (v & se);
    int32_t me = (q & sd) + (r & se);
    int64_t cd = static_cast<int64_t>(u) * d.v[0] + static_cast<int64_t>(v) * e.v[0];
    int64_t ce = static_cast<int64_t>(q) * d.v[0] + static_cast<int64_t>(r) * e.v[0];
    md -= static_cast<int32_t>((mi.inv30 * static_cast<uint32_t>(cd) + static_cast<uint32_t>(md)) & kM30);
    me -= static_cast<int32_t>((mi.inv30 * static_cast<uint32_t>(ce) + static_cast<uint32_t>(me)) & kM30);
    cd += static_cast<int64_t>(mi.m[0]) * md;
    ce += static_cast<int64_t>(mi.m[0]) * me;
    cd >>= 30;
    ce >>= 30;
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        cd += static_cast<int64_t>(u) * d.v[i] + static_cast<int64_t>(v) * e.v[i];
        ce += static_cast<int64_t>(q) * d.v[i] + static_cast<int64_t>(r) * e.v[i];
        cd += static_cast<int64_t>(mi.m[i]) * md;
        ce += static_cast<int64_t>(mi.m[i]) * me;
        d.v[i - 1] = static_cast<int32_t>(cd) & kM30;
        cd >>= 30;
        e.v[i - 1] = static_cast<int32_t>(ce) & kM30;
        ce >>= 30;
    }
    d.v[8] = static_cast<int32_t>(cd);
    e.v[8] = static_cast<int32_t>(ce);
}

// r in (-2m, m) -> sign * r mod m in [0, m)
F26_HD void normalize_30(S30& r, int32_t sign, const ModInfo30& mi) {
    int32_t ca = r.v[8] >> 31;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v[i] += mi.m[i] & ca;
    const int32_t cn = sign >> 31;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v[i] = (r.v[i] ^ cn) - cn;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r.v[i + 1] += r.v[i] >> 30;
        r.v[i] &= kM30;
    }
    ca = r.v[8] >> 31;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v[i] += mi.m[i] & ca;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r.v[i + 1] += r.v[i] >> 30;
        r.v[i] &= kM30;
    }
}

// ------------------------------------------------------------------ the inversion on a lane trio
// A divstep runs one recurrence three times under the same two masks,
//     x = +-A (by c1);  B += x & c2;  c1 &= c2;  A += B & c1;  then B >>= 1 (g) or A <<= 1 (u, v)
// with (A, B) = (f, g), (u, q), (v, r).  Here the three lanes of a trio run it once: role 0 holds (f, g),
// role 1 (u, q), role 2 (v, r).  Only c2 = -(g & 1) has to travel; every lane keeps its own zeta, whose
// update needs nothing but c2.  Lane position 15 of a DPP row, the phantom, is a role-0 lane without
// partners: it computes on whatever it holds, nobody reads it, and its fetches from outside the row
// read 0 (bound_ctrl).
//
// SYSTOLIC (shipped): c2 moves one lane per iteration (one row_shr:1 fetch and one select), so role k runs
// k steps behind role 0 and a batch takes 32 iterations; role k is active in iterations k .. k + 29 and the
// others are no-ops for it: its c2 is 0 there (nothing is added) and its shift is left out where it would
// change a word -- iteration 0 shifts no A (u = 1; v = 0 may be shifted while role 2 still idles in
// iteration 1), iterations 30 and 31 shift no B and 31 only role 2's A.  An idle iteration still counts zeta
// down, so role k enters with zeta + k and leaves with zeta - (2 - k).
// Lag-free (SYSTOLIC = false, kept for the comparison in DESIGN 5): both partners fetch role 0's bit in the
// same iteration, 30 iterations of two fetches and two selects.
//
// In: zeta on every lane, A = f's and B = g's low word on role 0.  Out: (A, B) = (u, q) on role 1 and
// (v, r) on role 2, word for word divsteps_30's matrix for the same zeta, f, g; the new zeta, returned, on
// every lane.
template <bool SYSTOLIC = true>
F26_HD int32_t divsteps_30_trio(int32_t zeta, uint32_t& A, uint32_t& B, const TrioLane& T) {
    using namespace trio;
    const int32_t role = T.r1 ? 1 : T.r2 ? 2 : 0;
    const uint32_t shr = T.r0 ? 1u : 0u, shl = T.r0 ? 0u : 1u;  // g >>= 1 on role 0, u, v <<= 1 on the others
    A = T.r0 ? A : T.r1 ? 1u : 0u;
    B = T.r0 ? B : T.r2 ? 1u : 0u;
    if constexpr (SYSTOLIC) {
        const uint32_t shl_last = T.r2 ? 1u : 0u;
        zeta += role;
        uint32_t c2 = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const uint32_t own = i < 30 ? 0u - (B & 1u) : 0u;  // role 0's steps are 0 .. 29
            if (i == 0) {
                c2 = T.r0 ? own : 0u;
            } else {
                const uint32_t cin = dpp<kL1>(c2);  // the left neighbour's c2 of the iteration before
                c2 = T.r0 ? own : cin;
            }
            uint32_t c1 = static_cast<uint32_t>(zeta >> 31);
            const uint32_t x = (A ^ c1) - c1;
            B += x & c2;
            c1 &= c2;
            zeta = (zeta ^ static_cast<int32_t>(c1)) - 1;
            A += B & c1;
            if (i < 30) B >>= shr;
            if (i == 31) A <<= shl_last;
            else if (i != 0) A <<= shl;
        }
        zeta += 2 - role;
    } else {
#pragma unroll
        for (int i = 0; i < 30; ++i) {
            const uint32_t own = 0u - (B & 1u);
            const uint32_t l1 = dpp<kL1>(own), l2 = dpp<kL2>(own);
            const uint32_t c2 = T.r0 ? own : T.r1 ? l1 : l2;
            uint32_t c1 = static_cast<uint32_t>(zeta >> 31);
            const uint32_t x = (A ^ c1) - c1;
            B += x & c2;
            c1 &= c2;
            zeta = (zeta ^ static_cast<int32_t>(c1)) - 1;
            A += B & c1;
            B >>= shr;
            A <<= shl;
        }
    }
    return zeta;
}

// One batch's two updates in one instruction stream, from the matrix as divsteps_30_trio leaves it:
// role 0's (P, Q) = (f, g) <- t (f, g) / 2^30, role 1's (P, Q) = (d, e) <- (t (d, e) + m (md, me)) / 2^30.
// update_fg_30 is update_de_30 without the modulus term, so the (f, g) lane runs the latter with md = me = 0
// (one mask apiece) and its new low words are in place for the next batch.  Four DPP fetches put all four
// matrix words on both lanes: role 1 holds (u, q) and takes (v, r) from its right neighbour, role 0 takes
// both pairs from its two right neighbours.  Role 2 runs the stream on P = Q = 0, which stay 0, and the
// phantom on a matrix of zeros (its neighbours lie outside the row).
F26_HD void update_trio_30(S30& P, S30& Q, uint32_t A, uint32_t B, const ModInfo30& mi, const TrioLane& T) {
    using namespace trio;
    const uint32_t a1 = dpp<kR1>(A), b1 = dpp<kR1>(B), a2 = dpp<kR2>(A), b2 = dpp<kR2>(B);
    int32_t t[4];
    t[0] = static_cast<int32_t>(T.r0 ? a1 : A);
    t[1] = static_cast<int32_t>(T.r0 ? a2 : a1);
    t[2] = static_cast<int32_t>(T.r0 ? b1 : B);
    t[3] = static_cast<int32_t>(T.r0 ? b2 : b1);
    const int32_t u = t[0], v = t[1], q = t[2], r = t[3];
    const int32_t de = T.r1 ? -1 : 0;  // the modulus term exists on the (d, e) lane only
    const int32_t sd = P.v[8] >> 31, se = Q.v[8] >> 31;
    int32_t md = (u & sd) + (v & se);
    int32_t me = (q & sd) + (r & se);
    int64_t cd = static_cast<int64_t>(u) * P.v[0] + static_cast<int64_t>(v) * Q.v[0];
    int64_t ce = static_cast<int64_t>(q) * P.v[0] + static_cast<int64_t>(r) * Q.v[0];
    md -= static_cast<int32_t>((mi.inv30 * static_cast<uint32_t>(cd) + static_cast<uint32_t>(md)) & kM30);
    me -= static_cast<int32_t>((mi.inv30 * static_cast<uint32_t>(ce) + static_cast<uint32_t>(me)) & kM30);
    md &= de;
    me &= de;
    cd += static_cast<int64_t>(mi.m[0]) * md;
    ce += static_cast<int64_t>(mi.m[0]) * me;
    cd >>= 30;
    ce >>= 30;
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        cd += static_cast<int64_t>(u) * P.v[i] + static_cast<int64_t>(v) * Q.v[i];
        ce += static_cast<int64_t>(q) * P.v[i] + static_cast<int64_t>(r) * Q.v[i];
        cd += static_cast<int64_t>(mi.m[i]) * md;
        ce += static_cast<int64_t>(mi.m[i]) * me;
        P.v[i - 1] = static_cast<int32_t>(cd) & kM30;
        cd >>= 30;
        Q.v[i - 1] = static_cast<int32_t>(ce) & kM30;
        ce >>= 30;
    }
    P.v[8] = static_cast<int32_t>(cd);
    Q.v[8] = static_cast<int32_t>(ce);
}

// out = x^-1 mod m on the lanes of role DST of every trio, for x in [0, m) on the lanes of role 0 (x = 0
// gives 0); what the other lanes hold in x is not read, what they get in out is not a result.  The same
// contract and the same value as modinv_safegcd.  20 batches at most: the loop ends, uniformly over the
// wave, once g == 0 on every lane that holds a g -- role 0 of a real trio.  The other roles keep matrix
// words and (d, e) in the same registers, and the phantom (lane position 15) is a role-0 lane whose g is
// nobody's, so neither takes part in that vote.  d grows on role 1 and is moved once, at the end.  Returns the
// number of batches run (the host test's check of the vote).
template <int DST, bool SYSTOLIC = true>
F26_HD int modinv_safegcd_trio(S30& out, const S30& x, const ModInfo30& mi, const TrioLane& T, int lane) {
    using namespace trio;
    static_assert(DST >= 0 && DST <= 2, "a trio has roles 0, 1, 2");
    const bool votes = T.r0 && (lane & 15) != 15;
    S30 P, Q;  // role 0: (f, g); role 1: (d, e); role 2: zeros
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        P.v[i] = T.r0 ? mi.m[i] : 0;
        Q.v[i] = T.r0 ? x.v[i] : 0;
    }
    Q.v[0] = T.r1 ? 1 : Q.v[0];
    int32_t zeta = -1;
    int batches = 0;
#pragma unroll 1
    for (int it = 0; it < 20; ++it) {
        ++batches;
        uint32_t A = static_cast<uint32_t>(P.v[0]), B = static_cast<uint32_t>(Q.v[0]);
        zeta = divsteps_30_trio<SYSTOLIC>(zeta, A, B, T);
        update_trio_30(P, Q, A, B, mi, T);
        int32_t gz = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) gz |= Q.v[i];
        if (!any(votes && gz != 0)) break;  // every g is 0: the rest are no-ops
    }
    const int32_t fsign = static_cast<int32_t>(dpp<kL1>(static_cast<uint32_t>(P.v[8])));  // role 1: f's top limb
    normalize_30(P, fsign, mi);
    if constexpr (DST == 1) {
        out = P;
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i)
            out.v[i] = static_cast<int32_t>(DST == 2 ? dpp<kL1>(static_cast<uint32_t>(P.v[i]))
                                                     : dpp<kR1>(static_cast<uint32_t>(P.v[i])));
    }
    return batches;
}

}  // namespace bcosgpu
