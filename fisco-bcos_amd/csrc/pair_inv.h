// pair_inv.h -- r^-1 and u2 = s / r (mod n, secp256k1's group order) for a PAIR of signatures from ONE
// inversion (Montgomery's simultaneous inversion), laid out for a lane trio of ec26_trio.h.  Host/device in
// the manner of glv_split.h and modinv30.h: no HIP header and no fe.h, the arithmetic comes in through Ops, so
// a host test runs the very sequence the kernel runs (tests/cpp/pair_inv_test.cpp).
//
// tx_verify_trio26_kernel's wave 0 has 20 trio seats and a workgroup 40 txs, so seat t takes txs a = t (role 0
// holds r_a, s_a) and b = t + 20 (role 1 holds r_b, s_b); role 2 holds r = 1, s = 0.  With M(x, y) = x y / R
// the Montgomery product (R = 2^256) the path is three product levels and one inversion, all values plain
// on entry:
//   level 1   pre  = ( M(r_a, r_b)   | M(r_b, s_a)   | M(r_a, s_b) )     = (r_a r_b | r_b s_a | r_a s_b) / R
//   inverse   t    = pre_0^-1 = R / (r_a r_b), on every lane of the trio (Ops::inv)
//   level 2   inv  = M(t, R^2)       = R^2 / (r_a r_b)                     (the one Montgomery correction)
//   level 3   u2   = ( M(inv, pre_1) | M(inv, pre_2) | - )                = (s_a / r_a | s_b / r_b), plain
//   level 4   rinv = ( M(inv, r_b)   | M(inv, r_a)   | - )                = (R / r_a | R / r_b), Montgomery form
// u2 feeds glv_split, rinv the helpers' u1 = -e / r; both are canonical residues, so they equal word for word
// what one inversion per tx gives.  Level 4 is off the chains' path (pair_rinv, called after the scalars are
// posted).
//
// A product of the pair's r is only invertible when both are: a member with r = 0 would zero the partner's
// inverse, and an unreduced r >= n leaves the Montgomery product's range.  So a member that is rejected or
// absent enters as r = 1, s = 0 (pair_enter): its own u2 is 0 and its rinv is R, as with one inversion per
// tx, and the partner's values are exact.
//
// Ops (every method acts on all lanes alike; V has uint32_t v[8], little-endian limbs):
//   right1(o, a), left1(o, a), left2(o, a)   o = a of the lane 1 to the right / 1, 2 to the left (DPP row shifts)
//   sel(o, roles, a, b)                      o = (this lane's role is in the mask `roles`) ? a : b
//   mul(o, a, b)                             o = M(a, b) mod n; a, b < n
//   inv(o, x)                                o = x^-1 mod n of role 0's x, on every lane of the trio
//   stamp(k)                                 a time stamp for the phase probe (kPairStamp*)
#pragma once
#include <stdint.h>

#include "fe26.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PAIR_TABLE __device__ __constant__ static const uint32_t
#else
#define PAIR_TABLE static const uint32_t
#endif

namespace bcosgpu {

// R^2 mod n (ParamN1::R2 of fe.h)
PAIR_TABLE kPairR2N1[8] = {0x67d7d140u, 0x896cf214u, 0x0e7cf878u, 0x741496c2u,
                           0x5bcd07c6u, 0xe697f5e4u, 0x81c69bc5u, 0x9d671cd5u};

constexpr int kPairRole0 = 1, kPairRole1 = 2, kPairRole2 = 4;
constexpr int kPairStampPre = 0, kPairStampInv = 1;

// the substitution rule: a member that is not a parsed, range-checked signature (0 < r, s < n) enters as
// r = 1, s = 0
template <class V>
F26_HD void pair_enter(V& r, V& s, bool ok) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r.v[i] = ok ? r.v[i] : (i == 0 ? 1u : 0u);
        s.v[i] = ok ? s.v[i] : 0u;
    }
}

// levels 1 .. 3: u2 on roles 0 and 1, and inv = R^2 / (r_a r_b) on every lane for pair_rinv
template <class V, class Ops>
F26_HD void pair_scalars(V& u2, V& inv, const V& r, const V& s, Ops& ops) {
    V rr1, rl2, sl1, x, y, pre, t, k;
    ops.right1(rr1, r);
    ops.left2(rl2, r);
    ops.left1(sl1, s);
    ops.sel(x, kPairRole2, rl2, r);   // (r_a | r_b | r_a)
    ops.sel(y, kPairRole0, rr1, sl1);  // (r_b | s_a | s_b)
    ops.mul(pre, x, y);
    ops.stamp(kPairStampPre);
    ops.inv(t, pre);
#pragma unroll
    for (int i = 0; i < 8; ++i) k.v[i] = kPairR2N1[i];
    ops.mul(inv, t, k);
    ops.stamp(kPairStampInv);
    ops.right1(y, pre);  // role 0: r_b s_a / R, role 1: r_a s_b / R
    ops.mul(u2, inv, y);
}

// level 4: r^-1 in Montgomery form on roles 0 and 1, each from the partner's r
template <class V, class Ops>
F26_HD void pair_rinv(V& rinv, const V& inv, const V& r, Ops& ops) {
    V rr1, rl1, y;
    ops.right1(rr1, r);
    ops.left1(rl1, r);
    ops.sel(y, kPairRole0, rr1, rl1);  // (r_b | r_a | -)
    ops.mul(rinv, inv, y);
}

}  // namespace bcosgpu
