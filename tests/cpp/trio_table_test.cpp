// trio_table_test.cpp -- host build (FE26_CHECK) of the recovery kernel's table on three waves
// (trio_table_shared, ec26_trio.h): the three roles run as three host threads over a host copy of the LDS
// struct (a fourth reads the table behind the three "done" flags, as a chain wave does), the hand-off a
// std::atomic with the device's orders (release store, acquire loads), and every word they leave in tab,
// tabphx, zc and kw is compared with the one-wave build (trio_table_staged) of the same inputs.  A role's
// thread walks the 64 lanes of its wave one after the other, each lane with flags of its own
// (on the device a wave posts once for all its lanes; a lane touches its own column only), so the sanitizers
// see every hand-off of every lane: -fsanitize=thread reports an entry stored ahead of the flag that guards
// its multiple, and a flag order that cannot finish ends at the watchdog (exit 3 after 10 s).
// Cases, for 1, 39 and 40 active lanes (the others hold r = 0, as the kernel's idle lanes): random x of curve
// points, x with no curve point, and what a rejected signature leaves (x = 0, whose R' has order 3 and meets
// the additions' special cases, x = 1, x = p - 1, raw x >= p).  Beside the comparison: each entry is (j + 1) R'
// by repeated addition on one lane, beta x is beta times x, K is Zc^2 w, and no magnitude assertion fires.
// The inputs are the table build's own: R' = (w x, w^2) and w formed here from x in fe26 (the table holds no
// y, so v's parity does not reach it).  The kernel's recover_w -- x = r + n for v & 2, and what it leaves of a
// rejected row -- is device code and is covered by the GPU tests only (tests/test_gpu_trio_table.py).
// Prints "trio table ok <lanes>" and exits 0, or the first mismatch and exits 1.
#define FE26_CHECK 1
#include "../../fisco-bcos_amd/csrc/ec26_trio.h"

#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

using namespace bcosgpu;

namespace bcosgpu {
// the table runs one lane per tx: no DPP
uint32_t trio_emu_dpp(uint32_t, int) { abort(); }
bool trio_emu_any(bool) { abort(); }
}  // namespace bcosgpu

namespace {
// the members of Trio26RecoverLds that the table build names
struct HostLds {
    uint32_t tab[8][20][64];
    uint32_t tabphx[8][10][64];
    uint32_t zc[8][64];
    uint32_t xg[2][31][64];
    uint32_t tsuf[6][10][64];
    uint32_t kw[10][64];
};
struct HostFlags {
    std::atomic<uint32_t> f[kTfSlots];
    HostFlags() {
        for (auto& a : f) a.store(0u, std::memory_order_relaxed);
    }
    void post(int s) { f[s].store(1u, std::memory_order_release); }
    void wait(int s) {
        while (f[s].load(std::memory_order_acquire) == 0u) std::this_thread::yield();
    }
    void stamp(int) {}
};

const uint32_t kBetaWords[8] = {0x719501eeu, 0xc1396c28u, 0x12f58995u, 0x9cf04975u,
                                0xac3434e9u, 0x6e64479eu, 0x657c0710u, 0x7ae96a2bu};

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return static_cast<uint32_t>(rng_state >> 11);
}
void rand_words(uint32_t w[8]) {
    for (int i = 0; i < 8; ++i) w[i] = (rnd() << 16) ^ rnd();
}
bool same(const fe26& a, const fe26& b) {
    fe26 x = a, y = b;
    fe26_normalize(x);
    fe26_normalize(y);
    return memcmp(x.v, y.v, sizeof x.v) == 0;
}
// w = x^3 + 7 (m 2) as recover_w forms it, and whether it is a square
bool rhs_of(fe26& w, const fe26& x) {
    fe26 t, seven, y;
    fe26_sqr(t, x);
    fe26_mul(w, t, x);
    fe26_set_small(seven, 7u);
    fe26_add(w, w, seven);
    fe26_sqrt_cand(y, w);
    fe26_sqr(t, y);
    return same(t, w);
}
void rand_x(fe26& x, bool on_curve) {
    for (;;) {
        uint32_t w8[8];
        fe26 w;
        rand_words(w8);
        w8[7] &= 0x7fffffffu;
        fe26_from_words(x, w8);
        if (rhs_of(w, x) == on_curve) return;
    }
}

int fail(const char* what, int c, int lane, int j) {
    printf("MISMATCH %s: case %d lane %d entry %d\n", what, c, lane, j);
    return 1;
}

// one workgroup: the three roles as threads, against the one-wave build
int run_case(int c, const fe26 (&x)[64]) {
    auto L = std::make_unique<HostLds>();
    auto Ref = std::make_unique<HostLds>();
    memset(L.get(), 0xa5, sizeof(HostLds));
    memset(Ref.get(), 0xa5, sizeof(HostLds));
    auto flags = std::make_unique<HostFlags[]>(64);
    static Aff26 R[64];
    static fe26 w[64];
    fe26 beta;
    fe26_from_words(beta, kBetaWords);
    for (int lane = 0; lane < 64; ++lane) {
        rhs_of(w[lane], x[lane]);
        fe26_mul(R[lane].x, w[lane], x[lane]);  // w x
        fe26_sqr(R[lane].y, w[lane]);           // w^2
        trio_table_staged(*Ref, R[lane], w[lane], beta, lane);
    }
    std::thread t1([&] {
        for (int lane = 0; lane < 64; ++lane)
            trio_table_shared<kTableLong>(*L, flags[lane], R[lane], w[lane], beta, lane);
    });
    std::thread t2([&] {
        for (int lane = 0; lane < 64; ++lane)
            trio_table_shared<kTablePrefix>(*L, flags[lane], R[lane], w[lane], beta, lane);
    });
    std::thread t3([&] {
        for (int lane = 0; lane < 64; ++lane)
            trio_table_shared<kTableShort>(*L, flags[lane], R[lane], w[lane], beta, lane);
    });
    // a chain wave: behind the three "done" flags it reads the column (a "done" posted before the wave's last
    // store is a race with these reads)
    auto Seen = std::make_unique<HostLds>();
    memset(Seen.get(), 0xa5, sizeof(HostLds));
    std::thread t0([&] {
        for (int lane = 0; lane < 64; ++lane) {
            for (int role = 0; role < 3; ++role) flags[lane].wait(kTfDone[role]);
            for (int j = 0; j < 8; ++j) {
                for (int q = 0; q < 20; ++q) Seen->tab[j][q][lane] = L->tab[j][q][lane];
                for (int q = 0; q < 10; ++q) Seen->tabphx[j][q][lane] = L->tabphx[j][q][lane];
            }
            for (int q = 0; q < 8; ++q) Seen->zc[q][lane] = L->zc[q][lane];
            for (int q = 0; q < 10; ++q) Seen->kw[q][lane] = L->kw[q][lane];
        }
    });
    t1.join();
    t2.join();
    t3.join();
    t0.join();
    for (int lane = 0; lane < 64; ++lane) {
        for (int j = 0; j < 8; ++j) {
            for (int q = 0; q < 20; ++q)
                if (Seen->tab[j][q][lane] != Ref->tab[j][q][lane]) return fail("tab as the chains read it", c, lane, j);
            for (int q = 0; q < 10; ++q)
                if (Seen->tabphx[j][q][lane] != Ref->tabphx[j][q][lane])
                    return fail("tabphx as the chains read it", c, lane, j);
        }
        for (int q = 0; q < 8; ++q)
            if (Seen->zc[q][lane] != Ref->zc[q][lane]) return fail("zc as the chains read it", c, lane, q);
        for (int q = 0; q < 10; ++q)
            if (Seen->kw[q][lane] != Ref->kw[q][lane]) return fail("kw as the chains read it", c, lane, q);
        for (int j = 0; j < 8; ++j) {
            for (int q = 0; q < 20; ++q)
                if (L->tab[j][q][lane] != Ref->tab[j][q][lane]) return fail("tab", c, lane, j);
            for (int q = 0; q < 10; ++q)
                if (L->tabphx[j][q][lane] != Ref->tabphx[j][q][lane]) return fail("tabphx", c, lane, j);
        }
        for (int q = 0; q < 8; ++q)
            if (L->zc[q][lane] != Ref->zc[q][lane]) return fail("zc", c, lane, q);
        for (int q = 0; q < 10; ++q)
            if (L->kw[q][lane] != Ref->kw[q][lane]) return fail("kw", c, lane, q);
    }
    // the values themselves, on one lane: entry j is (j + 1) R' over Zc, beta x, K = Zc^2 w
    for (int lane = 0; lane < 64; ++lane) {
        uint32_t z8[8];
        fe26 Zc, K, t;
        for (int q = 0; q < 8; ++q) z8[q] = L->zc[q][lane];
        fe26_from_words(Zc, z8);
        for (int q = 0; q < 10; ++q) K.v[q] = L->kw[q][lane];
        K.m = 1;
        fe26_sqr(t, Zc);
        fe26_mul(t, t, w[lane]);
        if (!same(t, K)) return fail("K", c, lane, 0);
        fe26 zero;
        fe26_zero(zero);
        if (same(Zc, zero)) continue;  // a multiple at infinity (x = 0): the co-Z table is degenerate
        Jac26 S;
        CurveK1x::from_aff(S, R[lane]);
        for (int j = 0; j < 8; ++j) {
            if (j) CurveK1x::madd(S, S, R[lane]);
            fe26 X, Y, bx, z2, z3, l;
            for (int q = 0; q < 10; ++q) {
                X.v[q] = L->tab[j][q][lane];
                Y.v[q] = L->tab[j][10 + q][lane];
                bx.v[q] = L->tabphx[j][q][lane];
            }
            X.m = Y.m = bx.m = 1;
            // (X, Y, Zc) and S are one point: X Zs^2 = Xs Zc^2, Y Zs^3 = Ys Zc^3
            fe26 zs2, zs3, r;
            fe26_sqr(z2, Zc);
            fe26_mul(z3, z2, Zc);
            fe26_sqr(zs2, S.Z);
            fe26_mul(zs3, zs2, S.Z);
            fe26_mul(l, X, zs2);
            fe26_mul(r, S.X, z2);
            if (S.inf || !same(l, r)) return fail("x of (j + 1) R'", c, lane, j);
            fe26_mul(l, Y, zs3);
            fe26_mul(r, S.Y, z3);
            if (!same(l, r)) return fail("y of (j + 1) R'", c, lane, j);
            fe26_mul(l, X, beta);
            if (!same(l, bx)) return fail("beta x", c, lane, j);
        }
    }
    return 0;
}
}  // namespace

int main() {
    std::atomic<bool> done{false};
    std::thread watchdog([&] {
        const auto t0 = std::chrono::steady_clock::now();
        while (!done.load()) {
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
                printf("STRANDED: a table wave did not end within 10 s\n");
                fflush(stdout);
                _exit(3);
            }
        }
    });
    fe26 beta, b3;
    fe26_from_words(beta, kBetaWords);
    fe26_sqr(b3, beta);
    fe26_mul(b3, b3, beta);
    fe26 one;
    fe26_one(one);
    int rc = same(b3, one) && !same(beta, one) ? 0 : fail("beta", -1, 0, 0);
    int lanes = 0, c = 0;
    const int actives[3] = {1, 39, 40};
    for (int a = 0; a < 3 && rc == 0; ++a) {
        for (int kind = 0; kind < 3 && rc == 0; ++kind, ++c) {
            static fe26 x[64];
            for (int lane = 0; lane < 64; ++lane) {
                fe26_zero(x[lane]);  // an idle lane: r = 0
                if (lane >= actives[a]) continue;
                if (kind == 0) {
                    rand_x(x[lane], true);
                } else if (kind == 1) {
                    rand_x(x[lane], false);
                } else {  // what a rejected signature can leave in r
                    uint32_t w8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    switch (lane % 5) {
                        case 0: break;                 // 0
                        case 1: w8[0] = 1u; break;     // 1
                        case 2:                        // p - 1
                            for (int i = 0; i < 8; ++i) w8[i] = 0xffffffffu;
                            w8[1] = 0xfffffffeu;
                            w8[0] = 0xfffffc2eu;
                            break;
                        case 3:                        // 2^256 - 1 (raw, >= p)
                            for (int i = 0; i < 8; ++i) w8[i] = 0xffffffffu;
                            break;
                        default: rand_words(w8); break;  // any 256 bits
                    }
                    fe26_from_words(x[lane], w8);
                }
            }
            rc = run_case(c, x);
            lanes += 64;
        }
    }
    done.store(true);
    watchdog.join();
    if (rc == 0) printf("trio table ok %d\n", lanes);
    return rc;
}
