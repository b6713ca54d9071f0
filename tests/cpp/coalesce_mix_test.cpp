// coalesce_mix_test.cpp -- every host-pointer signature entry point of the C ABI called concurrently in one
// process, so that the coalescer (csrc/coalesce.hip) queues jobs of all three kinds and of every shape together:
//   0 bcosgpu_secp256k1_recover            one signature
//   1 bcosgpu_secp256k1_recover_batch      n = 2..300, and once 2,500 (past the zero-copy staging); pub64 / addr20
//                                          set or null
//   2 bcosgpu_secp256k1_verify             one signature, named key (sig_len 64 or 65)
//   3 bcosgpu_sm2_verify                   one signature, named key
//   4 bcosgpu_sm2_verify_batch             n = 2..300, embedded key; addr20 set or null
//   5 bcosgpu_verify_batch secp256k1       n = 1..64, stride 64 or 65
//   6 bcosgpu_verify_batch SM2             n = 1..64, stride 64 or 128
// The named keys are few, so they are promoted to the registered-key kernel in the middle of the run.
//
//   coalesce_mix_test <datafile> <threads> <calls_per_thread> [seed]
// datafile (written by tests/test_gpu_coalesce.py, every expected value the oracle's): "BGMX", u32 m, then
//   secp256k1 recover: m x 32 hashes, m x 65 signatures, m verdicts, m x 64 keys, m x 20 addresses (keys and
//                      addresses of invalid signatures zero, here and for SM2: the kernels write zeros)
//   secp256k1 verify:  m x 32 hashes, m x 65 signatures, m x 64 keys, m verdicts
//   SM2 recover:       m x 32 hashes, m x 128 signatures (r||s||key), m verdicts, m x 20 addresses
//   SM2 verify:        m x 32 hashes, m x 128 signatures (r||s||key), m verdicts
// Every output buffer is filled with a guard byte and has 64 guard bytes on either side.  Prints one JSON line
// with the mismatch records of mismatch_record.h and the coalescer's statistics; exit 0 iff every result
// matched and every guard is intact, 77 without a device.
#include <bcos_gpu.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "mismatch_record.h"

namespace {

using mismatch::kGuard;

struct Guarded {
    std::vector<uint8_t> mem;
    explicit Guarded(size_t n) : mem(n + 128, kGuard) {}
    uint8_t* p() { return mem.data() + 64; }
    bool intact() const {
        return mismatch::all_bytes(mem.data(), 64, kGuard) && mismatch::all_bytes(mem.data() + mem.size() - 64, 64, kGuard);
    }
};

bool read_all(FILE* f, std::vector<uint8_t>& v, size_t n) {
    v.resize(n);
    return fread(v.data(), 1, n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s datafile threads calls_per_thread [seed]\n", argv[0]);
        return 2;
    }
    if (bcosgpu_device_count() <= 0) {
        printf("no gfx950 device\n");
        return 77;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    char magic[4];
    uint32_t m32 = 0;
    if (fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "BGMX", 4) != 0 || fread(&m32, 4, 1, f) != 1 || m32 < 2500) return 2;
    const size_t m = m32;
    std::vector<uint8_t> rk_h, rk_sig, rk_ok, rk_pub, rk_addr, vk_h, vk_sig, vk_key, vk_ok, rs_h, rs_sig, rs_ok, rs_addr, vs_h,
        vs_sig, vs_ok;
    if (!read_all(f, rk_h, 32 * m) || !read_all(f, rk_sig, 65 * m) || !read_all(f, rk_ok, m) || !read_all(f, rk_pub, 64 * m) ||
        !read_all(f, rk_addr, 20 * m) || !read_all(f, vk_h, 32 * m) || !read_all(f, vk_sig, 65 * m) ||
        !read_all(f, vk_key, 64 * m) || !read_all(f, vk_ok, m) || !read_all(f, rs_h, 32 * m) || !read_all(f, rs_sig, 128 * m) ||
        !read_all(f, rs_ok, m) || !read_all(f, rs_addr, 20 * m) || !read_all(f, vs_h, 32 * m) || !read_all(f, vs_sig, 128 * m) ||
        !read_all(f, vs_ok, m))
        return 2;
    fclose(f);
    // the compact forms: r||s at stride 64, the SM2 keys on their own
    std::vector<uint8_t> vk_sig64(64 * m), vs_sig64(64 * m), vs_key(64 * m);
    for (size_t i = 0; i < m; ++i) {
        std::memcpy(&vk_sig64[64 * i], &vk_sig[65 * i], 64);
        std::memcpy(&vs_sig64[64 * i], &vs_sig[128 * i], 64);
        std::memcpy(&vs_key[64 * i], &vs_sig[128 * i + 64], 64);
    }
    const int threads = atoi(argv[2]);
    const int calls = atoi(argv[3]);
    const uint64_t seed = argc > 4 ? strtoull(argv[4], nullptr, 10) : 1;
    if (bcosgpu_init(0) != 0) {
        printf("bcosgpu_init: %s\n", bcosgpu_last_error());
        return 2;
    }
    {  // warm the engine (tables, staging buffers)
        uint8_t pub[64];
        (void)bcosgpu_secp256k1_recover(0, rk_h.data(), rk_sig.data(), 65, pub);
    }
    uint64_t st[10] = {};
    (void)bcosgpu_coalesce_stats(0, st, 1);

    mismatch::Log log;
    log.tables.push_back({rk_pub.data(), 64, m});
    log.tables.push_back({rk_addr.data(), 20, m});
    log.tables.push_back({rs_addr.data(), 20, m});
    std::atomic<long> mismatches{0}, engine_errors{0}, guard_violations{0}, items{0};
    std::atomic<long> ops[7];
    for (auto& o : ops) o.store(0);
    static const uint8_t zero[64] = {};

    auto verdict = [&](int t, long c, const char* op, long item, int want, uint8_t got) {
        if (got == (want ? 1 : 0)) return;
        ++mismatches;
        const uint8_t w = want ? 1 : 0;
        log.add(t, c, op, "ok", item, want, got, got == kGuard ? &got : nullptr, &w, 1);
    };
    auto single = [&](int t, long c, const char* op, long item, int want, int rc) {
        if (rc < 0) {
            ++engine_errors;
            ++mismatches;
            log.add(t, c, op, "rc", item, want, rc, nullptr, nullptr, 0);
        } else {
            verdict(t, c, op, item, want, static_cast<uint8_t>(rc));
        }
    };
    auto failed = [&](int t, long c, const char* op, long item, int rc) {
        ++engine_errors;
        ++mismatches;
        log.add(t, c, op, "rc", item, -1, rc, nullptr, nullptr, 0);
    };

    std::vector<std::thread> pool;
    const auto t0 = std::chrono::steady_clock::now();
    for (int t = 0; t < threads; ++t) {
        pool.emplace_back([&, t] {
            std::mt19937_64 rng(seed * 1000003 + static_cast<uint64_t>(t));
            if (bcosgpu_init(0) != 0) {
                failed(t, -1, "bcosgpu_init", -1, -1);
                return;
            }
            for (long c = 0; c < calls; ++c) {
                const unsigned draw = rng() % 100;
                int op = draw < 30 ? 0 : draw < 45 ? 2 : draw < 60 ? 3 : draw < 70 ? 1 : draw < 80 ? 4 : draw < 90 ? 5 : 6;
                size_t n = op == 1 || op == 4 ? 2 + rng() % 299 : op >= 5 ? 1 + rng() % 64 : 1;
                if (t == 0 && c == 1) op = 1, n = 2500;
                const size_t at = rng() % (m - n + 1);
                ops[op].fetch_add(1);
                items.fetch_add(static_cast<long>(n));
                if (op == 0) {
                    Guarded pub(64);
                    const int rc = bcosgpu_secp256k1_recover(0, &rk_h[32 * at], &rk_sig[65 * at], 65, pub.p());
                    if (!pub.intact()) ++guard_violations;
                    const uint8_t* want = rk_ok[at] ? &rk_pub[64 * at] : zero;
                    if (rc < 0) {
                        failed(t, c, "secp256k1_recover", static_cast<long>(at), rc);
                    } else if (rc != rk_ok[at] || std::memcmp(pub.p(), want, 64) != 0) {
                        ++mismatches;
                        log.add(t, c, "secp256k1_recover", "pub", static_cast<long>(at), rk_ok[at], rc, pub.p(), want, 64);
                    }
                } else if (op == 1) {
                    const bool with_pub = rng() % 4 != 0, with_addr = rng() % 2;
                    Guarded pub(64 * n), addr(20 * n), ok(n);
                    const int rc = bcosgpu_secp256k1_recover_batch(&rk_h[32 * at], &rk_sig[65 * at], n, with_pub ? pub.p() : nullptr,
                                                                   with_addr ? addr.p() : nullptr, ok.p());
                    if (!pub.intact() || !addr.intact() || !ok.intact()) ++guard_violations;
                    if (rc != 0) {
                        failed(t, c, "secp256k1_recover_batch", static_cast<long>(at), rc);
                        continue;
                    }
                    // an output not asked for stays as the caller left it
                    if (!with_pub && !mismatch::all_bytes(pub.p(), 64 * n, kGuard)) ++guard_violations;
                    if (!with_addr && !mismatch::all_bytes(addr.p(), 20 * n, kGuard)) ++guard_violations;
                    for (size_t i = 0; i < n; ++i) {
                        const long item = static_cast<long>(at + i);
                        const int want_ok = rk_ok[at + i];
                        const uint8_t* want = want_ok ? &rk_pub[64 * (at + i)] : zero;
                        if (with_pub && std::memcmp(pub.p() + 64 * i, want, 64) != 0) {
                            ++mismatches;
                            log.add(t, c, "secp256k1_recover_batch", "pub", item, want_ok, ok.p()[i], pub.p() + 64 * i, want, 64);
                        } else if (with_addr && std::memcmp(addr.p() + 20 * i, &rk_addr[20 * (at + i)], 20) != 0) {
                            ++mismatches;
                            log.add(t, c, "secp256k1_recover_batch", "addr", item, want_ok, ok.p()[i], addr.p() + 20 * i,
                                    &rk_addr[20 * (at + i)], 20);
                        } else {
                            verdict(t, c, "secp256k1_recover_batch", item, want_ok, ok.p()[i]);
                        }
                    }
                } else if (op == 2) {
                    const bool full = rng() % 2;
                    const int rc = bcosgpu_secp256k1_verify(0, &vk_key[64 * at], &vk_h[32 * at], full ? &vk_sig[65 * at] : &vk_sig64[64 * at],
                                                            full ? 65 : 64);
                    single(t, c, "secp256k1_verify", static_cast<long>(at), vk_ok[at], rc);
                } else if (op == 3) {
                    const int rc = bcosgpu_sm2_verify(0, &vs_key[64 * at], &vs_h[32 * at], &vs_sig64[64 * at]);
                    single(t, c, "sm2_verify", static_cast<long>(at), vs_ok[at], rc);
                } else if (op == 4) {
                    const bool with_addr = rng() % 2;
                    Guarded addr(20 * n), ok(n);
                    const int rc = bcosgpu_sm2_verify_batch(&rs_h[32 * at], &rs_sig[128 * at], n, with_addr ? addr.p() : nullptr, ok.p());
                    if (!addr.intact() || !ok.intact()) ++guard_violations;
                    if (rc != 0) {
                        failed(t, c, "sm2_verify_batch", static_cast<long>(at), rc);
                        continue;
                    }
                    if (!with_addr && !mismatch::all_bytes(addr.p(), 20 * n, kGuard)) ++guard_violations;
                    for (size_t i = 0; i < n; ++i) {
                        const long item = static_cast<long>(at + i);
                        const int want_ok = rs_ok[at + i];
                        if (with_addr && std::memcmp(addr.p() + 20 * i, &rs_addr[20 * (at + i)], 20) != 0) {
                            ++mismatches;
                            log.add(t, c, "sm2_verify_batch", "addr", item, want_ok, ok.p()[i], addr.p() + 20 * i,
                                    &rs_addr[20 * (at + i)], 20);
                        } else {
                            verdict(t, c, "sm2_verify_batch", item, want_ok, ok.p()[i]);
                        }
                    }
                } else {
                    const bool sm2 = op == 6, wide = rng() % 2;
                    Guarded ok(n);
                    int rc;
                    if (sm2)
                        rc = bcosgpu_verify_batch(BCOSGPU_SUITE_SM2, &vs_key[64 * at], &vs_h[32 * at],
                                                  wide ? &vs_sig[128 * at] : &vs_sig64[64 * at], wide ? 128 : 64, n, ok.p());
                    else
                        rc = bcosgpu_verify_batch(BCOSGPU_SUITE_SECP256K1, &vk_key[64 * at], &vk_h[32 * at],
                                                  wide ? &vk_sig[65 * at] : &vk_sig64[64 * at], wide ? 65 : 64, n, ok.p());
                    const char* name = sm2 ? "verify_batch_sm2" : "verify_batch_secp256k1";
                    if (!ok.intact()) ++guard_violations;
                    if (rc != 0) {
                        failed(t, c, name, static_cast<long>(at), rc);
                        continue;
                    }
                    for (size_t i = 0; i < n; ++i)
                        verdict(t, c, name, static_cast<long>(at + i), sm2 ? vs_ok[at + i] : vk_ok[at + i], ok.p()[i]);
                }
            }
        });
    }
    for (auto& th : pool) th.join();
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    (void)bcosgpu_coalesce_stats(0, st, 0);
    int64_t kc[2][5] = {};
    (void)bcosgpu_key_cache_info(0, BCOSGPU_SUITE_SECP256K1, kc[0]);
    (void)bcosgpu_key_cache_info(0, BCOSGPU_SUITE_SM2, kc[1]);
    std::string opcounts, keyed;
    for (int k = 0; k < 7; ++k) opcounts += (k ? ", " : "") + std::to_string(ops[k].load());
    for (int s = 0; s < 2; ++s) {
        keyed += s ? ", [" : "[";
        for (int k = 0; k < 5; ++k) keyed += (k ? ", " : "") + std::to_string(kc[s][k]);
        keyed += "]";
    }
    printf("{\"threads\": %d, \"calls\": %ld, \"items\": %ld, \"ops\": [%s], \"mismatches\": %ld, \"engine_errors\": %ld, "
           "\"guard_violations\": %ld, \"seconds\": %.4f, \"key_cache\": [%s], \"records\": %s, \"coalesce_stats\": %s}\n",
           threads, static_cast<long>(threads) * calls, items.load(), opcounts.c_str(), mismatches.load(), engine_errors.load(),
           guard_violations.load(), dt, keyed.c_str(), log.json().c_str(), mismatch::stats_json(st).c_str());
    return mismatches.load() == 0 && guard_violations.load() == 0 ? 0 : 1;
}
