// cipher_host_check -- csrc/cipher_host.h against the standards' vectors (host-only, no device).
//   (no arguments)                               FIPS-197 C.3, SP 800-38A F.2.5 / F.2.6, GB/T 32907 A.1, key and IV
//                                                normalisation, padding and the decrypt failures; prints
//                                                "cipher_host_check: ok"
//   schedule <aes256|sm4> <enc|dec> <keyhex>     the schedule's words as hex, one line (tests/test_cipher.py
//                                                compares them with its restatement's)
//   cbc <aes256|sm4> <enc|dec> <keyhex> <ivhex|-> <datahex>    one value through cbc_encrypt / cbc_decrypt:
//                                                "<status> <hex>"
//   bench <aes256|sm4> <enc|dec> <threads> <file>   the CPU line of tools/cipher_bench.py: the packed values of
//                                                <file> (u64 n, u64 off[n+1], data) through cbc_* on <threads>
//                                                threads, best of five; prints the seconds
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>
#include "../csrc/cipher_host.h"

using namespace bcosgpu::cipher;
using Bytes = std::vector<uint8_t>;

static int g_fail = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                    \
        }                                                                \
    } while (0)

static Bytes unhex(const std::string& s) {
    Bytes b;
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back(static_cast<uint8_t>(std::stoi(s.substr(i, 2), nullptr, 16)));
    return b;
}
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) s += d[p[i] >> 4], s += d[p[i] & 15];
    return s;
}
static std::string hex(const Bytes& b) { return hex(b.data(), b.size()); }

static Bytes encrypt(int cipher, const Bytes& key, const Bytes* iv, const Bytes& in) {
    const Schedule s = make_schedule(cipher, false, key.data(), key.size(), iv ? iv->data() : nullptr, iv ? iv->size() : 0);
    Bytes out(cbc_padded_size(in.size()));
    cbc_encrypt(cipher, s, in.data(), in.size(), out.data());
    return out;
}
static int decrypt(int cipher, const Bytes& key, const Bytes* iv, const Bytes& in, Bytes& out) {
    const Schedule s = make_schedule(cipher, true, key.data(), key.size(), iv ? iv->data() : nullptr, iv ? iv->size() : 0);
    out.assign(in.size(), 0);
    uint64_t n = 0;
    const int st = cbc_decrypt(cipher, s, in.data(), in.size(), out.data(), &n);
    out.resize(n);
    return st;
}

static void vectors() {
    // FIPS-197 C.3: AES-256, key 00..1f, plaintext 00112233..ff
    {
        const Bytes key = unhex("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f");
        const Bytes pt = unhex("00112233445566778899aabbccddeeff");
        const Schedule e = make_schedule(kAes256, false, key.data(), key.size(), nullptr, 0);
        const Schedule d = make_schedule(kAes256, true, key.data(), key.size(), nullptr, 0);
        uint8_t ct[16], back[16];
        encrypt_block(kAes256, e, pt.data(), ct);
        CHECK(hex(ct, 16) == "8ea2b7ca516745bfeafc49904b496089");
        decrypt_block(kAes256, d, ct, back);
        CHECK(hex(back, 16) == hex(pt));
    }
    // SP 800-38A F.2.5 / F.2.6: CBC-AES256, four blocks (the fifth is this build's padding block)
    {
        const Bytes key = unhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4");
        const Bytes iv = unhex("000102030405060708090a0b0c0d0e0f");
        const Bytes pt = unhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
                               "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710");
        const std::string want = "f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d"
                                 "39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b";
        const Bytes ct = encrypt(kAes256, key, &iv, pt);
        CHECK(ct.size() == 80 && hex(ct.data(), 64) == want);
        Bytes back;
        CHECK(decrypt(kAes256, key, &iv, ct, back) == kStatusOk && back == pt);
    }
    // GB/T 32907-2016 A.1: key = block = 0123456789abcdeffedcba9876543210
    {
        const Bytes key = unhex("0123456789abcdeffedcba9876543210");
        const Schedule e = make_schedule(kSm4, false, key.data(), key.size(), nullptr, 0);
        const Schedule d = make_schedule(kSm4, true, key.data(), key.size(), nullptr, 0);
        uint8_t ct[16], back[16];
        encrypt_block(kSm4, e, key.data(), ct);
        CHECK(hex(ct, 16) == "681edf34d206965e86b3e94f536e4246");
        decrypt_block(kSm4, d, ct, back);
        CHECK(hex(back, 16) == hex(key));
        CHECK(e.rk[0] == 0xf12186f9u && e.rk[31] == 0x9124a012u);  // A.1's rk[0] and rk[31]
    }
    // key and IV rules, padding sizes, round trips and the decrypt failures, for both ciphers
    for (int cipher : {kAes256, kSm4}) {
        const int K = key_bytes(cipher);
        const Bytes shortk = {'a', 'b', 'c', 'd'};
        Bytes padded(shortk);
        padded.resize(K, 0);
        Bytes longk(69);
        for (size_t i = 0; i < longk.size(); ++i) longk[i] = static_cast<uint8_t>(7 * i + 1);
        const Bytes cut(longk.begin(), longk.begin() + K);
        Bytes iv47(47), iv16;
        for (size_t i = 0; i < iv47.size(); ++i) iv47[i] = static_cast<uint8_t>(200 - i);
        iv16.assign(iv47.begin(), iv47.begin() + 16);
        const Bytes zero_iv16 = {'a', 'b', 'c', 'd', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t len : {0u, 1u, 15u, 16u, 17u, 31u, 32u, 33u, 47u, 48u, 1000u}) {
            Bytes pt(len);
            for (size_t i = 0; i < len; ++i) pt[i] = static_cast<uint8_t>(i * 31 + len);
            const Bytes ct = encrypt(cipher, shortk, nullptr, pt);
            CHECK(ct.size() == (len / 16 + 1) * 16);
            CHECK(ct == encrypt(cipher, padded, &zero_iv16, pt));  // short key: zero-filled key, zero-filled default IV
            CHECK(encrypt(cipher, longk, &iv47, pt) == encrypt(cipher, cut, &iv16, pt));  // both cut
            const Bytes first16(longk.begin(), longk.begin() + 16);
            CHECK(encrypt(cipher, longk, nullptr, pt) == encrypt(cipher, cut, &first16, pt));  // default IV: raw key
            Bytes back;
            CHECK(decrypt(cipher, shortk, nullptr, ct, back) == kStatusOk && back == pt);
            Bytes bad(ct);
            bad.push_back(0);
            CHECK(decrypt(cipher, shortk, nullptr, bad, back) == kStatusBadLength && back.empty());
        }
        Bytes back;
        CHECK(decrypt(cipher, shortk, nullptr, Bytes(), back) == kStatusBadLength);
        // forged padding: encrypt raw blocks (no padding of ours) whose last byte is 0, 17, or a broken run
        for (int kind = 0; kind < 4; ++kind) {
            uint8_t blk[16];
            for (int i = 0; i < 16; ++i) blk[i] = kind == 0 ? 0 : kind == 1 ? 17 : 4;
            if (kind == 2) blk[13] = 5;  // ..., 5, 4, 4 with p = 4: one wrong
            const Schedule e = make_schedule(cipher, false, shortk.data(), shortk.size(), nullptr, 0);
            uint32_t w[4];
            load_block(cipher, blk, w);
            for (int i = 0; i < 4; ++i) w[i] ^= e.iv[i];
            encrypt_words(cipher, e, w);
            Bytes ct(16);
            store_block(cipher, ct.data(), w);
            const int st = decrypt(cipher, shortk, nullptr, ct, back);
            CHECK(st == (kind == 3 ? kStatusOk : kStatusBadPadding));
            CHECK(back.size() == (kind == 3 ? 12u : 0u));
        }
    }
}

static int cipher_of(const std::string& s) { return s == "sm4" ? kSm4 : s == "aes256" ? kAes256 : -1; }

static int bench(int cipher, bool dec, int threads, const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    uint64_t n = 0;
    if (std::fread(&n, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> off(n + 1);
    if (std::fread(off.data(), 8, n + 1, f) != n + 1) return 2;
    Bytes data(off[n] + 1);
    if (off[n] && std::fread(data.data(), 1, off[n], f) != off[n]) return 2;
    std::fclose(f);
    std::vector<uint64_t> ooff(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) ooff[i + 1] = ooff[i] + (dec ? off[i + 1] - off[i] : cbc_padded_size(off[i + 1] - off[i]));
    Bytes out(ooff[n] + 1);
    const uint8_t key[32] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20};
    const Schedule s = make_schedule(cipher, dec, key, 32, nullptr, 0);
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                for (uint64_t i = n * t / threads; i < n * (t + 1) / threads; ++i) {
                    uint64_t m = 0;
                    if (dec) (void)cbc_decrypt(cipher, s, data.data() + off[i], off[i + 1] - off[i], out.data() + ooff[i], &m);
                    else cbc_encrypt(cipher, s, data.data() + off[i], off[i + 1] - off[i], out.data() + ooff[i]);
                }
            });
        for (auto& th : pool) th.join();
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (dt < best) best = dt;
    }
    std::printf("%.9f\n", best);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "schedule" && argc == 5) {
        const int cipher = cipher_of(argv[2]);
        if (cipher < 0) return 2;
        const Bytes key = unhex(argv[4]);
        const Schedule s = make_schedule(cipher, std::string(argv[3]) == "dec", key.data(), key.size(), nullptr, 0);
        for (int i = 0; i < (cipher == kSm4 ? kSm4Words : kAesWords); ++i) std::printf("%08x", s.rk[i]);
        std::printf(" ");
        for (int i = 0; i < 4; ++i) std::printf("%08x", s.iv[i]);
        std::printf("\n");
        return 0;
    }
    if (mode == "cbc" && argc == 7) {
        const int cipher = cipher_of(argv[2]);
        if (cipher < 0) return 2;
        const Bytes key = unhex(argv[4]), iv = unhex(argv[5]), in = unhex(argv[6]);
        const Bytes* ivp = std::string(argv[5]) == "-" ? nullptr : &iv;
        if (std::string(argv[3]) == "dec") {
            Bytes out;
            const int st = decrypt(cipher, key, ivp, in, out);
            std::printf("%d %s\n", st, hex(out).c_str());
        } else {
            std::printf("0 %s\n", hex(encrypt(cipher, key, ivp, in)).c_str());
        }
        return 0;
    }
    if (mode == "bench" && argc == 6) {
        const int cipher = cipher_of(argv[2]);
        if (cipher < 0) return 2;
        return bench(cipher, std::string(argv[3]) == "dec", std::atoi(argv[4]), argv[5]);
    }
    if (argc > 1) {
        std::printf("usage: cipher_host_check [schedule|cbc|bench ...]\n");
        return 2;
    }
    vectors();
    if (g_fail) return 1;
    std::printf("cipher_host_check: ok\n");
    return 0;
}
