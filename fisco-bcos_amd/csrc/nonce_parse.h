// nonce_parse.h -- TransactionImpl::nonce() (bcos-tars-protocol/.../protocol/TransactionImpl.cpp:62-68) for
// canonical nonce strings, one __host__ __device__ function in the manner of tars_decode.h (host build:
// tests/cpp/txpool_host_test.cpp; no kernel calls it yet): an empty string is 0, anything else goes
// through boost::lexical_cast<u256>.
// Boost's stream parser has corners this library does not restate (octal after a leading 0, signs, what happens
// past 256 bits), so exactly the canonical form is parsed -- what BlockImpl::setNonceList writes and SDKs send:
//   empty, or 1..78 ASCII digits with no leading '0' unless the string is "0", and a value below 2^256.
// Everything else returns false: such a transaction is to be handed back to the host's own code.
// The value is the 32-byte big-endian key of the nonce sets.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NONCE_HD __host__ __device__ inline
#else
#define NONCE_HD inline
#endif

namespace bcosgpu {

constexpr uint32_t kNonceMaxDigits = 78;  // 2^256 - 1 has 78 decimal digits

// s[0 .. len) -> out32 (big-endian); false: not canonical (out32 is then unspecified)
NONCE_HD bool parse_canonical_nonce(const uint8_t* s, uint32_t len, uint8_t* out32) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // little-endian limbs
    if (len > kNonceMaxDigits) return false;
    if (len > 1 && s[0] == '0') return false;
    uint32_t i = 0;
    // terminates: every pass consumes 1..9 digits of the at most 78
    while (i < len) {
        // up to nine digits at a time: value = value * 10^k + chunk (chunk < 10^9 < 2^32)
        uint32_t k = (len - i) % 9u;
        if (k == 0) k = 9;
        uint32_t chunk = 0, scale = 1;
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t d = static_cast<uint32_t>(s[i + j]) - '0';
            if (d > 9u) return false;
            chunk = chunk * 10u + d;
            scale *= 10u;
        }
        uint64_t carry = chunk;
        for (int l = 0; l < 8; ++l) {
            const uint64_t t = static_cast<uint64_t>(w[l]) * scale + carry;
            w[l] = static_cast<uint32_t>(t);
            carry = t >> 32;
        }
        if (carry) return false;  // >= 2^256
        i += k;
    }
    for (int l = 0; l < 8; ++l) {
        const uint32_t v = w[7 - l];
        out32[4 * l + 0] = static_cast<uint8_t>(v >> 24);
        out32[4 * l + 1] = static_cast<uint8_t>(v >> 16);
        out32[4 * l + 2] = static_cast<uint8_t>(v >> 8);
        out32[4 * l + 3] = static_cast<uint8_t>(v);
    }
    return true;
}

}  // namespace bcosgpu
