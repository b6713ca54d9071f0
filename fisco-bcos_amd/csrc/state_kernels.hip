// state_kernels.hip -- the state root: a fused hash-and-XOR reduction over packed storage entries (gfx950).
//
// Replaces, for a block's dirty entries:
//   StateStorage::hash            bcos-table/src/StateStorage.h:397-431
//     XOR over dirty entries of H(table) ^ H(key) ^ Entry::hash(table, key, H, blockVersion)
//   KeyPageStorage::hash          bcos-table/src/KeyPageStorage.cpp:351-406   (system-table entries: the same sum)
//   PageData::hash                bcos-table/src/KeyPageStorage.h:862-893     (page entries: Entry::hash alone from
//                                 3.1 on, with H(table) ^ H(key) at 3.0 -- the caller's per-entry XOR_NAMES flag)
//   Entry::hash                   bcos-framework/bcos-framework/storage/Entry.h:229-309
//     >= V3_1_VERSION: MODIFIED H(table || key || value), DELETED H(table || key)
//     3.0:             MODIFIED H(value),                 DELETED HashType(0x1) (FixedBytes.h:171)
//     a clean entry (NORMAL, EMPTY) is not dirty: nothing
//
// Input is the layout of bcosgpu_pack_state_entries (pack.cpp): table || key || value back to back, off3[3i + j]
// the start of entry i's part j, so every message above is one contiguous slice.  An entry has up to three
// jobs -- 0 the entry hash, 1 H(table), 2 H(key) -- and a lane runs one job (the default) or one entry's
// three.  Jobs are laid out kind-major (lanes [0, n) the entry hashes, [n, 2n) the tables, [2n, 3n) the keys):
// a wave then holds one kind, so the one-block name hashes never wait on a long value beside them, and with
// XOR_NAMES on no entry the name waves leave at once.  Digests never reach memory: a lane's digest is XORed
// across the wave in registers (__shfl_xor), across the workgroup's waves through LDS, and each workgroup
// stores one 32-byte partial into the slab in d_work, which state_fold_kernel XORs into the root.  Every
// slab row the fold reads is written by this call's kernels, so d_work's earlier contents never matter.
// Entry lengths are wildly mixed (32-byte slots beside contract code of tens of kilobytes), and a wave costs its
// longest message: an entry hash over more than kStateLongBytes is therefore not run in place but listed
// (a vector atomicAdd on a count the launcher zeroes on the stream), and state_long_kernel hashes the list
// with the long messages sharing waves.  The list's order varies from run to run; the XOR does not.
// XOR commutes with the byte swap of SM3's big-endian words, so partials stay in the hasher's word order
// until the fold stores the root.
#include <cstdlib>
#include <cstring>
#include "hash_device.h"
#include "engine.h"

namespace bcosgpu {

namespace {

constexpr int kStateThreads = 256;
constexpr uint32_t kEntryDeleted = BCOSGPU_ENTRY_DELETED, kEntryModified = BCOSGPU_ENTRY_MODIFIED;

// XOR of d[0..8) over the workgroup -> row[0..8) (written by threads 0..7)
__device__ __forceinline__ void block_xor_store(uint32_t d[8], uint32_t* __restrict__ row) {
    __shared__ uint32_t part[kStateThreads / 64][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) d[k] ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(d[k]), m, 64));
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) part[wave][k] = d[k];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < kStateThreads / 64; ++w) v ^= part[w][threadIdx.x];
        row[threadIdx.x] = v;
    }
}

// The slice job 0 (the entry hash) of a dirty entry hashes; false for 3.0's DELETED constant.
__device__ __forceinline__ bool entry_slice(const uint64_t* __restrict__ o, uint32_t st, int v31, uint64_t& a,
                                            uint64_t& b) {
    if (v31) {  // Entry.h:233-278
        a = o[0], b = st == kEntryModified ? o[3] : o[2];
        return true;
    }
    a = o[2], b = o[3];  // Entry.h:281-292
    return st == kEntryModified;
}

// PER_ENTRY: lane t runs the three jobs of entry t; else lane t runs job t / n of entry t % n.  An entry hash
// over more than long_len bytes is not run here: its entry index is appended to long_list (*long_count,
// zeroed by the launcher on the stream), which state_long_kernel hashes in full waves.
template <int H, bool PER_ENTRY>
__global__ __launch_bounds__(kStateThreads) void state_root_kernel(const uint8_t* __restrict__ data,
                                                                   const uint64_t* __restrict__ off3,
                                                                   const uint8_t* __restrict__ kind, uint64_t n,
                                                                   int v31, uint32_t long_len,
                                                                   uint32_t* __restrict__ long_count,
                                                                   uint32_t* __restrict__ long_list,
                                                                   uint32_t* __restrict__ slab) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kStateThreads + threadIdx.x;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int job = 0, jobs = 0;
    uint64_t i = t;
    if (PER_ENTRY) {
        jobs = t < n ? 3 : 0;
    } else if (t < 3 * n) {
        job = t >= 2 * n ? 2 : t >= n ? 1 : 0;
        i = t - static_cast<uint64_t>(job) * n;
        jobs = job + 1;
    }
    if (jobs) {
        const uint32_t kd = kind[i], st = kd & 15u;
        const bool names = ((kd >> 4) & BCOSGPU_STATE_XOR_NAMES) != 0;
        if (st != kEntryDeleted && st != kEntryModified) jobs = 0;  // clean: Entry.h:269-274, StateStorage.h:412
        else if (!names && jobs > 1) jobs = PER_ENTRY ? 1 : 0;
        const uint64_t* o = off3 + 3 * i;
#pragma unroll 1
        for (; job < jobs; ++job) {
            uint64_t a, b;
            if (job == 1) {
                a = o[0], b = o[1];
            } else if (job == 2) {
                a = o[1], b = o[2];
            } else if (!entry_slice(o, st, v31, a, b)) {  // HashType(0x1): 31 zero bytes, then 0x01 (Entry.h:293-295)
                acc[7] ^= H == SM3 ? 1u : 0x01000000u;
                continue;
            }
            const uint32_t len = static_cast<uint32_t>(b - a);
            if (job == 0 && len > long_len) {
                long_list[atomicAdd(long_count, 1u)] = static_cast<uint32_t>(i);
                continue;
            }
            FlatReader rd(data + a, len);
            uint32_t d[8];
            if (H == KECCAK256) keccak256_msg(rd, len, d);
            else sm3_msg(rd, len, d);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] ^= d[k];
        }
    }
    block_xor_store(acc, slab + 8 * static_cast<uint64_t>(blockIdx.x));
}

// The entry hashes state_root_kernel left in long_list, one per lane: the long messages share waves, so a wave
// costs its longest message with every lane at work, not one lane's message with 63 lanes waiting.  The grid
// covers the most the list can hold; a workgroup past *long_count stores a zero row.
template <int H>
__global__ __launch_bounds__(kStateThreads) void state_long_kernel(const uint8_t* __restrict__ data,
                                                                   const uint64_t* __restrict__ off3,
                                                                   const uint8_t* __restrict__ kind, int v31,
                                                                   const uint32_t* __restrict__ long_count,
                                                                   const uint32_t* __restrict__ long_list,
                                                                   uint32_t* __restrict__ slab) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kStateThreads + threadIdx.x;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t < *long_count) {
        const uint64_t i = long_list[t];
        uint64_t a, b;
        if (entry_slice(off3 + 3 * i, kind[i] & 15u, v31, a, b)) {
            const uint32_t len = static_cast<uint32_t>(b - a);
            FlatReader rd(data + a, len);
            if (H == KECCAK256) keccak256_msg(rd, len, acc);
            else sm3_msg(rd, len, acc);
        }
    }
    block_xor_store(acc, slab + 8 * static_cast<uint64_t>(blockIdx.x));
}

// root = XOR of the slab's rows (one workgroup; rows == 0 gives the zero hash)
template <int H>
__global__ __launch_bounds__(kStateThreads) void state_fold_kernel(const uint32_t* __restrict__ slab, uint64_t rows,
                                                                   uint8_t* __restrict__ root) {
    const uint32_t word = threadIdx.x & 7u;
    uint32_t v = 0;
    for (uint64_t r = threadIdx.x >> 3; r < rows; r += kStateThreads / 8) v ^= slab[8 * r + word];
    __shared__ uint32_t part[kStateThreads];
    part[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x < 8) {
        uint32_t x = 0;
        for (int k = 0; k < kStateThreads / 8; ++k) x ^= part[8 * k + threadIdx.x];
        reinterpret_cast<uint32_t*>(root)[threadIdx.x] = H == SM3 ? bswap32(x) : x;
    }
}

uint64_t state_rows(uint64_t lanes) { return (lanes + kStateThreads - 1) / kStateThreads; }

// an entry hash over more bytes than this goes through the long list (8 Keccak / 16 SM3 blocks stay in place)
constexpr uint32_t kStateLongBytes = 1024;

}  // namespace

// d_work: the slab (one 32-byte row per workgroup of the one-lane-per-job grid, then of the long list's grid),
// the long list's count, the long list (one uint32 entry index per entry at most)
uint64_t state_root_work_bytes(uint64_t n) { return 32 * (state_rows(3 * n) + state_rows(n)) + 32 + 4 * n + 32; }

int launch_state_root(int hasher, uint32_t block_version, const uint8_t* d_data, const uint64_t* d_off3,
                      const uint8_t* d_kind, uint64_t n, void* d_work, uint64_t work_bytes, uint8_t* d_root,
                      hipStream_t st) {
    if (n > 0xFFFFFFFFull || (n && work_bytes < state_root_work_bytes(n))) return BCOSGPU_E_ARG;
    // the mapping, read once (the measurement's other legs, tools/state_root_bench.py): BCOSGPU_STATE_MAP=entry
    // runs one lane per entry, =flat one lane per job with no long list; anything else one lane per job and
    // the long list
    static const int map = [] {
        const char* e = std::getenv("BCOSGPU_STATE_MAP");
        return e && std::strcmp(e, "entry") == 0 ? 1 : e && std::strcmp(e, "flat") == 0 ? 2 : 0;
    }();
    const bool pe = map == 1;
    const uint32_t long_len = map == 2 ? 0xFFFFFFFFu : kStateLongBytes;
    const uint64_t rows = n ? state_rows(pe ? n : 3 * n) : 0, long_rows = n && map != 2 ? state_rows(n) : 0;
    uint32_t* slab = static_cast<uint32_t*>(d_work);
    uint32_t* long_count = slab + 8 * (state_rows(3 * n) + state_rows(n));
    uint32_t* long_list = long_count + 8;
    const int v31 = block_version >= 0x03010000u;  // BlockVersion::V3_1_VERSION
    const dim3 g(static_cast<unsigned>(rows)), gl(static_cast<unsigned>(long_rows)), b(kStateThreads);
    if (long_rows && hipMemsetAsync(long_count, 0, 4, st) != hipSuccess) return BCOSGPU_E_HIP;
#define STATE_ROOT(HH, PE)                                                                                        \
    hipLaunchKernelGGL((state_root_kernel<HH, PE>), g, b, 0, st, d_data, d_off3, d_kind, n, v31, long_len, long_count, \
                       long_list, slab)
#define STATE_LONG(HH)                                                                                             \
    hipLaunchKernelGGL(state_long_kernel<HH>, gl, b, 0, st, d_data, d_off3, d_kind, v31, long_count, long_list, \
                       slab + 8 * rows)
    if (rows) {
        if (hasher == SM3) {
            if (pe) STATE_ROOT(SM3, true); else STATE_ROOT(SM3, false);
            if (long_rows) STATE_LONG(SM3);
        } else {
            if (pe) STATE_ROOT(KECCAK256, true); else STATE_ROOT(KECCAK256, false);
            if (long_rows) STATE_LONG(KECCAK256);
        }
    }
#undef STATE_ROOT
#undef STATE_LONG
    if (hasher == SM3) hipLaunchKernelGGL(state_fold_kernel<SM3>, dim3(1), b, 0, st, slab, rows + long_rows, d_root);
    else hipLaunchKernelGGL(state_fold_kernel<KECCAK256>, dim3(1), b, 0, st, slab, rows + long_rows, d_root);
    return hipGetLastError() == hipSuccess ? 0 : BCOSGPU_E_HIP;
}

}  // namespace bcosgpu
