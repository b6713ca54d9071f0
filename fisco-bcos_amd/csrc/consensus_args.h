// consensus_args.h -- the arguments of the block-header check and the PBFT message check, shared by their
// launchers (engine.h, header_kernels.hip, pbft_kernels.hip) and by the host code that stages them
// (consensus_stage.h).  Host-only: no HIP header.
#pragma once
#include <stdint.h>

namespace bcosgpu {

// header_kernels.hip: the block-header check (hash, known-key verify of the rows, verdict and parent link); the
// arguments are bcosgpu_headers_check_dev's, all device pointers
struct HeadersCheckArgs {
    const uint8_t* d_pre = nullptr;
    const uint64_t* d_pre_off = nullptr;
    const uint8_t* d_given32 = nullptr;     // nullable, with d_given_mask
    const uint8_t* d_given_mask = nullptr;
    const uint8_t* d_pre_status = nullptr;
    const int64_t* d_number = nullptr;
    const int64_t* d_parent_number = nullptr;
    const uint8_t* d_parent_hash32 = nullptr;
    const uint8_t* d_parent_ok = nullptr;
    const uint8_t* d_prev_hash32 = nullptr;  // nullable
    int64_t prev_number = 0;
    const uint64_t* d_sig_off = nullptr;
    const uint8_t* d_sig = nullptr;
    const uint64_t* d_row_weight = nullptr;
    const int32_t* d_row_slot = nullptr;     // exactly one of d_row_slot, d_row_pub64
    const uint8_t* d_row_pub64 = nullptr;
    uint64_t quorum = 0, n = 0, rows = 0;
    uint8_t* d_hash32 = nullptr;
    uint8_t* d_check = nullptr;
    uint8_t* d_link = nullptr;
    uint8_t* d_sig_ok = nullptr;             // nullable
    void* d_work = nullptr;
    uint64_t work_bytes = 0;
};

// pbft_kernels.hip: the signatures of a drained PBFT message queue (hash, known-key verify of the rows, message
// and prepared-proposal verdicts, NewView groups); the arguments are bcosgpu_pbft_check_dev's, all device pointers
struct PbftCheckArgs {
    const uint8_t* d_data = nullptr;
    const uint64_t* d_data_off = nullptr;
    const uint8_t* d_given32 = nullptr;      // nullable, with d_given_mask
    const uint8_t* d_given_mask = nullptr;
    const uint8_t* d_pre_flags = nullptr;
    const uint64_t* d_msg_weight = nullptr;
    const uint8_t* d_checks = nullptr;
    const int64_t* d_msg_row = nullptr;
    const int64_t* d_prop_row = nullptr;
    const uint64_t* d_prep_off = nullptr;
    const uint64_t* d_prep_row_off = nullptr;
    uint64_t nprep = 0;
    uint8_t* d_row_hash32 = nullptr;         // in / out: the message rows are written
    const uint8_t* d_sig = nullptr;
    const uint64_t* d_row_weight = nullptr;
    const int32_t* d_row_slot = nullptr;     // exactly one of d_row_slot, d_row_pub64
    const uint8_t* d_row_pub64 = nullptr;
    const uint64_t* d_groups = nullptr;      // nullable when ngroups == 0
    uint64_t ngroups = 0, quorum = 0, n = 0, rows = 0;
    uint8_t* d_msg_hash32 = nullptr;
    uint32_t* d_msg_flags = nullptr;
    uint8_t* d_prepared_check = nullptr;
    uint8_t* d_sig_ok = nullptr;             // nullable
    void* d_work = nullptr;
    uint64_t work_bytes = 0;
};

}  // namespace bcosgpu
