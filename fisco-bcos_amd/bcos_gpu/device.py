"""Device-resident entry points over torch tensors (HBM-resident inputs, stream-ordered launches).

PyTorch only provides the device memory and the stream here; the compute is libbcosgpu.so.
Every function takes uint8 / int64 CUDA tensors and launches on torch's current stream (or the
given one) without synchronising.
"""
import torch

from . import _lib
from ._lib import check, ensure_device, lib

KECCAK256, SM3 = _lib.KECCAK256, _lib.SM3
SUITE_SECP256K1, SUITE_SM2 = _lib.SUITE_SECP256K1, _lib.SUITE_SM2


def _s(stream):
    return (stream if stream is not None else torch.cuda.current_stream()).cuda_stream


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA tensors"
    return t.data_ptr()


def _dev(t):
    ensure_device(t.device.index if t.device.index is not None else 0)


def hash_batch(hasher, data, offsets, out, stream=None):
    """data uint8[B], offsets int64[n+1], out uint8[n,32]."""
    _dev(out)
    n = offsets.numel() - 1
    check(lib().bcosgpu_hash_batch_dev(hasher, _p(data), _p(offsets), n, _p(out), _s(stream)))


def state_root_work_size(n):
    return int(lib().bcosgpu_state_root_work_size(n))


def state_root(hasher, block_version, data, off3, kind, work, root, stream=None):
    """The state root of n packed storage entries (bcosgpu_state_root_dev; the layout of
    state.pack_state_entries): data uint8[B], off3 int64[3n+1], kind uint8[n], work uint8[>=
    state_root_work_size(n)], root uint8[32]."""
    _dev(root)
    n = kind.numel()
    assert off3.numel() == 3 * n + 1
    check(lib().bcosgpu_state_root_dev(hasher, block_version, _p(data), _p(off3), _p(kind), n, _p(work),
                                       work.numel() * work.element_size(), _p(root), _s(stream)))


CIPHER_AES256, CIPHER_SM4 = _lib.CIPHER_AES256, _lib.CIPHER_SM4


def cbc_work_size(n):
    return int(lib().bcosgpu_cbc_work_size(n))


def cbc_encrypt(cipher, key, data, offsets, out, out_off, work, iv=None, stream=None):
    """CBC + PKCS#7 over n packed values under one key (bcosgpu_cbc_encrypt_batch_dev): key / iv host bytes
    (iv None: the default IV), data uint8[B], offsets int64[n+1], out uint8[sum of (len // 16 + 1) * 16] (16-byte
    aligned), out_off int64[n+1] (written), work uint8[>= cbc_work_size(n)]."""
    _dev(out)
    n = offsets.numel() - 1
    assert out_off.numel() == n + 1
    check(lib().bcosgpu_cbc_encrypt_batch_dev(cipher, key, len(key), iv, 0 if iv is None else len(iv), _p(data),
                                              _p(offsets), n, _p(out), _p(out_off), _p(work),
                                              work.numel() * work.element_size(), _s(stream)))


def cbc_decrypt(cipher, key, data, offsets, out, out_len, status, iv=None, stream=None):
    """The inverse over n packed ciphertexts (bcosgpu_cbc_decrypt_batch_dev): data uint8[B] (16-byte aligned),
    offsets int64[n+1] (multiples of 16), out uint8[B] (not data: item i's plaintext at offsets[i], padding
    included), out_len int32[n] (read as u32), status uint8[n] (0 ok, 1 bad length, 2 bad padding)."""
    _dev(out)
    n = offsets.numel() - 1
    assert out_len.numel() == n and status.numel() == n
    check(lib().bcosgpu_cbc_decrypt_batch_dev(cipher, key, len(key), iv, 0 if iv is None else len(iv), _p(data),
                                              _p(offsets), n, _p(out), _p(out_len), _p(status), _s(stream)))


def headers_check_work_size(n, rows):
    return int(lib().bcosgpu_headers_check_work_size(n, rows))


def headers_check(suite, pre, pre_off, pre_status, number, parent_number, parent_hash, parent_ok, sig_off, sig,
                  row_weight, quorum, hashes, check_out, link, work, given=None, given_mask=None, prev_hash=None,
                  prev_number=0, row_slot=None, row_pub=None, sig_ok=None, stream=None):
    """The block-header check of n headers over `rows` signature rows (bcosgpu_headers_check_dev): pre uint8[B],
    pre_off int64[n+1], pre_status uint8[n], number / parent_number int64[n], parent_hash uint8[n,32], parent_ok
    uint8[n], sig_off int64[n+1], sig uint8[rows,64], row_weight int64[rows] (read as u64), exactly one of
    row_slot int32[rows] / row_pub uint8[rows,64]; given uint8[n,32] with given_mask uint8[n], prev_hash
    uint8[32] and sig_ok uint8[rows] may be None -> hashes uint8[n,32], check_out uint8[n], link uint8[n]."""
    _dev(hashes)
    n = pre_off.numel() - 1
    rows = row_weight.numel()
    check(lib().bcosgpu_headers_check_dev(suite, _p(pre), _p(pre_off), _p(given), _p(given_mask), _p(pre_status),
                                          _p(number), _p(parent_number), _p(parent_hash), _p(parent_ok),
                                          _p(prev_hash), prev_number, _p(sig_off), _p(sig), _p(row_weight),
                                          _p(row_slot), _p(row_pub), quorum, n, rows, _p(hashes), _p(check_out),
                                          _p(link), _p(sig_ok), _p(work), work.numel() * work.element_size(),
                                          _s(stream)))


def pbft_check_work_size(n, rows):
    return int(lib().bcosgpu_pbft_check_work_size(n, rows))


def pbft_check(suite, data, data_off, pre_flags, msg_weight, checks, msg_row, prop_row, prep_off, prep_row_off,
               row_hash, sig, row_weight, quorum, msg_hash, msg_flags, prepared_check, work, given=None,
               given_mask=None, row_slot=None, row_pub=None, groups=None, sig_ok=None, stream=None):
    """The signature checks of n PBFT messages over `rows` signature rows (bcosgpu_pbft_check_dev): data uint8[B],
    data_off int64[n+1], pre_flags uint8[n], msg_weight int64[n] (read as u64), checks uint8[n], msg_row /
    prop_row int64[n], prep_off int64[n+1], prep_row_off int64[nprep+1], row_hash uint8[rows,32] (in / out: the
    message rows are written), sig uint8[rows,64], row_weight int64[rows] (read as u64), exactly one of row_slot
    int32[rows] / row_pub uint8[rows,64]; given uint8[n,32] with given_mask uint8[n], groups int64[ngroups,3]
    and sig_ok uint8[rows] may be None -> msg_hash uint8[n,32], msg_flags int32[n], prepared_check uint8[nprep]."""
    _dev(msg_hash)
    n = data_off.numel() - 1
    rows = row_weight.numel()
    nprep = prep_row_off.numel() - 1
    ngroups = groups.numel() // 3 if groups is not None else 0
    check(lib().bcosgpu_pbft_check_dev(suite, _p(data), _p(data_off), _p(given), _p(given_mask), _p(pre_flags),
                                       _p(msg_weight), _p(checks), _p(msg_row), _p(prop_row), _p(prep_off),
                                       _p(prep_row_off), nprep, _p(row_hash), _p(sig), _p(row_weight), _p(row_slot),
                                       _p(row_pub), _p(groups) if ngroups else None, ngroups, quorum, n, rows,
                                       _p(msg_hash), _p(msg_flags), _p(prepared_check), _p(sig_ok), _p(work),
                                       work.numel() * work.element_size(), _s(stream)))


def merkle_size(n, width):
    return int(lib().bcosgpu_merkle_size(n, width))


def merkle_root(hasher, width, leaves, tree, root, stream=None):
    """leaves uint8[n,32]; tree uint8[merkle_size(n,width),32]; root uint8[32]."""
    _dev(leaves)
    check(lib().bcosgpu_merkle_root_dev(hasher, width, _p(leaves), leaves.shape[0], _p(tree), _p(root),
                                        _s(stream)))


def merkle_frontier(hasher, width, leaves, levels, work, frontier, stream=None):
    """Reference-tree level `levels` over a width^levels-aligned shard (bcosgpu_merkle_frontier_dev)."""
    _dev(leaves)
    check(lib().bcosgpu_merkle_frontier_dev(hasher, width, _p(leaves), leaves.shape[0], levels, _p(work),
                                            _p(frontier), _s(stream)))


def merkle_roots_work_size(total_leaves, nblocks, width):
    return int(lib().bcosgpu_merkle_roots_work_size(total_leaves, nblocks, width))


def merkle_roots_batch(hasher, width, leaves, block_off, work, roots, stream=None):
    """Roots of many blocks' trees (bcosgpu_merkle_roots_batch_dev).  leaves uint8[N,32] (device),
    block_off: host uint64 numpy array [nblocks+1] of row indices into `leaves`, work: uint8 device
    tensor >= merkle_roots_work_size bytes, roots uint8[nblocks,32]."""
    import ctypes
    import numpy as np
    _dev(leaves)
    bo = np.ascontiguousarray(block_off, dtype=np.uint64)
    nb = bo.size - 1
    base = leaves[int(bo[0]):] if nb > 0 and int(bo[0]) < leaves.shape[0] else leaves
    check(lib().bcosgpu_merkle_roots_batch_dev(hasher, width, _p(base), bo.ctypes.data_as(ctypes.c_void_p), nb,
                                               _p(work), _p(roots), _s(stream)))


def verify(suite, pubs, hashes, sigs, ok, stream=None):
    """SignatureCrypto::verify with the keys given (bcosgpu_verify_batch_dev): pubs uint8[n,64], hashes
    uint8[n,32], sigs uint8[n, stride >= 64] (r || s read) -> ok uint8[n].  The generic kernels: no key lookup."""
    _dev(ok)
    n = pubs.shape[0]
    assert hashes.shape[0] == n and sigs.shape[0] == n and ok.numel() == n
    check(lib().bcosgpu_verify_batch_dev(suite, _p(pubs), _p(hashes), _p(sigs), sigs.shape[1] if n else 64, n, _p(ok),
                                         _s(stream)))


def verify_keyed(suite, slots, hashes, sigs, ok, stream=None):
    """SignatureCrypto::verify against registered keys (bcosgpu_verify_keyed_batch_dev): slots int32[n]
    (from _lib.register_keys), hashes uint8[n,32], sigs uint8[n, stride >= 64] (r || s read) -> ok uint8[n]."""
    _dev(ok)
    n = slots.numel()
    check(lib().bcosgpu_verify_keyed_batch_dev(suite, _p(slots), _p(hashes), _p(sigs), sigs.shape[1] if n else 64, n,
                                               _p(ok), _s(stream)))


def secp256k1_recover(hashes, sigs, pub, addr, ok, stream=None):
    """hashes uint8[n,32], sigs uint8[n,65] -> pub uint8[n,64] (or None), addr uint8[n,20] (or None), ok uint8[n]."""
    _dev(hashes)
    check(lib().bcosgpu_secp256k1_recover_batch_dev(_p(hashes), _p(sigs), hashes.shape[0], _p(pub), _p(addr),
                                                    _p(ok), _s(stream)))


def sm2_verify(hashes, sigs, addr, ok, stream=None):
    """hashes uint8[n,32], sigs uint8[n,128] (r||s||pub) -> addr uint8[n,20] (or None), ok uint8[n]."""
    _dev(hashes)
    check(lib().bcosgpu_sm2_verify_batch_dev(_p(hashes), _p(sigs), hashes.shape[0], _p(addr), _p(ok), _s(stream)))


def secp256k1_sign(sks, hashes, pub, sigs, ok, stream=None):
    _dev(sks)
    check(lib().bcosgpu_secp256k1_sign_batch_dev(_p(sks), _p(hashes), sks.shape[0], _p(pub), _p(sigs), _p(ok),
                                                 _s(stream)))


def sm2_sign(sks, hashes, sigs, ok, stream=None):
    _dev(sks)
    check(lib().bcosgpu_sm2_sign_batch_dev(_p(sks), _p(hashes), sks.shape[0], _p(sigs), _p(ok), _s(stream)))


def tx_verify(suite, pre, pre_off, sig, sig_off, txhash, sender, status, stream=None):
    """Batched Transaction::verify; all device tensors (see bcosgpu_tx_verify_batch_dev)."""
    _dev(pre)
    n = pre_off.numel() - 1
    check(lib().bcosgpu_tx_verify_batch_dev(suite, _p(pre), _p(pre_off), _p(sig), _p(sig_off), n, _p(txhash),
                                            _p(sender), _p(status), _s(stream)))


def tars_decode_work_size(n):
    return int(lib().bcosgpu_tars_decode_work_size(n))


def tars_tx_decode(enc, enc_off, pre, pre_off, sig, sig_off, dec_status, work, stream=None):
    """Device Tars decode of n transactions into the packed preimage / signature layout
    (bcosgpu_tars_tx_decode_dev); dec_status may be None."""
    _dev(enc)
    n = enc_off.numel() - 1
    check(lib().bcosgpu_tars_tx_decode_dev(_p(enc), _p(enc_off), n, _p(pre), _p(pre_off), _p(sig), _p(sig_off),
                                           None if dec_status is None else _p(dec_status), _p(work),
                                           work.numel() * work.element_size(), _s(stream)))


def tars_tx_verify(suite, enc, enc_off, pre, pre_off, sig, sig_off, work, txhash, sender, status, check_sig=True,
                   check_hash=False, stream=None):
    """Device createTransaction: decode + hash (+ Transaction::verify when check_sig)
    (bcosgpu_tars_tx_verify_batch_dev)."""
    _dev(enc)
    n = enc_off.numel() - 1
    check(lib().bcosgpu_tars_tx_verify_batch_dev(suite, _p(enc), _p(enc_off), n, int(bool(check_sig)),
                                                 int(bool(check_hash)), _p(pre),
                                                 _p(pre_off), _p(sig), _p(sig_off), _p(work),
                                                 work.numel() * work.element_size(), _p(txhash), _p(sender),
                                                 _p(status), _s(stream)))


TXPOOL_FULL, TXPOOL_PROPOSAL = 0, 1


def txpool_admit(pool, enc, enc_off, txhash, sender, nonce, status, mode=TXPOOL_FULL):
    """Stateful admission of n Tars-encoded transactions over device tensors (bcosgpu_txpool_admit_dev): `pool` a
    bcos_gpu.txpool.Pool; enc uint8[B], enc_off int64[n+1], txhash uint8[n,32], sender uint8[n,20], nonce
    uint8[n,32], status int32[n].  Runs on the pool's own stream: this waits for torch's current stream first,
    and the outputs are complete when it returns."""
    _dev(enc)
    n = enc_off.numel() - 1
    assert status.element_size() == 4 and enc.numel() < 2 ** 63
    torch.cuda.current_stream().synchronize()
    check(lib().bcosgpu_txpool_admit_dev(pool.handle, mode, _p(enc), _p(enc_off), n, enc.numel(), _p(txhash),
                                         _p(sender), _p(nonce), _p(status)))
