"""Header-side mirror: the block-header hash and the check a syncing node runs on every downloaded block.

  impl_calculate<Hasher>(BlockHeader)   bcos-tars-protocol/bcos-tars-protocol/impl/TarsHashable.h:77-126
  BlockValidator::asyncCheckBlock       bcos-pbft/bcos-pbft/pbft/engine/BlockValidator.cpp:28-182
  the ledger's parent check             bcos-ledger/src/libledger/LedgerImpl.h:290-312
"""
import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from ._lib import check, ensure_device, lib
from .crypto import _ptr
from .tx import _BytesView

HEADER_RECOMPUTE = 1
# check[] codes (a header is accepted iff the code is < 16) and link[] codes, as in include/bcos_gpu.h
HEADER_OK, HEADER_GENESIS, HEADER_NO_TXS = 0, 1, 2
HEADER_E_COMMITTED, HEADER_E_SEALER, HEADER_E_SEALER_LIST, HEADER_E_SIGNATURE, HEADER_E_QUORUM = 16, 17, 18, 19, 20
LINK_BROKEN, LINK_OK, LINK_UNCHECKED = 0, 1, 2
SIG_FAILED, SIG_OK, SIG_UNCHECKED = 0, 1, 2


@dataclass
class HeaderSignature:
    """bcostars::Signature (Block.tars): the sealer's index in the consensus node list and its signature."""
    index: int = 0
    signature: bytes = b""


@dataclass
class BlockHeader:
    """bcostars::BlockHeader as the check sees it; parents: (blockNumber, blockHash) pairs; tx_count is
    Block::transactionsSize()."""
    version: int = 0
    parents: List[Tuple[int, bytes]] = field(default_factory=list)
    txs_root: bytes = b""
    receipt_root: bytes = b""
    state_root: bytes = b""
    number: int = 0
    gas_used: bytes = b""
    timestamp: int = 0
    sealer: int = 0
    sealer_list: List[bytes] = field(default_factory=list)
    extra_data: bytes = b""
    consensus_weights: List[int] = field(default_factory=list)
    data_hash: bytes = b""
    signatures: List[HeaderSignature] = field(default_factory=list)
    tx_count: int = 1


@dataclass
class ConsensusSet:
    """The consensus node list the headers are checked against: 64-byte node ids (public keys), weights,
    minRequiredQuorum() and committedProposal()->index()."""
    node_ids: List[bytes] = field(default_factory=list)
    weights: List[int] = field(default_factory=list)
    min_required_quorum: int = 0
    committed_index: int = -1


class _ParentInfoView(ctypes.Structure):
    _fields_ = [("block_number", ctypes.c_int64), ("block_hash", ctypes.c_char_p), ("block_hash_len", ctypes.c_size_t)]


class _HeaderSignatureView(ctypes.Structure):
    _fields_ = [("sealer_index", ctypes.c_int64), ("signature", ctypes.c_char_p), ("signature_len", ctypes.c_size_t)]


class _BlockHeaderView(ctypes.Structure):
    """bcosgpu_BlockHeaderData (include/bcos_gpu.h): pointers into the caller's fields."""
    _fields_ = [("version", ctypes.c_int32),
                ("parents", ctypes.POINTER(_ParentInfoView)), ("nparents", ctypes.c_size_t),
                ("txs_root", ctypes.c_char_p), ("txs_root_len", ctypes.c_size_t),
                ("receipt_root", ctypes.c_char_p), ("receipt_root_len", ctypes.c_size_t),
                ("state_root", ctypes.c_char_p), ("state_root_len", ctypes.c_size_t),
                ("block_number", ctypes.c_int64),
                ("gas_used", ctypes.c_char_p), ("gas_used_len", ctypes.c_size_t),
                ("timestamp", ctypes.c_int64),
                ("sealer", ctypes.c_int64),
                ("sealer_list", ctypes.POINTER(_BytesView)), ("nsealer_list", ctypes.c_size_t),
                ("extra_data", ctypes.c_char_p), ("extra_data_len", ctypes.c_size_t),
                ("consensus_weights", ctypes.POINTER(ctypes.c_int64)), ("nconsensus_weights", ctypes.c_size_t),
                ("data_hash", ctypes.c_char_p), ("data_hash_len", ctypes.c_size_t),
                ("signatures", ctypes.POINTER(_HeaderSignatureView)), ("nsignatures", ctypes.c_size_t),
                ("tx_count", ctypes.c_uint64)]


class _ConsensusSetView(ctypes.Structure):
    _fields_ = [("node_ids64", ctypes.c_void_p), ("weights", ctypes.c_void_p), ("n", ctypes.c_size_t),
                ("min_required_quorum", ctypes.c_uint64), ("committed_index", ctypes.c_int64)]


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def header_views(headers):
    """ctypes views of BlockHeader objects; returns (views array, keep-alive list)."""
    n = len(headers)
    views = (_BlockHeaderView * max(n, 1))()
    keep = []
    for i, h in enumerate(headers):
        v = views[i]
        v.version, v.block_number, v.timestamp, v.sealer = h.version, h.number, h.timestamp, h.sealer
        v.tx_count = h.tx_count
        for name, val in (("txs_root", h.txs_root), ("receipt_root", h.receipt_root), ("state_root", h.state_root),
                          ("gas_used", h.gas_used), ("extra_data", h.extra_data), ("data_hash", h.data_hash)):
            b = _b(val)
            keep.append(b)
            setattr(v, name, b)
            setattr(v, name + "_len", len(b))
        if h.parents:
            ps = (_ParentInfoView * len(h.parents))()
            for p, (num, ph) in zip(ps, h.parents):
                b = _b(ph)
                keep.append(b)
                p.block_number, p.block_hash, p.block_hash_len = num, b, len(b)
            keep.append(ps)
            v.parents, v.nparents = ps, len(h.parents)
        if h.sealer_list:
            sl = (_BytesView * len(h.sealer_list))()
            for s, nid in zip(sl, h.sealer_list):
                b = _b(nid)
                keep.append(b)
                s.data, s.len = b, len(b)
            keep.append(sl)
            v.sealer_list, v.nsealer_list = sl, len(h.sealer_list)
        if h.consensus_weights:
            ws = (ctypes.c_int64 * len(h.consensus_weights))(*h.consensus_weights)
            keep.append(ws)
            v.consensus_weights, v.nconsensus_weights = ws, len(h.consensus_weights)
        if h.signatures:
            sg = (_HeaderSignatureView * len(h.signatures))()
            for s, hs in zip(sg, h.signatures):
                b = _b(hs.signature)
                keep.append(b)
                s.sealer_index, s.signature, s.signature_len = hs.index, b, len(b)
            keep.append(sg)
            v.signatures, v.nsignatures = sg, len(h.signatures)
    return views, keep


def consensus_view(consensus):
    """ctypes view of a ConsensusSet; returns (view, keep-alive list)."""
    n = len(consensus.node_ids)
    assert len(consensus.weights) == n and all(len(k) == 64 for k in consensus.node_ids)
    ids = np.frombuffer(b"".join(consensus.node_ids), dtype=np.uint8).copy() if n else np.zeros(64, np.uint8)
    ws = np.array(list(consensus.weights) or [0], dtype=np.uint64)
    v = _ConsensusSetView(ids.ctypes.data, ws.ctypes.data, n, consensus.min_required_quorum,
                          consensus.committed_index)
    return v, [ids, ws]


def pack_headers(headers, recompute=False):
    """The native packer (bcosgpu_pack_header_preimages, host C++): list[BlockHeader] -> (uint8 data,
    uint64 offsets[n+1]), the header-hash preimages back to back; a header whose dataHash is used (non-empty,
    and not `recompute`) gets an empty preimage."""
    views, keep = header_views(headers)
    n = len(headers)
    flags = HEADER_RECOMPUTE if recompute else 0
    size = int(lib().bcosgpu_header_preimage_size(views, n, flags))
    out = np.zeros(max(size, 1), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    check(lib().bcosgpu_pack_header_preimages(views, n, flags, _ptr(out), size, _ptr(off)))
    del keep
    return out[:size], off


def check_headers(suite, headers, consensus, prev: Optional[Tuple[int, bytes]] = None, recompute=False):
    """bcosgpu_headers_check: hash, BlockValidator::asyncCheckBlock and the parent link of a run of headers on
    the GPU.  prev: (number, hash) of the header before the first one, or None.  Returns (hashes uint8[n, 32],
    check uint8[n], link uint8[n], sig_ok uint8[total signatures]) -- see include/bcos_gpu.h for the codes."""
    ensure_device()
    views, keep = header_views(headers)
    cv, ckeep = consensus_view(consensus)
    n = len(headers)
    nsig = sum(len(h.signatures) for h in headers)
    hashes = np.zeros((n, 32), dtype=np.uint8)
    chk = np.zeros(n, dtype=np.uint8)
    link = np.zeros(n, dtype=np.uint8)
    sig_ok = np.zeros(max(nsig, 1), dtype=np.uint8)
    prev_hash = None
    if prev is not None:
        assert len(prev[1]) == 32
        prev_hash = ctypes.c_char_p(bytes(prev[1]))
    check(lib().bcosgpu_headers_check(suite, views, n, ctypes.byref(cv), prev_hash, prev[0] if prev else 0,
                                      HEADER_RECOMPUTE if recompute else 0, _ptr(hashes), _ptr(chk), _ptr(link),
                                      _ptr(sig_ok)))
    del keep, ckeep
    return hashes, chk, link, sig_ok[:nsig]


def header_hashes(hasher, headers, recompute=False):
    """The header hashes alone (BlockHeader::hash): the packed preimages through bcosgpu_hash_batch, a used
    dataHash (zero-filled to 32 bytes) in place of the digest.  Returns uint8[n, 32]."""
    ensure_device()
    data, off = pack_headers(headers, recompute)
    n = len(headers)
    out = np.zeros((max(n, 1), 32), dtype=np.uint8)
    if n:
        src = data if data.size else np.zeros(1, dtype=np.uint8)
        check(lib().bcosgpu_hash_batch(hasher, _ptr(src), _ptr(off), n, _ptr(out)))
    out = out[:n]
    if not recompute:
        for i, h in enumerate(headers):
            if h.data_hash:
                out[i] = np.frombuffer(_b(h.data_hash).ljust(32, b"\0"), dtype=np.uint8)
    return out
