"""PBFT-side mirror: every signature of a drained PBFT message queue in one engine call.

  checkSignature                            bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:732-750
  checkProposalSignature                    bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:752-771
  PBFTCacheProcessor::checkPrecommitWeight  bcos-pbft/bcos-pbft/pbft/cache/PBFTCacheProcessor.cpp:795-821
  isValidNewViewMsg                         bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:1230-1271
"""
import ctypes
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

from ._lib import check, ensure_device, lib
from .crypto import _ptr
from .header import HeaderSignature, _HeaderSignatureView, _b, consensus_view

CHECK_MSG_SIG, CHECK_PROPOSAL_SIG, CHECK_PREPARED = 1, 2, 4
# msg_flags bits (a message is accepted iff 0) and prepared_check codes, as in include/bcos_gpu.h
E_NODE, E_MSG_SIG, E_PROPOSAL_SIG, E_PREPARED, E_VIEWCHANGE, E_GROUP_QUORUM = 1, 2, 4, 8, 16, 32
PREPARED_OK, PREPARED_E_PROOF, PREPARED_E_QUORUM, PREPARED_UNCHECKED = 0, 1, 2, 3
SIG_FAILED, SIG_OK, SIG_UNREQUESTED = 0, 1, 2


@dataclass
class PrecommitProof:
    """A prepared (precommitted) proposal as a view change carries it: PBFTProposal::hash() and its
    signatureProof list of (node index, signature)."""
    hash: bytes = b""
    proofs: List[HeaderSignature] = field(default_factory=list)


@dataclass
class PBFTMessage:
    """A PBFT message as its signature checks see it.  signed_data is what the signature is over (hashFieldsData
    or the codec payLoad); a non-empty signature_hash is used in its place, unhashed."""
    generated_from: int = 0
    signed_data: bytes = b""
    signature_hash: bytes = b""
    signature: bytes = b""
    proposal_hash: bytes = b""
    proposal_signature: bytes = b""
    prepared: List[PrecommitProof] = field(default_factory=list)
    checks: int = CHECK_MSG_SIG


class _PrecommitProofView(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_char_p), ("hash_len", ctypes.c_size_t),
                ("proofs", ctypes.POINTER(_HeaderSignatureView)), ("nproofs", ctypes.c_size_t)]


class _PBFTMessageView(ctypes.Structure):
    """bcosgpu_PBFTMessageData (include/bcos_gpu.h): pointers into the caller's fields."""
    _fields_ = [("generated_from", ctypes.c_int64),
                ("signed_data", ctypes.c_char_p), ("signed_data_len", ctypes.c_size_t),
                ("signature_hash", ctypes.c_char_p), ("signature_hash_len", ctypes.c_size_t),
                ("signature", ctypes.c_char_p), ("signature_len", ctypes.c_size_t),
                ("proposal_hash", ctypes.c_char_p), ("proposal_hash_len", ctypes.c_size_t),
                ("proposal_signature", ctypes.c_char_p), ("proposal_signature_len", ctypes.c_size_t),
                ("prepared", ctypes.POINTER(_PrecommitProofView)), ("nprepared", ctypes.c_size_t),
                ("checks", ctypes.c_uint32)]


class _PBFTGroupView(ctypes.Structure):
    _fields_ = [("parent", ctypes.c_size_t), ("first", ctypes.c_size_t), ("count", ctypes.c_size_t)]


def message_views(msgs):
    """ctypes views of PBFTMessage objects; returns (views array, keep-alive list)."""
    views = (_PBFTMessageView * max(len(msgs), 1))()
    keep = []
    for v, m in zip(views, msgs):
        v.generated_from, v.checks = m.generated_from, m.checks
        for name in ("signed_data", "signature_hash", "signature", "proposal_hash", "proposal_signature"):
            b = _b(getattr(m, name))
            keep.append(b)
            setattr(v, name, b)
            setattr(v, name + "_len", len(b))
        if m.prepared:
            ps = (_PrecommitProofView * len(m.prepared))()
            for p, pp in zip(ps, m.prepared):
                b = _b(pp.hash)
                keep.append(b)
                p.hash, p.hash_len = b, len(b)
                if pp.proofs:
                    sg = (_HeaderSignatureView * len(pp.proofs))()
                    for s, pr in zip(sg, pp.proofs):
                        sb = _b(pr.signature)
                        keep.append(sb)
                        s.sealer_index, s.signature, s.signature_len = pr.index, sb, len(sb)
                    keep.append(sg)
                    p.proofs, p.nproofs = sg, len(pp.proofs)
            keep.append(ps)
            v.prepared, v.nprepared = ps, len(m.prepared)
    return views, keep


def check_messages(suite, msgs, consensus, groups: Sequence[Tuple[int, int, int]] = ()):
    """bcosgpu_pbft_check: every requested signature of the messages on the GPU in one call.  groups: (parent,
    first, count) -- a NewView at `parent` whose view changes are msgs[first:first+count].  Returns (msg_hash
    uint8[n, 32], msg_flags uint32[n], prepared_check uint8[prepared proposals], sig_ok uint8[per message 2 +
    its proofs]) -- see include/bcos_gpu.h for the bits and codes."""
    ensure_device()
    views, keep = message_views(msgs)
    cv, ckeep = consensus_view(consensus)
    n = len(msgs)
    nprep = sum(len(m.prepared) for m in msgs)
    nsig = sum(2 + sum(len(p.proofs) for p in m.prepared) for m in msgs)
    gv = (_PBFTGroupView * max(len(groups), 1))(*[_PBFTGroupView(*g) for g in groups])
    hashes = np.zeros((n, 32), dtype=np.uint8)
    flags = np.zeros(max(n, 1), dtype=np.uint32)
    prep = np.zeros(max(nprep, 1), dtype=np.uint8)
    sig_ok = np.zeros(max(nsig, 1), dtype=np.uint8)
    check(lib().bcosgpu_pbft_check(suite, views, n, gv, len(groups), ctypes.byref(cv), 0, _ptr(hashes), _ptr(flags),
                                   _ptr(prep), _ptr(sig_ok)))
    del keep, ckeep
    return hashes, flags[:n], prep[:nprep], sig_ok[:nsig]
