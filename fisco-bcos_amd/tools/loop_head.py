#!/usr/bin/env python3
"""Where the lane-trio kernels' window loop (trio_glv_chain, csrc/ecc_coop.hip) lies in the built gfx950 code
(tools/hazard_check.py's disassembler), per instantiation of tx_verify_trio26_kernel and for
sig_verify_trio26_kernel: its head's address, that address modulo 64 (the instruction cache's line), its length
in bytes.  Addresses and branch targets only.  tests/test_trio_loop_pin.py asserts the offset; DESIGN.md 5 has
why it matters.

The loops of a kernel are its backward branches; those that span more than 20 KB are the window loop, the
safegcd inversions (about 25 KB each) and whatever encloses them.  The window loop is the longest of them that
holds no other's head (28 KB; several branches may close one loop: the farthest counts).

usage: loop_head.py LIB_OR_OBJECT   (one JSON object)"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hazard_check  # noqa: E402

KERNELS = ("tx_verify_trio26_kernel", "sig_verify_trio26_kernel")
MIN_SPAN = 20 * 1024


def long_loops(insts, base):
    """{head address: address of the farthest backward branch to it} of the loops that span more than MIN_SPAN."""
    index = {a for a, _, _ in insts}
    loops = {}
    for a, mn, ops in insts:
        if mn.startswith("s_cbranch") or mn == "s_branch":
            m = re.search(r"<.+\+0x([0-9a-f]+)>", ops)
            if m:
                tgt = base + int(m.group(1), 16)
                if tgt in index and a - tgt > MIN_SPAN:
                    loops[tgt] = max(loops.get(tgt, 0), a)
    return loops


def window_loops(path):
    """{kernel symbol: (head address, bytes)} of the window loop of every trio kernel in the file."""
    out = {}
    for name, base, insts in hazard_check.functions(path):
        if not any(k in name for k in KERNELS):
            continue
        loops = long_loops(insts, base)
        inner = {h: e for h, e in loops.items() if not any(h < h2 <= e for h2 in loops)}
        if inner:
            h = max(inner, key=lambda x: inner[x] - x)
            out[name] = (h, inner[h] + 4 - h)
    return out


def main():
    rec = {name: {"head": "0x%x" % h, "head_mod_64": h % 64, "bytes": b} for name, (h, b) in window_loops(sys.argv[1]).items()}
    print(json.dumps(rec, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
