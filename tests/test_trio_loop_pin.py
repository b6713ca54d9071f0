"""The head of the lane-trio kernels' window loop (trio_glv_chain, csrc/ecc_coop.hip) stays where it was measured.

The loop is 28 KB of straight code and its time depends on where its head falls within a 64-byte line of the
instruction cache (profiles/trio_loop_pin.json: the sixteen offsets on the MI355X).  The source pins it with an
alignment and a pad of s_nop in front of the loop, but the compiler may still put preheader instructions between
the pad and the head, so the offset is read from the built code: the Makefile's own rule brings build/ecc_coop.o
up to date with the sources (nothing to do after a build), tools/loop_head.py disassembles it and finds the window
loop in every instantiation of tx_verify_trio26_kernel (TxIO, SigIO, EcrecIO) and in sig_verify_trio26_kernel, and
this test compares the head's address modulo 64 with kTrioLoopHeadMod64 of the source.  It reads addresses and
branch targets only.  A later edit that moves the loop fails here instead of costing 1-2 % unseen.  CPU-only."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fisco-bcos_amd")
sys.path.insert(0, os.path.join(PKG, "tools"))


def _constant(name):
    src = open(os.path.join(PKG, "csrc", "ecc_coop.hip")).read()
    m = re.search(r"static constexpr int %s = (\d+);" % name, src)
    assert m, name
    return int(m.group(1))


def _code():
    """build/ecc_coop.o, brought up to date with the sources by the Makefile's own rule."""
    obj = os.path.join(PKG, "build", "ecc_coop.o")
    r = subprocess.run(["make", "-C", PKG, obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return obj


@pytest.fixture(scope="module")
def loops():
    import hazard_check
    import loop_head
    for t in ("llvm-objcopy", "llvm-objdump"):
        assert os.path.exists(os.path.join(hazard_check.LLVM, t)), "%s: the ROCm LLVM tools that built the object" % t
    return loop_head.window_loops(_code())


def test_every_trio_kernel_has_its_window_loop(loops):
    names = sorted(loops)
    assert len(names) == 4, names
    for io in ("TxIO", "SigIO", "EcrecIO"):
        assert sum("tx_verify_trio26_kernel" in n and io in n for n in names) == 1, (io, names)
    assert sum("sig_verify_trio26_kernel" in n for n in names) == 1, names
    for n, (head, size) in loops.items():
        assert 26 * 1024 < size < 40 * 1024, (n, hex(head), size)  # the window's body (28 KB), not an inversion (25 KB)


def test_window_loop_head_is_pinned(loops):
    want = _constant("kTrioLoopHeadMod64")
    got = {n: head % 64 for n, (head, _) in loops.items()}
    print(got)
    for n, off in got.items():
        assert off == want, "%s: window loop head at %d modulo 64, measured and pinned at %d" % (n, off, want)
