"""The lane-trio point operations on a real wave against affine arithmetic over Python integers.
fisco-bcos_amd/lib/triovec (secp256k1, ec26_trio.h) and lib/triovec_sm2 (SM2, ecp26_trio.h; the same source
built with the SM2 translation unit's scheduler flag), both built by `make -C fisco-bcos_amd`, run 20 trios to
a wave:
  secp256k1  trio_dbl, trio_dbl_zz, trio_madd<true>, trio_madd_zz, trio_add, trio_window for every digit -8..8
             (trio_dbln<0..3> and trio_maddq_zz with keep true and false), trio_chain_start for every t in 0..16
             (so 11..16 run on the device), trio_scale_xz + trio_scale_y, trio_add_z;
  SM2        trio_dbl_sm2, trio_dbl_sm2_d, trio_madd_sm2_d, trio_add_sm2_jd, trio_madd_sm2<true>.
The CPU test runs these as 16 host threads, where the vote is over one row, the v_cndmask_b32_dpp select is
replaced and the DPP fence is empty; here one exceptional trio (P = Q, P = -Q, an infinite operand) sits in
row 0 trio 0, in row 3 trio 4 beside the phantom lane, in three rows at once, or in all twenty, and the
ordinary trios around it must give the very limbs they give in an all-ordinary wave.  Operands hug the entry
contracts' limb bounds; results are checked in affine coordinates, with the infinity flag, ZZ = Z^2 and
delta = Z^2, each kind's own magnitude bound, and operands handed through limb for limb.  Cases and checker
are tests/trio_vectors.py."""
import os
import subprocess

import pytest

import trio_vectors as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fisco-bcos_amd", "lib")


@pytest.mark.gpu
@pytest.mark.parametrize("exe,ops", [("triovec", tv.K1_OPS), ("triovec_sm2", tv.SM2_OPS)], ids=["secp256k1", "sm2"])
def test_trio_ops_vs_python(exe, ops):
    path = os.path.join(LIB, exe)
    assert os.path.exists(path), "build fisco-bcos_amd/lib/%s first (make -C fisco-bcos_amd)" % exe
    ts = tv.trios(ops)
    r = subprocess.run([path], input=tv.text(ts), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = tv.check_all(ts, r.stdout.splitlines())
    assert all(seen[(op, "ord")] >= tv.N_RANDOM for op in ops), seen
    assert seen["repeated"] >= 19 * sum(1 for op in ops if op in tv.KINDS), seen
