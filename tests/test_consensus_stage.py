"""The host half of bcosgpu_headers_check and bcosgpu_pbft_check (csrc/consensus_stage.h) without a GPU.

tests/cpp/consensus_stage_test.cpp runs the stages' own validate, plan, pack, args and scatter over hand-made
views and compares with offsets and bytes worked by hand from the stated order of regions: every region 8-byte
aligned, disjoint and in order (rows odd with slot ids, rows with keys, n not a multiple of 8); a header with an
early verdict has no rows and its sig_ok entries are 2; a row with an unknown index or a short signature fails
without a key; the parent [0] rule; a given dataHash against BCOSGPU_HEADER_RECOMPUTE; an absent proposal
signature has no row and reads 0; prepared proposals with the check on and off; an unknown generated_from; an
empty consensus set; every bad view with the message the entry points return; the kernels' arguments on two base
pointers.  Every block is a heap array of exactly plan.total bytes.  It is built with csrc/pack.cpp (the packer
of the header preimages) twice, each run as a child process: plain, and with -fsanitize=address,undefined.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": [],
          "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", list(BUILDS))
def test_staging_plans_of_the_header_and_pbft_checks(tmp_path, build):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    exe = str(tmp_path / ("consensus_stage_test_" + build))
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + BUILDS[build]
                   + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "consensus_stage_test.cpp"),
                      os.path.join(ROOT, "fisco-bcos_amd", "csrc", "pack.cpp"), "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", "exit %d\n%s\n%s" % (out.returncode, out.stdout[-4000:], out.stderr[-8000:])
    assert out.stdout.startswith("consensus stage ok"), out.stdout
