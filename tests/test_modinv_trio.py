"""The safegcd inversion on lane trios (csrc/modinv30.h: divsteps_30_trio, update_trio_30, modinv_safegcd_trio)
without a GPU.

tests/cpp/modinv_trio_test.cpp runs the 16 lanes of one DPP row -- five trios and the phantom lane -- as host
threads in lockstep and compares, for both secp256k1 moduli: every batch's matrix and zeta with the one-lane
divsteps_30 of the same header (random words, the edge words of g and zeta, whole inversions' trajectories; the
systolic and the lag-free form); whole inversions with the one-lane loop and with x x^-1 = 1 by a plain 512-bit
product (edge values, 2,000 random residues, rows of one value, rows mixing 0 with live values); the number of
batches each row runs, which is what the wave-uniform exit decides; and every row a second time with other words
on the phantom lane.  It is built twice, each run as a child process: plain, and with
-fsanitize=address,undefined.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": [],
          "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", list(BUILDS))
def test_trio_inversion_equals_one_lane_inversion(tmp_path, build):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    exe = str(tmp_path / ("modinv_trio_test_" + build))
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"]
                   + BUILDS[build] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "modinv_trio_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", "exit %d\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-8000:])
    assert out.stdout.startswith("modinv trio ok"), out.stdout
