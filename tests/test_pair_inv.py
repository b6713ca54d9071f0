"""r^-1 and u2 = s / r for a pair of signatures from one inversion (csrc/pair_inv.h) without a GPU.

tests/cpp/pair_inv_test.cpp runs the header's own sequence -- the substitution of rejected members, the products
before the inversion, the un-pairing -- on the three lanes of a trio in lockstep and compares u2 and r^-1 of both
members, word for word, with one inversion per signature (the path tx_verify_trio26_kernel took before), and with
r^-1 r = 1, u2 r = s: 1,000,000 random pairs and the crafted ones (equal r, r = 1, r = n - 1, r_b = 1 / r_a,
members rejected by r = 0, n, n + 1, 2^256 - 1, by s = 0 or by the parser, in either seat and in both).  It is built
twice, each run as a child process: plain, and with -fsanitize=address,undefined.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": [],
          "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", list(BUILDS))
def test_pair_inversion_equals_one_inversion_per_signature(tmp_path, build):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    exe = str(tmp_path / ("pair_inv_test_" + build))
    subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"]
                   + BUILDS[build] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "pair_inv_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stderr == "", "exit %d\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-8000:])
    assert out.stdout.startswith("pair inv ok"), out.stdout
