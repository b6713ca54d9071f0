"""The exact-integer GLV split (csrc/glv_split.h: glv_split_core, which glv_split of every secp256k1 kernel calls)
without a GPU.

tests/cpp/glv_split_test.cpp holds a literal restatement of the split's earlier form (512-bit rounding products,
k2 and k1 = k - k2 lambda by plain arithmetic mod n in 64-bit limbs, the comparison with (n - 1) / 2) and compares
magnitudes and signs with it for: the edge scalars 0, 1, 2, n-1, n-2, (n-1)/2, (n+1)/2, lambda, n-lambda,
lambda+-1, 2^128-1, 2^128, 2^255; +-t and +-t lambda mod n for t = 1..64 (one half is zero); 1,000,000 seeded
random k < n; and 1,000,000 more, searched for the largest |k1|, |k2| and the rounding fractions nearest 1/2
(printed).  Independently of that yardstick it asserts k1 + k2 lambda = k (mod n) with the signs applied and both
halves below 2^128.  Built twice, each run as a child process: plain, and with -fsanitize=address,undefined.
Nothing is loaded into Python.

The test can fail: on scratch copies of the header, dropping the rounding bit, a2 without its 129th bit, and the
truncated products cut to 128 bits each failed it at once (at k = n - 1, n - 1 and (n - 1) / 2)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": [],
          "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", list(BUILDS))
def test_exact_split_equals_the_modular_form(tmp_path, build):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    exe = str(tmp_path / ("glv_split_test_" + build))
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"]
                   + BUILDS[build] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "glv_split_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", "exit %d\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-8000:])
    assert out.stdout.startswith("glv split ok: 2000270 scalars"), out.stdout
    print(out.stdout)
    # the scalars the search found are the ones tests/test_gpu_glv_split.py sends through the kernels
    found = [int(x, 16) for x in re.findall(r"^  at k\s+([0-9a-f]{64})$", out.stdout, re.M)]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_glv_split
    assert found == test_gpu_glv_split.FOUND, [hex(x) for x in found]
