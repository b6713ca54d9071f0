"""The recovery kernel's table of R' on three waves (csrc/ec26_trio.h, trio_table_shared) without a GPU.

tests/cpp/trio_table_test.cpp runs the three roles as three host threads over a host copy of the kernel's LDS
struct, the flags a std::atomic with the device's orders, and a fourth thread that reads the table behind the
three "done" flags as a chain wave does; every word of tab, tabphx, zc and the stored K must equal the one-wave
build's (trio_table_staged), under FE26_CHECK's magnitude assertions, for x on the curve, x with no curve point
and what a rejected signature leaves, with 1, 39 and 40 active lanes.  A flag order that cannot finish ends at
the program's watchdog (exit 3 after 10 s).  It is built three ways, each run as a child process: plain, with
-fsanitize=address,undefined, and with -fsanitize=thread, which reports an entry stored ahead of the flag that
guards its multiple or a "done" posted before the last entry.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": [],
          "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          "tsan": ["-fsanitize=thread"]}


@pytest.mark.parametrize("build", list(BUILDS))
def test_three_wave_table_equals_one_wave_table(tmp_path, build):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    exe = str(tmp_path / ("trio_table_test_" + build))
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"]
                   + BUILDS[build] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "trio_table_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", "exit %d\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-8000:])
    assert out.stdout.startswith("trio table ok"), out.stdout
