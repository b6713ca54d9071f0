"""The lane-trio kernel's split square root on the CPU: tests/cpp/trio_sqrt_split_test.cpp checks that
fe26_sqrt_head then fe26_sqrt_tail is fe26_sqrt_cand limb for limb (both cuts), and that the split last
addition -- Z3 without y on one side (trio_add_z), X3 and Y3 on the other (trio_add) -- gives the affine
point of CurveK1x::add, exceptional cases included, with FE26_CHECK's magnitude assertions on every lane of
a DPP row run as lockstep threads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sqrt_split_matches_one_lane(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "trio_sqrt_split_test")
    subprocess.run([cxx, "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror",
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "trio_sqrt_split_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("sqrt split ok"), out.stdout
