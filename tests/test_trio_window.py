"""The lane-trio kernel's lean window on the CPU: tests/cpp/trio_window_test.cpp checks that trio_window --
four sign-flipping doublings and the unscaled mixed addition on a TrioAcc -- gives the point of the window it
replaces (three trio_dbl, trio_dbl_zz, trio_madd_zz) and of four doublings and an addition on one lane, by
projective equality, for every digit in -8..8, both chains and both signs, limbs at the entry contract's
bounds, the accumulator infinite on all, some and none of a row's trios, 32 windows deep; that the chain
start followed by lean windows is right for every t in 0..16; and that whole 128-bit chains equal a one-lane
double-and-add, with FE26_CHECK's magnitude assertions on every lane of a DPP row run as lockstep threads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lean_window_matches_old_window_and_one_lane(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "trio_window_test")
    subprocess.run([cxx, "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror",
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "trio_window_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("trio window ok"), out.stdout
