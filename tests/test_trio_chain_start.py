"""The lane-trio kernel's chain start on the CPU: tests/cpp/trio_chain_start_test.cpp checks that
trio_chain_start -- the two top Booth digits of a GLV half as one table load, one doubling and one
addition -- gives the point of the start it replaces (top digit onto infinity, then a whole window) and of
t additions on one lane, for every t in 0..16, both chains and both signs, that the digits after it still
sum to the scalar, and that whole chains equal a one-lane double-and-add, with FE26_CHECK's magnitude
assertions on every lane of a DPP row run as lockstep threads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_start_matches_old_start(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path / "trio_chain_start_test")
    subprocess.run([cxx, "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror",
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "trio_chain_start_test.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("chain start ok"), out.stdout
