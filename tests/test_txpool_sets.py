"""The kernel bodies of the transaction pool's sorted key sets and of admission (csrc/sorted_set.h,
csrc/txpool_admit.h) on the CPU, before any GPU sees them.

tests/cpp/txpool_sets_test.cpp calls every body for every thread index of its grid, serially, with each buffer
malloc'ed at exactly the capacity the body is told; it is built once with -fsanitize=address,undefined
-fno-sanitize-recover=all and run on its own (no Python in the process), so one index out of range, one signed
overflow or one misaligned access ends the run.  The expected values are std::set's and a literal loop of the
reference's order (the C++ twin of tests/txpool_restatement.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    out = str(tmp_path_factory.mktemp("txpool_sets") / "txpool_sets_test")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", out, os.path.join(ROOT, "tests", "cpp", "txpool_sets_test.cpp")],
                   check=True)
    return out


def _run(exe, what):
    r = subprocess.run([exe, what], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == what + ": ok"


def test_sets_against_std_set(exe):
    """Random operation sequences, the empty batch, one key, 130 copies of one key, a batch equal to / larger than
    the set, erase of absent keys, erase of everything then insert, a union landing exactly on capacity and one key
    over it (refused, error word set), keys 0 and 2^256 - 1, keys differing in the last byte."""
    _run(exe, "sets")


def test_admission_against_the_literal_order(exe):
    """verdict / rule / finalize, both modes, several calls per pool, on batches dense in repeated nonces and
    repeated whole transactions, against the one-after-another loop."""
    _run(exe, "admit")
