"""The host leg of fisco-bcos_amd/tools/f26vec.hip: the GPU test's driver compiled as plain C++ with
FE26_CHECK, so the kernel body runs as a loop over the very case file tests/test_gpu_f26.py sends to the
device, on the C++ fallbacks of fe26.h / fp26.h, with every magnitude contract and limb bound asserted on the
way.  The same checker (tests/f26_vectors.py, Python integers mod p) judges the output: generator and
checker are proven here before anything runs on a GPU, and a case that would break a contract aborts."""
import os
import shutil
import subprocess

import pytest

import f26_vectors as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "fisco-bcos_amd", "tools", "f26vec.hip")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    # the host leg is the gate in front of the GPU run: without a host compiler it fails, it does not skip
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++, clang++, c++) to build the f26vec host leg"
    out = str(tmp_path_factory.mktemp("f26vec") / "f26vec_host")
    subprocess.run([cxx, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror",
                    "-DFE26_CHECK", "-o", out, SRC], check=True)
    return out


def test_host_leg_matches_integers(exe):
    cs = fv.cases()
    r = subprocess.run([exe], input=fv.text(cs), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = fv.check_all(cs, r.stdout.split(), host=True)
    assert seen["random"] == fv.N_RANDOM * sum(len(fv.op_list(f)) for f in fv.FIELDS.values())
    assert all(seen[k] > 0 for k in ("bound", "single", "kp", "canon", "limb3")), seen


def test_tool_rejects_what_it_cannot_run(exe):
    """An op or instantiation outside the dispatch is an error, never a silent copy of the operand."""
    z = ",".join(["0"] * 10)
    for line in ("k1 sub5 %s %s" % (z, z), "k1 to_mont %s %s" % (z, z), "p2 sqrt_cand %s %s" % (z, z),
                 "q9 mul %s %s" % (z, z), "k1 mul 1,2,3 %s" % z):
        r = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and r.stdout == "", line
