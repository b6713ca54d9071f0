"""The host runtime layer the C ABI's files share (csrc/host_rt.h: grow-only buffers, device scope, stream
drain), checked by the stand-alone program fisco-bcos_amd/lib/hostrt_check (built by `make -C fisco-bcos_amd`):
the growth rule and, where no HIP device is visible, the failure paths; on a GPU the same objects for real."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fisco-bcos_amd", "lib", "hostrt_check")


def _run(*args):
    assert os.path.exists(EXE), "build fisco-bcos_amd/lib/hostrt_check first (make -C fisco-bcos_amd)"
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hostrt_check: ok" in r.stdout, r.stdout


def test_hostrt_growth_rule_and_failure_paths():
    _run()


@pytest.mark.gpu
def test_hostrt_on_device():
    _run("device")
