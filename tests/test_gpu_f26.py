"""fe26 and fp26 as the device runs them, against Python integers: fisco-bcos_amd/lib/f26vec (built by `make -C
fisco-bcos_amd`) evaluates one operation per lane on operands given as raw limbs.  On the device fe26_mul /
fe26_sqr / fp26_mul / fp26_sqr are the generated inline-asm blocks of fe_asm.h, which the host builds of the
CPU suite never execute; here they meet operands at their contract bounds (every limb at m 2^26 for m up to 16
resp. 15, where a signed fp26 column comes within 2^56.5 of 2^63), single limbs at the bound, lazy multiples
of p, the canonical edge values and seeded random operands, for every sub<K> / neg<K> / mul_int<C> the
kernels instantiate, the square-root chain whole and cut in two, and fp26's conversions and inversion.
Cases, contracts and checker are tests/f26_vectors.py, which tests/test_f26vec_host.py runs on the CPU first."""
import os
import subprocess

import pytest

import f26_vectors as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fisco-bcos_amd", "lib", "f26vec")


@pytest.mark.gpu
def test_f26_device_ops_vs_python():
    assert os.path.exists(EXE), "build fisco-bcos_amd/lib/f26vec first (make -C fisco-bcos_amd)"
    cs = fv.cases()
    r = subprocess.run([EXE], input=fv.text(cs), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = fv.check_all(cs, r.stdout.split())
    assert seen["random"] == fv.N_RANDOM * sum(len(fv.op_list(f)) for f in fv.FIELDS.values())
    assert all(seen[k] > 0 for k in ("bound", "single", "kp", "canon", "limb3")), seen
