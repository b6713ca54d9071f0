"""The row-spread fields of fe_row.h and the row helpers of ec_row.h on the device, against Python integers:
fisco-bcos_amd/lib/rowvec (built by `make -C fisco-bcos_amd`) runs one op per 16-lane row, four rows to a wave.
The code is device-only (DPP row moves, permlane swaps), so this is its unit test: frow::mul / sqr / mul_sm2
with every limb at m B (limb 9 included) for m up to 16, single limbs at 16 B, multiples of p, the canonical
edge values and 500 seeded random operands; sub<K> / neg<K> / sub_sm2<K> / neg_sm2<K> / mul_int<C> as ec_row.h
instantiates them; to_fe26, is_zero, is_zero_sm2, from_fe26, from_words; gather4, gather01, gather0, sel4.
Checked: the value mod p, lanes 10..15 zero, every limb under the header's bound (which covers reduce_sm2's
"nothing leaves lane 9"), and that a row's answer is the same limbs whatever the neighbouring rows hold.
Cases, contracts and checker are tests/row_vectors.py."""
import os
import subprocess

import pytest

import row_vectors as rv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fisco-bcos_amd", "lib", "rowvec")


@pytest.mark.gpu
def test_row_fields_vs_python():
    assert os.path.exists(EXE), "build fisco-bcos_amd/lib/rowvec first (make -C fisco-bcos_amd)"
    rs = rv.rows()
    r = subprocess.run([EXE], input=rv.text(rs), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = rv.check_all(rs, r.stdout.split())
    assert all(seen[k] > 0 for k in ("bound", "single", "kp", "canon", "random", "case", "neighbour")), seen
