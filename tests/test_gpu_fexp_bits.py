"""`fexp` of cedarsim.jl_amd/csrc/ch_bsim4.hpp is the library's exp(double) on gfx950 bit for bit, with its polynomial coefficients
from either source (literals; the table in LDS the device-resident stepper reads them from).  tests/gpu_fexp_bits.hip runs both and
the library function in one kernel over 2^20 points evenly spread over [-40, 40], 2^16 over each of [-746, -700] and [700, 710], and
+-0, +-34 (EXP_TH) with their two neighbours, +-inf and NaN, and prints how many 64-bit patterns differ (NaN compared as NaN)."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_fexp_is_the_library_exp_bit_for_bit(tmp_path):
    exe = str(tmp_path / "gpu_fexp_bits")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "gpu_fexp_bits.hip"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout.strip())
    m = re.search(r"points (\d+) differ_literal (\d+) differ_lds (\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) == (1 << 20) + 2 * (1 << 16) + 12 + 3
    assert (int(m.group(2)), int(m.group(3))) == (0, 0)
