"""The host instantiation of csrc/va_rt.hpp (every VD rule, first order and nested, the scalar functions, the integer helpers, the
seeds and ddx) on the records of tests/device_math_cases.py, as a stand-alone program under AddressSanitizer / UBSan.  What it writes
is compared with the mpmath reference by tests/test_device_math_reference.py."""
import numpy as np

import device_math_cases as DC
from test_host_analysis_fuzz import build_sanitized


def test_host_device_math_is_sanitizer_clean(tmp_path):
    exe = build_sanitized(tmp_path, "host_device_math.cpp", "host_device_math")
    out = DC.run_program(exe, tmp_path, "host")
    for g in DC.GROUPS:   # every record of a rule the host has was answered
        if g.kind in (DC.K_VD1, DC.K_VD2, DC.K_INT, DC.K_SEED1) and g.judge != "table":
            assert not np.isnan(out[g.lo:g.hi, 0]).any(), g.name
