"""The HIP-free half of the transient sensitivities (ch_transens_host.hpp) as a stand-alone program under AddressSanitizer / UBSan:
the ring, row and dump layout and the column-chunk rule at 1, 16, 96 and 97 unknowns, the test that refuses a slot which moves a
break point (PULSE levels and a SIN's frequency do not; td, tr, tf, pw do), the derivative of a known node's value at a time, and the
scalar one-step recursion against 2 x 2 cases worked out by hand."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_transient_sensitivity_host_half(tmp_path):
    exe = build_sanitized(tmp_path, "host_transens.cpp", "transens_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "transens host:" in r.stdout and " 0 bad" in r.stdout
