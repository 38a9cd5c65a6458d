"""The arithmetic of the frequency-domain measurements (ch_fmeasure_host.hpp: what both kernels of ch_fmeasure_kernels.hpp call) as a
stand-alone program under AddressSanitizer / UBSan: the event rules at their edges, g_i == L, a relative level, phase wraps in both
directions and in consecutive intervals, windows outside the grid and empty windows, NaN rows, |H| = 0, the spec and grid checks,
closed-form values and sensitivities, and a serial replay of the wave form against the one-pass form."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_fmeasure_host_half(tmp_path):
    exe = build_sanitized(tmp_path, "host_fmeasure.cpp", "fmeasure_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "fmeasure host:" in r.stdout and " 0 bad" in r.stdout
