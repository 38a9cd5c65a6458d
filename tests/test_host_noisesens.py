"""The HIP-free half of the noise sensitivities (ch_noisesens_host.hpp) as a stand-alone program under AddressSanitizer / UBSan:
panel widths, LDS and workspace sizes at 1, 2, 16, 95, 96, 97 and 4096 unknowns (the launch that only stores y included), the
frequency-chunk rule at the workspace cap, and the MOSFET noise-parameter table with the extra row of a perturbed instance column."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_noisesens_layout_chunks_and_extra_row(tmp_path):
    exe = build_sanitized(tmp_path, "host_noisesens.cpp", "noisesens_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "noisesens host:" in r.stdout and " 0 bad" in r.stdout
