"""The HIP-free half of the AC sensitivities (ch_acsens_host.hpp) as a stand-alone program under AddressSanitizer / UBSan: panel
width, workspace and frequency-chunk sizes at 1, 2, 16, 95, 96, 97 and 4096 unknowns; the step of the state term (zero node part:
skipped; a direction with branch rows only; a huge or non-finite s_k); the complex expansion to MNA order on the hand-built
analysis of host_sens_steps.cpp (known node = 0, merged node, eliminated branch current = NaN, a sample that was not served)."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_acsens_layout_state_step_and_mna_expansion(tmp_path):
    exe = build_sanitized(tmp_path, "host_acsens.cpp", "acsens_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "acsens host:" in r.stdout and " 0 bad" in r.stdout
