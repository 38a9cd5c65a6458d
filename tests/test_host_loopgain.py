"""The HIP-free half of the loop-gain analysis (ch_loopgain_host.hpp) as a stand-alone program under AddressSanitizer / UBSan:
u -> T and du -> dT against long-double arithmetic (the pole 1 - u = 0 included), the checks of the probe and of the slots, the sign of
the current-injection right-hand side, and the LDS / workspace sizes of loopgain_solve_kernel at 1 .. 96, 97 and 4096 unknowns."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_loopgain_combination_probe_checks_and_layout(tmp_path):
    exe = build_sanitized(tmp_path, "host_loopgain.cpp", "loopgain_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "loopgain host:" in r.stdout and " 0 bad" in r.stdout
