"""The HIP-free start vector of the DC operating point (ch_dc_start.hpp) as a stand-alone program under AddressSanitizer / UBSan:
for seeds 10 and 11 and S = 1 and 3 the cached unknown-space start and three restarts' worth of draws from the cached generator
states are bit for bit what the loop dc_solve ran on every call gave (written out in the program with its own generator)."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_cached_dc_start_and_restart_draws_equal_the_old_loop_bit_for_bit(tmp_path):
    exe = build_sanitized(tmp_path, "host_dc_start.cpp", "dc_start")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "dc start:" in r.stdout and " 0 bad" in r.stdout
