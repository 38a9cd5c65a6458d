"""The HIP-free parts of the transient and DC drivers (ch_stepper_host.hpp: resolve_tran_plan, persist_max_rows, collect_breakpoints,
add_newton_iters; ch_dc_start.hpp: the restart passes' guess and harvest) as a stand-alone program under AddressSanitizer / UBSan:
each gives bit for bit what the rule it replaced gave, written out in the program as the drivers had it."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_plan_rows_breakpoints_and_restart_passes_equal_the_old_rules_bit_for_bit(tmp_path):
    exe = build_sanitized(tmp_path, "host_tran_plan.cpp", "tran_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "tran plan:" in r.stdout and " 0 bad" in r.stdout
