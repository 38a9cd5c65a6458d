"""The HIP-free half of the DC sensitivities (ch_sens_host.hpp) as a stand-alone program under AddressSanitizer / UBSan: the
finite-difference step rule per slot kind (absolute forward step where the residual is linear in the parameter, p = 0 and negative
p included; gmin with and without a compiled Verilog-A instance; central relative step elsewhere; abs_step overrides) and the
expansion to MNA order on a hand-built analysis (a known node fed by two sources with coefficients, a node merged by a 0 V
ammeter, an eliminated branch current = NaN, a failed operating point)."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_sensitivity_step_rule_and_mna_expansion(tmp_path):
    exe = build_sanitized(tmp_path, "host_sens_steps.cpp", "sens_steps")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "sens host:" in r.stdout and " 0 bad" in r.stdout
