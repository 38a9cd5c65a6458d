"""The HIP-free half of the network-parameter analysis (ch_netparams_host.hpp) as a stand-alone program under AddressSanitizer /
UBSan: Yp -> S, Yp -> Z, dYp -> dS, dYp -> dZ against long-double arithmetic for 1, 2, 3 and 8 ports, the exactly singular Yp (NaN in Z
only), the checks of the ports and of the slots, and the LDS / workspace sizes of netparams_solve_kernel for 1 .. 8 ports at 1 .. 96,
97 and 4096 unknowns."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_netparams_conversions_port_checks_and_layout(tmp_path):
    exe = build_sanitized(tmp_path, "host_netparams.cpp", "netparams_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "netparams host:" in r.stdout and " 0 bad" in r.stdout
