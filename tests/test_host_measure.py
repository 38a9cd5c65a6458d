"""The arithmetic of the waveform measurements (ch_measure_host.hpp: what both kernels of ch_measure_kernels.hpp call) as a stand-alone
program under AddressSanitizer / UBSan: the event rules at their edges, the interpolation window clamped near the start, window ends
outside the run and empty windows, NaN rows, the chunk rules, closed-form values and sensitivities, and a serial replay of the wave
form against the one-pass form."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_measure_host_half(tmp_path):
    exe = build_sanitized(tmp_path, "host_measure.cpp", "measure_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "measure host:" in r.stdout and " 0 bad" in r.stdout
