"""The gather schedule built with the padded strides of the device stepper's LDS images (cedarsim.jl_amd/csrc/ch_gather_plan.hpp,
GatherStrides) as a stand-alone host program under AddressSanitizer / UBSan: which strides a circuit gets (narrow, compiled
Verilog-A, bordered, too large), and for every block size 1 .. NC under NC = 12 and NC = 16, four classes each: the padded plan has
the unpadded plan's lanes, trips and sources; every destination offset lies inside its image and decodes to the unpadded plan's
(row, column) or vector entry; F and hq sit one row of nc below and above Q behind C's nc rows; no pad entry is a destination; a
replay of the kernel's trip loop leaves the pad pattern untouched and gives every real entry the unpadded replay's bits."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_padded_strides_move_every_destination_and_touch_no_pad_entry(tmp_path):
    exe = build_sanitized(tmp_path, "host_gather_strides.cpp", "gather_strides")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "gather strides: 112 plans, 0 bad" in r.stdout, r.stdout[-2000:]
