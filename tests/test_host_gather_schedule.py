"""The lane schedule of the device-resident stepper's gather (cedarsim.jl_amd/csrc/ch_gather_plan.hpp) as a stand-alone host program
under AddressSanitizer / UBSan: the DFF class's source counts (T = 3), all-light classes (T = 1), one item heavier than everything
else together, more than 128 items, nc = 1, 8, 11, 12, 16 and 300 random classes up to nc = 64.  Per class: every item exactly once,
its sources in list order and contiguous in one lane, no lane above T, max(ceil(trips / 64), heaviest item) <= T <= ceil(trips / 64)
+ heaviest - 1 (what first fit guarantees), every destination offset the work-list epilogue's r * lda + col / e, and a replay of the
kernel's trip loop on random stamp values equal bit for bit to the plain per-item sums for A, C, F and Q."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_gather_schedule_packs_every_item_once_and_replays_bit_for_bit(tmp_path):
    exe = build_sanitized(tmp_path, "host_gather_schedule.cpp", "gather_schedule")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "gather schedule: 313 classes, 0 bad" in r.stdout, r.stdout[-2000:]
