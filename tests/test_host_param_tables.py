"""The HIP-free table builders (ch_param_tables.hpp) as a stand-alone program under AddressSanitizer / UBSan.  On a circuit of two
blocks (four MOSFETs on the default BSIM4 card, two of them of one geometry, a resistor, a capacitor, a DC voltage source, a pulse
current source, two Verilog-A parameter entries) and for S = 1 and 3: for every slot kind, with the slot unset, set, and with a
second slot set on the same field, the tables perturb_tables returns — resolved per flattened device and per sample through
[d * Spar + s], dcls and, independently, bmeta / mc_list / dcls_local — are bit-for-bit those of build_param_tables run again with
the new values, and tables the slot does not reach are absent.  Further: class sharing (identical instances, equal per-sample
overrides), the private column of an instance slot on a shared class, mc[j] mirroring the list for j < 8, the two padding doubles
of mosp, CH_ERR_UNSUPPORTED for an instance slot in a block of 64 classes, the geometry and sub-model errors with their messages,
a slot on a MOSFET the analysis does not hold, and SlotValues::value."""
import subprocess

from test_host_analysis_fuzz import build_sanitized


def test_perturbed_tables_equal_a_rebuild_bit_for_bit(tmp_path):
    exe = build_sanitized(tmp_path, "host_param_tables.cpp", "param_tables")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "param tables:" in r.stdout and " 0 bad" in r.stdout
