#!/usr/bin/env python3
"""What three frequency-domain measures per Monte-Carlo sample, with their derivatives, cost where the AC solve leaves its result, and
what that replaces.

The MOSFET amplifier of tests/test_gpu_ac_noise.py (the DFF workload has no AC source) with 1024 samples (rd and the width of m1
spread by a few per cent), 8 slots, 61 frequencies from 100 Hz to 100 MHz; the unity-gain frequency, the phase there and the gain at
10 kHz.  Reports, all whole-call wall times around the C entry point, best of three after a warm-up:
  ac_measure_ms     ch_ac_measure: the launches of ch_ac_sens, the gather, one measure kernel, [n_meas][(n_par)][S] back
  ac_sens_ms        ch_ac_sens with its full read-back and expansion to MNA order: what the measures were computed from before
  reference_ms      the float64 reference of tests/fmeasure_reference.py over those rows, one sample after the other
  rows_layer_ms     ch_freq_measure_rows on the same host rows (upload of the three rows and their sensitivities, one kernel)
and the worst scaled difference between ch_ac_measure and the reference.  Prints one JSON line.
    python scripts/ac_measure_timing.py [samples]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in bench.py)

from cedarsim_jl_amd import dc_opts, db, fevent, ffind_at, ffind_when, phase, unity_gain_freq  # noqa: E402
from cedarsim_jl_amd.acmeasure import mna_rows, resolve_fmeasures  # noqa: E402
from cedarsim_jl_amd.engine import EngineCircuit  # noqa: E402
import fmeasure_cases as fc  # noqa: E402
import fmeasure_reference as fr  # noqa: E402
from test_gpu_ac_noise import amp_circuit  # noqa: E402

SLOTS = ["rd", "vdd", ("rb1", "m"), ("m1", "w"), ("m1", "l"), ("nfet_06v0", "vth0"), "temp", "co"]
ALL = {}


def best_of(n, f, name):
    out = None
    for _ in range(n):
        t0 = time.perf_counter()
        out = f()
        ALL.setdefault(name, []).append(round((time.perf_counter() - t0) * 1e3, 3))
    return min(ALL[name]), out


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    c = amp_circuit()
    ids = [c.slot(*n) if isinstance(n, tuple) else c.slot(n) for n in SLOTS]
    f = 10.0 ** np.linspace(2.0, 8.0, 61)
    measures = [unity_gain_freq("fug", "o"), ffind_when("ph", phase("o"), fevent(db("o"), 0.0, "fall")), ffind_at("a0", db("o"), 1e4)]
    res = resolve_fmeasures(measures, mna_rows(c))
    eng = EngineCircuit(c, small_signal=True)
    eng.set_samples(S)
    rng = np.random.default_rng(7)
    eng.set_params([ids[0], ids[3]], [20e3 * (1.0 + 0.03 * rng.standard_normal(S)), 2e-6 * (1.0 + 0.03 * rng.standard_normal(S))])
    o = dc_opts(abstol=1e-12)

    def measured():
        rc, val, status, sens, sample_status, st = eng.ac_measure(ids, f, res.specs, len(res.names), o)
        assert rc == 0, eng.ctx.last_error()
        return val, status, sens, st

    def solved():
        rc, x, _, sens, status, st = eng.ac_sens(ids, f, o)
        assert rc == 0, eng.ctx.last_error()
        return x, sens, st

    measured(), solved()   # (first calls: code objects are loaded, buffers sized)
    ac_measure_ms, (val, status, dval, st_m) = best_of(3, measured, "ac_measure_ms")
    ac_sens_ms, (x, sens, st_s) = best_of(3, solved, "ac_sens_ms")
    row = c.mna_index("v", "o")
    H = np.ascontiguousarray(np.transpose(x[:, :, row])[None])                            # [1][n_freq][S]
    dH = np.ascontiguousarray(np.transpose(sens[:, :, :, row], (2, 1, 0))[None])          # [1][n_par][n_freq][S]
    S1 = fr.side
    ref_specs = [fr.spec("when", S1(0, sig="db", level=0.0, edge="fall")), fr.spec("find_when", S1(0, sig="db", level=0.0, edge="fall"), S1(0, sig="phase")),
                 fr.spec("find_at", S1(0, sig="db"), at=1e4)]
    t0 = time.perf_counter()
    ref = [[fr.measure_f64(f, H[:, :, s], dH[:, :, :, s], sp) for s in range(S)] for sp in ref_specs]
    reference_ms = (time.perf_counter() - t0) * 1e3
    rows_ms, (val_r, status_r, dval_r) = best_of(3, lambda: eng.ctx.freq_measure_rows(f, H, fc.to_ctypes(ref_specs), 3, dH), "rows_layer_ms")
    worst = 0.0
    for k, sp in enumerate(ref_specs):
        for s in range(S):
            v, stt, d = ref[k][s]
            assert stt == status[k, s] == status_r[k, s], (k, s, stt, status[k, s])
            if stt == 0:
                vs, ss = fc.scales(sp, f, H[:, :, s], dH[:, :, :, s])
                worst = max(worst, *fc.figure_errors(sp, float(val[k, s]), [float(q) for q in dval[k, :, s]], v, d, vs, ss))
    ok = status[0] == 0
    print(json.dumps({"samples": S, "slots": len(ids), "frequencies": len(f), "measures": len(measures), "ac_measure_ms": round(ac_measure_ms, 3),
                      "ac_sens_ms": round(ac_sens_ms, 3), "reference_ms": round(reference_ms, 1), "rows_layer_ms": round(rows_ms, 3), "all_timings_ms": ALL,
                      "kernel_launches": [st_m["n_kernel_launches"], st_s["n_kernel_launches"]], "measured_ok": int(ok.sum()),
                      "worst_scaled_difference": worst,
                      "fug_hz_min_max": [float(val[0][ok].min()), float(val[0][ok].max())] if ok.any() else None,
                      "phase_deg_sample0": float(val[1, 0]), "a0_db_sample0": float(val[2, 0])}))
    assert worst < 1e-9


if __name__ == "__main__":
    main()
