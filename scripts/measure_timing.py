#!/usr/bin/env python3
"""What one clock-to-q measurement per Monte-Carlo sample costs on the rows a device-stepper run keeps in HBM, and what it replaces.

`dff_mc_builder` with 8192 samples on the device stepper, saveat grid (0.5 ns), q observed; one DELAY (q rising through 0.5 V to q rising
through 4.5 V behind the clock edge at 400 ns, where every sample captures d = 1) and one WHEN.  Reports
  measure_ms        wall time of ch_result_measure on the kept rows (one call: upload of the specs, one kernel, three small copies back), best of three
  copy_ms           the device-to-host copy of the rows alone (torch, synchronised), best of three
  reference_ms      the float64 reference of tests/measure_reference.py over the copied rows, one sample after the other
and checks that the two agree.  Prints one JSON line.
    python scripts/measure_timing.py [samples]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (torch's HIP runtime first, as in bench.py)

from cedarsim_jl_amd import CircuitSweep, delay, event, tran_opts, when  # noqa: E402
from cedarsim_jl_amd.engine import _pf64, _pi32  # noqa: E402
from cedarsim_jl_amd.measure import resolve_measures  # noqa: E402
from cedarsim_jl_amd.workloads import dff_mc_builder, mc_tandem_sweep  # noqa: E402
import measure_reference as mr  # noqa: E402


ALL = {}   # every timing of a best-of, by name: the spread goes into the JSON line beside the best


def best_of(n, f, name):
    out = None
    for _ in range(n):
        t0 = time.perf_counter()
        out = f()
        ALL.setdefault(name, []).append(round((time.perf_counter() - t0) * 1e3, 3))
    return min(ALL[name]), out


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    torch.cuda.set_device(0)
    build, _ = dff_mc_builder()
    b = CircuitSweep(build, mc_tandem_sweep(S))._engine(0, S, None, views=False)
    eng, L = b.eng, b.eng.L
    measures = [delay("rise", event("q", 0.5, "rise", td=400e-9), event("q", 4.5, "rise", td=400e-9)), when("tq", "q", 2.5, "rise", td=400e-9)]
    names, specs = resolve_measures(b.ckt, measures)
    tspan, grid = (0.0, 4.5e-7), np.linspace(0.0, 4.5e-7, 901)
    opts = tran_opts(abstol=1e-5, reltol=1e-5, saveat=grid, stepper="device")
    r = C.c_void_p()
    t0 = time.perf_counter()
    rc = L.ch_tran(eng.h, tspan[0], tspan[1], C.byref(opts), C.byref(r))
    tran_ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0 and r, eng.ctx.last_error()
    try:
        t, v, _, st = eng._result(r)
        val, status = np.zeros((len(names), S)), np.zeros((len(names), S), np.int32)

        def measure():
            assert L.ch_result_measure(r, len(names), specs, val.ctypes.data_as(_pf64), None, status.ctypes.data_as(_pi32)) == 0, eng.ctx.last_error()
            return val.copy(), status.copy()

        measure()   # (first call: the kernel's code object is loaded)
        measure_ms, (val, status) = best_of(3, measure, "measure_ms")
        kept = st["device_rows"] is not None
        copy_ms = None
        if kept:
            dev = torch.as_tensor(st["device_rows"], device="cuda")

            def copy():
                out = dev.cpu()
                torch.cuda.synchronize()
                return out.numpy()
            copy_ms, rows = best_of(3, copy, "copy_ms")
            assert np.array_equal(rows, v)
    finally:
        L.ch_result_free(r)
    side = lambda e: mr.side(0, level=e.level, edge=e.edge, count=e.n, td=e.td)   # noqa: E731  (q is observable 0)
    ref_specs = [mr.spec("delay", side(measures[0].trig), side(measures[0].targ)), mr.spec("when", side(measures[1].trig))]
    t0 = time.perf_counter()
    ref = np.array([[mr.measure_f64(sp, t, None, v[:, :, s])[0] for s in range(S)] for sp in ref_specs])
    reference_ms = (time.perf_counter() - t0) * 1e3
    ok = status == 0
    worst = float(np.max(np.abs(val[ok] - ref[ok]))) / (tspan[1] - tspan[0]) if ok.any() else 0.0
    print(json.dumps({"samples": S, "rows": len(t), "rows_kept_in_hbm": bool(kept), "stepper": st["stepper"], "tran_ms": round(tran_ms, 3),
                      "measure_ms": round(measure_ms, 3), "copy_ms": None if copy_ms is None else round(copy_ms, 3), "reference_ms": round(reference_ms, 1), "all_timings_ms": ALL,
                      "measured_ok": int(ok.sum()), "worst_difference_over_span": worst,
                      "delay_ns_min_max": [round(float(val[0][ok[0]].min()) * 1e9, 4), round(float(val[0][ok[0]].max()) * 1e9, 4)] if ok[0].any() else None}))
    assert worst < 1e-12


if __name__ == "__main__":
    main()
