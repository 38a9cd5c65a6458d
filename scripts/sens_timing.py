#!/usr/bin/env python3
"""Whole-call wall times of the sensitivity drivers, for comparing two builds of the library (CEDARHIP_LIB selects one per process).

The 1024-sample amplifier batch of scripts/ac_measure_timing.py (rd and the width of m1 spread by a few per cent, 8 slots, 61
frequencies from 100 Hz to 100 MHz): ch_dc_sens, ch_ac_sens, ch_noise_sens (at the drain), ch_ac_measure (three measures) and a short
ch_tran_sens (the same amplifier with a SIN on its input, 64 samples, 5 ns).  Every call is timed around the C entry point after one
warm-up call, with the profiler off; the median of `rounds` calls and all of them are reported.  Prints one JSON line.
    python scripts/sens_timing.py [rounds]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in bench.py)

from cedarsim_jl_amd import SIN, dc_opts, db, fevent, ffind_at, ffind_when, phase, tran_opts, unity_gain_freq  # noqa: E402
from cedarsim_jl_amd.acmeasure import mna_rows, resolve_fmeasures  # noqa: E402
from cedarsim_jl_amd.engine import LIB_PATH, EngineCircuit  # noqa: E402
from test_gpu_ac_noise import amp_circuit  # noqa: E402

SLOTS = ["rd", "vdd", ("rb1", "m"), ("m1", "w"), ("m1", "l"), ("nfet_06v0", "vth0"), "temp", "co"]
TRAN_SAMPLES, TRAN_SPAN = 64, (0.0, 5e-9)


def spread(eng, ids, S):
    rng = np.random.default_rng(7)
    eng.set_samples(S)
    eng.set_params([ids[0], ids[3]], [20e3 * (1.0 + 0.03 * rng.standard_normal(S)), 2e-6 * (1.0 + 0.03 * rng.standard_normal(S))])


def slots_of(c):
    return [c.slot(*n) if isinstance(n, tuple) else c.slot(n) for n in SLOTS]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    assert not os.environ.get("CEDARHIP_HOST_PROFILE"), "time with the profiler off"
    S = 1024
    c = amp_circuit()
    ids = slots_of(c)
    f = 10.0 ** np.linspace(2.0, 8.0, 61)
    measures = [unity_gain_freq("fug", "o"), ffind_when("ph", phase("o"), fevent(db("o"), 0.0, "fall")), ffind_at("a0", db("o"), 1e4)]
    res = resolve_fmeasures(measures, mna_rows(c))
    eng = EngineCircuit(c, small_signal=True)
    spread(eng, ids, S)
    o = dc_opts(abstol=1e-12)

    ct = amp_circuit()
    i = ct.dev_ipar[ct.dev_names.index("vin")][0]
    ct.sources[i] = (0.0, SIN(0.0, 0.05, 2e6))
    ct.observe_all_nodes()
    idt = slots_of(ct)
    engt = EngineCircuit(ct)
    spread(engt, idt, TRAN_SAMPLES)

    def tran():
        return engt.tran_sens(TRAN_SPAN[0], TRAN_SPAN[1], idt, tran_opts(stepper="host", dc=dc_opts(abstol=1e-12), abstol=1e-9, reltol=1e-6))

    calls = {
        "dc_sens": lambda: eng.dc_sens(ids, o),
        "ac_sens": lambda: eng.ac_sens(ids, f, o),
        "noise_sens": lambda: eng.noise_sens(0, c._n("d"), ids, f, o),
        "ac_measure": lambda: eng.ac_measure(ids, f, res.specs, len(res.names), o),
        "tran_sens": tran,
    }
    out = {"library": os.path.basename(LIB_PATH), "samples": S, "slots": len(ids), "frequencies": len(f), "tran_samples": TRAN_SAMPLES, "rounds": rounds}
    for name, call in calls.items():
        r = call()   # (first call: code objects are loaded, buffers sized)
        assert r[0] == 0, (name, r[0])
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            r = call()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
            assert r[0] == 0, (name, r[0])
        out[name + "_ms"] = round(statistics.median(ms), 3)
        out[name + "_all_ms"] = ms
    print(json.dumps(out))


if __name__ == "__main__":
    main()
