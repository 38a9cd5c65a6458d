"""Shapes and runners shared by tests/test_gpu_b4_bits.py and tests/golden/make_b4_bits.py: what the BSIM4 device code computes,
pinned bit by bit over the card space of tests/bsim4_cards.py (the DFF cards of tests/lockstep_bits_cases.py never take the
branches for mobmod 1 / 2, capmod 0, the xpart cases, ngate, isub, gidl, dvtp0, pdits, k1 = 0, nor the junction-free case).

  stamps    ch_mos_eval on fet_bank(name, 41 rows) for every card variant at 27 C and `base` at -40 and 125 C; ch_mos_eval_quad
            for base, mob2, cap0 and geom.  Rows: the 11 edge rows of bias_rows() and the first 10 of each of its three random boxes.
  chain     inverter_chain(name) on the device stepper (lock-step), once paired and once with CEDARHIP_PERSIST_NOPAIR=1; the
            operating point is the engine's own.  CHAIN_CANDIDATES are tried when the goldens are recorded; those whose run returns 0
            are recorded, and the recorded list is the test's list.  Every name of CIRCUIT_NAMES must be among them.
  own       dff_array(3) with private, skewed clocks on the DFF_CHECK_TIMES grid: the per-block step controller.

The stepper, its mode and the step counts are part of what is recorded, so a case that took another kernel fails."""
import os

import numpy as np

import bsim4_cards as BC
from cedarsim_jl_amd import dc_opts, tran_opts
from cedarsim_jl_amd.workloads import DFF_CHECK_TIMES, DFF_TSPAN, dff_array

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "b4_bits.npz")

_ALL = BC.bias_rows()                     # three random boxes of 30 rows, then the 11 edge rows
ROWS = np.vstack([_ALL[90:], _ALL[0:10], _ALL[30:40], _ALL[60:70]])
assert ROWS.shape == (41, 4) and len(_ALL) == 101
VBANK = BC.bank_voltages(ROWS)            # 82 instances

QUAD_NAMES = ("base", "mob2", "cap0", "geom")
# (variant, temperature in Celsius)
STAMP_CASES = [(n, 27.0) for n in BC.NAMES] + [("base", -40.0), ("base", 125.0)]


def stamp_key(name, temp, quad):
    return "stamps/%s/%g/%s" % (name, temp, "quad" if quad else "plain")


def run_stamps(EngineCircuit, name, temps):
    """{key: (82, 40) record array} for one variant at each of `temps`; one engine circuit serves them all."""
    c = BC.fet_bank(name, rows=len(ROWS))
    e = EngineCircuit(c)
    st = c.slot("temp")
    out = {}
    for temp in temps:
        e.set_params([st], [[temp]])
        out[stamp_key(name, temp, False)] = np.asarray(e.mos_eval(VBANK), dtype=np.float64)
        if name in QUAD_NAMES:
            out[stamp_key(name, temp, True)] = np.asarray(e.mos_eval(VBANK, quad=True), dtype=np.float64)
    return out


def _record(rc, t, v, xf, st):
    xf = np.asarray(xf, dtype=np.float64)
    keep = ~np.isnan(xf)                       # eliminated branches carry NaN in the final state
    meta = np.array([st["stepper"], st["stepper_mode"], st["naccept"], st["nreject"], st["nnonliniter"]], dtype=np.int64)
    return {"t": np.asarray(t, dtype=np.float64), "v": np.asarray(v, dtype=np.float64), "xf": xf[keep],
            "xf_kept": keep.astype(np.uint8).ravel(), "meta": meta}


CHAIN_CANDIDATES = list(BC.CIRCUIT_NAMES) + ["minv", "rout"]
CHAIN_TOL = 1e-7                               # test_gpu_bsim4_cards.py


def run_chain(EngineCircuit, name):
    """(rc, record or None).  The caller sets or clears CEDARHIP_PERSIST_NOPAIR before the call."""
    e = EngineCircuit(BC.inverter_chain(name))
    opts = tran_opts(stepper="device", abstol=CHAIN_TOL, reltol=CHAIN_TOL, saveat=BC.CHAIN_SAVEAT, dc=dc_opts(abstol=1e-14))
    rc, t, v, xf, st = e.tran(BC.CHAIN_TSPAN[0], BC.CHAIN_TSPAN[1], opts)
    return rc, (_record(rc, t, v, xf, st) if rc == 0 else None)


def run_own(EngineCircuit):
    e = EngineCircuit(dff_array(3, skew=[0.0, 20e-12, 40e-12], observe="q"))
    opts = tran_opts(stepper="device", abstol=1e-4, reltol=1e-4, saveat=np.array(DFF_CHECK_TIMES), dc=dc_opts(abstol=1e-14))
    rc, t, v, xf, st = e.tran(DFF_TSPAN[0], DFF_TSPAN[1], opts)
    assert rc == 0, (rc, e.ctx.last_error())
    return _record(rc, t, v, xf, st)


def recorded_chain_names():
    """The chain variants the golden file holds, in CHAIN_CANDIDATES order."""
    with np.load(GOLDEN) as z:
        have = set(k.split("/")[1] for k in z.files if k.startswith("chain/"))
    return [n for n in CHAIN_CANDIDATES if n in have]
