"""Cases and the one runner shared by tests/test_gpu_tran_driver_bits.py and tests/golden/make_tran_driver_bits.py: the paths of the
transient and DC drivers (csrc/ch_engine_tran.hpp, ch_engine_dc.hpp, ch_engine_persist.hpp) that tests/lockstep_bits_cases.py does
not reach.

  case             circuit                         what it exercises
  own_batch        one DFF x 3 samples, saveat     device stepper, own steps per sample (a batch)
  own_blocks       dff_array(3), saveat            device stepper, own steps per block: per-workgroup constants and break points
  resume           dff_array(3), 100 rows/launch   device stepper, lock-step, drained and resumed launches
  host_rows        star(12, 8), stepper="host"     host stepper, every accepted step saved by the kernel's epilogue
  host_saveat      the same on a saveat grid       host stepper, dense output rows
  skip_dc          one DFF, u0 given               no operating point: the state is uploaded (u0 = this library's own DC result)
  tranop           one DFF, tran_mode              operating point with the sources at their t = 0 values
  dc_restarts_x3   one DFF x 3 samples, ch_dc      restarts, the donor pass and the gmin ladder (5 iterations per pass): x and status
  dc_restarts_b3   dff_array(3), ch_dc             the same with three blocks in one sample

A transient's record is t, v, the final state without eliminated branches and (stepper, mode, accepted, rejected, Newton iterations,
kernel launches); a DC case's is x, status and (rc, restarts, Newton iterations, block iterations)."""
import os

import numpy as np

from cedarsim_jl_amd import dc_opts, tran_opts
from cedarsim_jl_amd.workloads import DFF_TSPAN, dff_array

SPAN = (0.0, 2.0e-7)          # the clock's first edges: every phase of the stepper runs
GRID = np.linspace(0.0, 2.0e-7, 41)
_DFF = dict(abstol=1e-4, reltol=1e-4)
_RC = dict(abstol=1e-9, reltol=1e-9)
_FEW = dict(abstol=1e-14, maxiters=5, n_restarts=2)


def _engine(E, name):
    from test_gpu_tran_setup_cache import engine
    return engine(E, name)


def _star(E):
    from test_gpu_newton_linear_path import star
    return E(star(12, 8))


def _tran(e, span, maxrows=None, u0_from_dc=False, dc=None, **kw):
    dc = dict(dc or {})
    dc.setdefault("abstol", 1e-14)
    if u0_from_dc:
        rc, x, _, _ = e.dc(dc_opts(**dc))
        assert rc == 0, (rc, e.ctx.last_error())
        dc["x0"] = np.nan_to_num(np.asarray(x, np.float64), nan=0.0)
        kw["skip_dc"] = True
    if maxrows is not None:
        os.environ["CEDARHIP_PERSIST_MAXROWS"] = str(maxrows)
    try:
        rc, t, v, xf, st = e.tran(span[0], span[1], tran_opts(dc=dc_opts(**dc), **kw))
    finally:
        if maxrows is not None:
            del os.environ["CEDARHIP_PERSIST_MAXROWS"]
    assert rc == 0, (rc, e.ctx.last_error())
    xf = np.asarray(xf, np.float64)
    keep = ~np.isnan(xf)
    meta = [st[k] for k in ("stepper", "stepper_mode", "naccept", "nreject", "nnonliniter", "n_kernel_launches")]
    return {"t": np.asarray(t, np.float64), "v": np.asarray(v, np.float64), "xf": xf[keep], "xf_kept": keep.astype(np.uint8).ravel(),
            "meta": np.array(meta, np.int64)}


def _dc(e, **kw):
    rc, x, status, st = e.dc(dc_opts(**kw))
    x = np.asarray(x, np.float64)
    keep = ~np.isnan(x)
    meta = [rc, st["nrestarts"], st["nnonliniter"], st["n_block_iters"]]
    return {"x": x[keep], "x_kept": keep.astype(np.uint8).ravel(), "status": np.asarray(status, np.int64), "meta": np.array(meta, np.int64)}


# name -> (runner(EngineCircuit), expected (stepper, mode) of a transient or None for a DC case)
CASES = {
    "own_batch": (lambda E: _tran(_engine(E, "dff1x3"), SPAN, saveat=GRID, stepper="device", **_DFF), (2, 2)),
    "own_blocks": (lambda E: _tran(_engine(E, "dff3"), SPAN, saveat=GRID, stepper="device", **_DFF), (2, 2)),
    "resume": (lambda E: _tran(_engine(E, "dff3"), DFF_TSPAN, maxrows=100, stepper="device", **_DFF), (2, 1)),
    "host_rows": (lambda E: _tran(_star(E), (0.0, 1e-5), stepper="host", dc=dict(abstol=1e-10), **_RC), (1, 0)),
    "host_saveat": (lambda E: _tran(_star(E), (0.0, 1e-5), stepper="host", saveat=np.linspace(0.0, 1e-5, 33), dc=dict(abstol=1e-10), **_RC), (1, 0)),
    "skip_dc": (lambda E: _tran(E(dff_array(1, observe="q")), SPAN, u0_from_dc=True, stepper="device", **_DFF), (2, 1)),
    "tranop": (lambda E: _tran(E(dff_array(1, observe="q")), SPAN, dc=dict(tran_mode=True), stepper="device", **_DFF), (2, 1)),
    "dc_restarts_x3": (lambda E: _dc(_engine(E, "dff1x3"), **_FEW), None),
    "dc_restarts_b3": (lambda E: _dc(_engine(E, "dff3"), **_FEW), None),
}


def run_case(EngineCircuit, name):
    return CASES[name][0](EngineCircuit)
