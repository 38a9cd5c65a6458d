"""Shapes and the one runner shared by tests/test_gpu_lockstep_bits.py and tests/golden/make_lockstep_bits.py: the device stepper's
complete outputs (t, every observed row, the final state without eliminated branches) for circuits that between them run the paired
lock-step kernel with and without a helper wave, a full workgroup, a pair whose every slot is a linear device, and a coupled array.

  case            circuit                        what it exercises
  dff3            dff_array(3)                   paired; three blocks: the last pair has a helper wave
  dff4            dff_array(4)                   paired; a full workgroup
  star_12_8       star(12, 8)                    every slot linear
  star12          star(11, 8)                    every slot linear, 32 slots: paired (the `star12` shape of test_gpu_newton_linear_path.py),
                                                 so the charge wave evaluates everything and the current wave nothing
  dff4_rails      dff_array(4, supply_r=1.0)     coupled through its rails, rows at DFF_CHECK_TIMES.  Its one block of 46 unknowns is below
                                                 the size at which an array is torn at its rails and above what the device stepper
                                                 takes, so it runs the host stepper over the per-attempt Newton kernels: the same
                                                 BSIM4 header in the other kernels that include it
  dff6_rails      dff_array(6, supply_r=1.0)     the same with more than 64 unknowns in the coupled block: the bordered form on the
                                                 device stepper

The stepper, its mode and the step counts are part of what is recorded, so a case that silently took another kernel fails."""
import numpy as np

from cedarsim_jl_amd import dc_opts, tran_opts
from cedarsim_jl_amd.workloads import DFF_CHECK_TIMES, DFF_TSPAN, dff_array


def _star(n_leaves, n_extra):
    from test_gpu_newton_linear_path import star
    return star(n_leaves, n_extra)


def _rails(tiles):
    c = dff_array(tiles, observe="q", supply_r=1.0)
    for n in ("vdd", "vss"):
        c.observe_node(n)
    return c


_DFF = dict(abstol=1e-4, reltol=1e-4, dc=dict(abstol=1e-14))
_RC = dict(abstol=1e-9, reltol=1e-9)
_RAILS = dict(abstol=1e-4, reltol=1e-4, saveat=np.array(DFF_CHECK_TIMES), dc=dict(abstol=1e-12))

# name -> (circuit maker, time span, transient options; `dc` holds the operating point's options, `stepper` defaults to "device")
CASES = {
    "dff3": (lambda: dff_array(3, observe="q"), DFF_TSPAN, _DFF),
    "dff4": (lambda: dff_array(4, observe="q"), DFF_TSPAN, _DFF),
    "star_12_8": (lambda: _star(12, 8), (0.0, 1e-5), _RC),
    "star12": (lambda: _star(11, 8), (0.0, 1e-5), _RC),
    "dff4_rails": (lambda: _rails(4), DFF_TSPAN, dict(_RAILS, stepper="auto")),
    "dff6_rails": (lambda: _rails(6), DFF_TSPAN, _RAILS),
}


def run_case(EngineCircuit, name):
    """One transient; returns {t, v, xf, meta} with meta = (stepper, mode, accepted, rejected, iterations)."""
    make, span, kw = CASES[name]
    kw = dict(kw)
    dc = kw.pop("dc", None)
    stepper = kw.pop("stepper", "device")
    e = EngineCircuit(make())
    opts = tran_opts(stepper=stepper, dc=dc_opts(**dc) if dc else None, **kw)
    rc, t, v, xf, st = e.tran(span[0], span[1], opts)
    assert rc == 0, (name, rc, e.ctx.last_error())
    xf = np.asarray(xf, dtype=np.float64)
    keep = ~np.isnan(xf)                       # eliminated branches carry NaN in the final state
    meta = np.array([st["stepper"], st["stepper_mode"], st["naccept"], st["nreject"], st["nnonliniter"]], dtype=np.int64)
    return {"t": np.asarray(t, dtype=np.float64), "v": np.asarray(v, dtype=np.float64), "xf": xf[keep],
            "xf_kept": keep.astype(np.uint8).ravel(), "meta": meta}
