"""Cases and the one runner shared by tests/test_gpu_pad_edges_bits.py and tests/golden/make_pad_edges_bits.py: circuits at the edges
of the padding that the device stepper's solve applies to a block (csrc/ch_persist.hpp: every block padded to the register-LU size
NC of its kernel, 12 or 16; lu_solve_block<NC, true>, RowDot<NC, 0, true> in csrc/ch_kernels.hpp).

  case        circuit                          nc / NC   what it exercises
  nc12        star(11, 8)                      12 / 12   no pad rows; every slot linear, 32 slots: the paired kernel
  dff1        dff_array(1)                     11 / 12   one pad row; one wave of the pair owns no block
  dff3        dff_array(3)                     11 / 12   one pad row; three blocks, the last pair has a helper wave
  dff3_own    dff_array(3) on a saveat grid    11 / 12   the same in own-steps mode (PM_OWN, per-workgroup constants)
  rc1         R-C low-pass, PWL drive           1 / 12   eleven pad rows
  rc1_own     the same x 3 samples, saveat      1 / 12   eleven pad rows in own-steps mode, unpaired
  nc13        star(12, 8)                      13 / 16   three pad rows on the NC = 16 kernel
  nc16        ring16()                         16 / 16   no pad rows on the NC = 16 kernel
  vfloat      a voltage source between two     3 / 12    the branch row has no diagonal: the static pivot order (the identity) stops
              unknown nodes                              holding, the full search (lu_solve_full_padded) runs and hands back a new order
  ind         an inductor between two nodes    3 / 12    the same through an inductor's branch
  bordered    dff_array(6, supply_r=1.0)       bordered form: keeps the unpadded images and its guarded solve

None of the circuits of test_gpu_newton_linear_path.py / test_gpu_stepper.py leaves the static pivot order at the recording commit
(stars, ring16, the R-C cases, the DFF at 1e-4 and 1e-7); vfloat and ind do, once each (profiles/r11_notes.md).

A record is t, v, the final state without eliminated branches and (stepper, mode, accepted, rejected, Newton iterations,
convergence failures); the stepper and the mode are asserted, so a case that fell back to the host stepper fails."""
import numpy as np

from cedarsim_jl_amd import PWL, Circuit, dc_opts, tran_opts
from cedarsim_jl_amd.workloads import DFF_CHECK_TIMES, DFF_TSPAN, dff_array

SPAN = (0.0, 2.0e-7)          # the DFF clock's first edges: every phase of the stepper runs
GRID = np.linspace(0.0, 2.0e-7, 41)
_DFF = dict(abstol=1e-4, reltol=1e-4, dc=dict(abstol=1e-14))
_RC = dict(abstol=1e-9, reltol=1e-9)


def _linear(name):
    import test_gpu_newton_linear_path as lp
    return {"nc12": lambda: lp.star(11, 8), "nc13": lambda: lp.star(12, 8), "nc16": lp.ring16}[name]()


def _rc1():
    c = Circuit()
    c.V("v", "in", 0, dc=0.0, tran=PWL([0.0, 0.0, 1e-6, 1.0, 4e-6, 1.0, 5e-6, 0.25, 9e-6, 0.25]))
    c.R("r", "in", "o", 1e3)
    c.C("c", "o", 0, 1e-9)
    c.observe_node("o")
    return c


def _branch(kind):
    """in -R- a -[V = 0.5 | L = 1 mH]- b -R||C- ground: three unknowns, one of them a branch current"""
    c = Circuit()
    c.V("v", "in", 0, dc=0.0, tran=PWL([0.0, 0.0, 1e-6, 1.0, 4e-6, 1.0, 5e-6, 0.25, 9e-6, 0.25]))
    c.R("r1", "in", "a", 1e3)
    if kind == "v":
        c.V("v2", "a", "b", dc=0.5)
    else:
        c.L("l1", "a", "b", 1e-3)
    c.R("r2", "b", 0, 1e3)
    c.C("c2", "b", 0, 1e-9)
    c.observe_node("a")
    c.observe_node("b")
    return c


def _rails6():
    c = dff_array(6, observe="q", supply_r=1.0)
    for n in ("vdd", "vss"):
        c.observe_node(n)
    return c


def _rc1_batch(E):
    c = _rc1()
    slot = c.slot("r", "r")
    e = E(c)
    e.set_samples(3)
    e.set_params([slot], [np.array([1000.0, 1300.0, 700.0])])
    return e


# name -> (engine maker(EngineCircuit), time span, transient options, expected (stepper, mode))
CASES = {
    "nc12": (lambda E: E(_linear("nc12")), (0.0, 1e-5), _RC, (2, 1)),
    "dff1": (lambda E: E(dff_array(1, observe="q")), SPAN, _DFF, (2, 1)),
    "dff3": (lambda E: E(dff_array(3, observe="q")), SPAN, _DFF, (2, 1)),
    "dff3_own": (lambda E: E(dff_array(3, observe="q")), SPAN, dict(_DFF, saveat=GRID), (2, 2)),
    "rc1": (lambda E: E(_rc1()), (0.0, 1e-5), _RC, (2, 1)),
    "rc1_own": (_rc1_batch, (0.0, 1e-5), dict(_RC, saveat=np.linspace(0.0, 1e-5, 33)), (2, 2)),
    "nc13": (lambda E: E(_linear("nc13")), (0.0, 1e-5), _RC, (2, 1)),
    "nc16": (lambda E: E(_linear("nc16")), (0.0, 1e-5), _RC, (2, 1)),
    "vfloat": (lambda E: E(_branch("v")), (0.0, 1e-5), _RC, (2, 1)),
    "ind": (lambda E: E(_branch("l")), (0.0, 1e-5), _RC, (2, 1)),
    "bordered": (lambda E: E(_rails6()), DFF_TSPAN, dict(abstol=1e-4, reltol=1e-4, saveat=np.array(DFF_CHECK_TIMES), dc=dict(abstol=1e-12)), (2, 3)),
}


def run_case(EngineCircuit, name):
    """One transient on the device stepper; returns {t, v, xf, xf_kept, meta}."""
    make, span, kw, _ = CASES[name]
    kw = dict(kw)
    dc = kw.pop("dc", None)
    e = make(EngineCircuit)
    rc, t, v, xf, st = e.tran(span[0], span[1], tran_opts(stepper="device", dc=dc_opts(**dc) if dc else None, **kw))
    assert rc == 0, (name, rc, e.ctx.last_error())
    xf = np.asarray(xf, dtype=np.float64)
    keep = ~np.isnan(xf)                       # eliminated branches carry NaN in the final state
    meta = np.array([st["stepper"], st["stepper_mode"], st["naccept"], st["nreject"], st["nnonliniter"], st["nnonlinconvfail"]], dtype=np.int64)
    return {"t": np.asarray(t, dtype=np.float64), "v": np.asarray(v, dtype=np.float64), "xf": xf[keep],
            "xf_kept": keep.astype(np.uint8).ravel(), "meta": meta}
