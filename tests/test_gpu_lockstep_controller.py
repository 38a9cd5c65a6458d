"""The lock-step device controller's per-attempt path outside the device evaluation (cedarsim.jl_amd/csrc/ch_persist.hpp): BDF /
predictor coefficients (`p_coef`), the predictor's ring reads, the cached source pieces with their out-of-line miss path, the
saveat use of `p_coef`, and the wave-pair hand-off with a helper wave.  Everything is checked against the host stepper of the same
engine (one policy, two implementations: equal step and iteration counts) and against the oracle.  Small shapes: five tiles leave
the last wave pair with a helper wave; the linear circuits have one unknown."""
import numpy as np
import pytest

from cedarsim_jl_amd import PULSE, PWL, SIN, Circuit, dc_opts, tran_opts
from cedarsim_jl_amd.workloads import DFF_CHECK_TIMES, DFF_TSPAN, dff_array

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def counts(st):
    return st["naccept"], st["nreject"], st["nnonliniter"]


@pytest.mark.parametrize("tol", [1e-4, 1e-7])
def test_five_tiles_lockstep_counts_equal_the_host_steppers(E, tol):
    """Odd tile count without a saveat grid: workgroup 1 holds one block, its pair's second wave only helps.  1e-4 is the bench's
    tolerance; at 1e-7 the orders up to kmax and the order-raise path (the third predictor, ckp1) are in use.  Same bounds as
    test_bench_instantiation_is_the_lockstep_device_kernel_at_full_size."""
    e = E(dff_array(5, observe="q"))
    opts = dict(abstol=tol, reltol=tol, dc=dc_opts(abstol=1e-14))
    rc, t, v, _, st = e.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(**opts))
    assert rc == 0 and st["stepper"] == 2 and st["stepper_mode"] == 1, (rc, st["stepper"], st["stepper_mode"], e.ctx.last_error())
    rc_h, t_h, v_h, _, st_h = e.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(stepper="host", **opts))
    assert rc_h == 0 and st_h["stepper"] == 1
    print("tol %g: device %r host %r" % (tol, counts(st), counts(st_h)))
    assert counts(st) == counts(st_h)
    dt, dv = np.max(np.abs(t_h - t)), np.max(np.abs(v_h - v))
    print("max |dt| %.3e s, max |dv| %.3e V, tiles vs tile 0 %.3e V" % (dt, dv, np.max(np.abs(v - v[0:1]))))
    assert dt < 1e-12 and dv < 1e-4
    assert np.max(np.abs(v - v[0:1])) < 1e-9


def rc_lowpass(wave, held_through_0v_source=False):
    c = Circuit()
    c.V("v", "in", 0, dc=0.0, tran=wave)
    if held_through_0v_source:   # node "drv" = v(in) + 0 V: a known node whose entry has two terms
        c.V("v0", "drv", "in", dc=0.0)
    c.R("r", "drv" if held_through_0v_source else "in", "o", 1e3)
    c.C("c", "o", 0, 1e-9)
    c.observe_node("o")
    return c


SOURCE_CASES = {
    "pwl_corner": (PWL([0.0, 0.0, 1e-6, 1.0, 4e-6, 1.0, 5e-6, 0.25, 9e-6, 0.25]), False),
    "pwl_jump": (PWL([0.0, 0.0, 1e-6, 0.0, 1e-6, 1.0, 4e-6, 1.0, 6e-6, 0.0]), False),
    "pulse": (PULSE(0.0, 1.0, 5e-7, 2e-7, 3e-7, 1.5e-6, 4e-6), False),          # finite edges, 2.5 periods in the span
    "sin": (SIN(0.2, 1.0, 3e5, 1e-6, 1e5, 30.0), False),                        # delay and damping
    "two_terms": (PWL([0.0, 0.0, 1e-6, 1.0, 4e-6, 1.0, 5e-6, 0.25]), True),
}


@pytest.mark.parametrize("kind", sorted(SOURCE_CASES))
def test_source_entries_device_against_host_and_oracle(E, O, kind):
    """One RC low-pass (1 kOhm, 1 nF) per source kind, every step saved (lock-step).  PWL and the two-term entry stay inside a cached
    piece between corners (hit path) and leave it at every corner (miss path); PULSE and SIN have no piece and take the general
    body at every attempt; the corner / jump cases give both break-point codes.  Integration tolerances 1e-9 and the 1e-6 V bound are
    those of the RC closed form in test_transient_rc_and_pwl_closed_forms."""
    wave, two = SOURCE_CASES[kind]
    ckt = rc_lowpass(wave, two)
    e, o = E(ckt), O(ckt)
    span = (0.0, 1e-5)
    kw = dict(abstol=1e-9, reltol=1e-9)
    rc, t, v, _, st = e.tran(span[0], span[1], tran_opts(stepper="device", **kw))
    assert rc == 0 and st["stepper"] == 2 and st["stepper_mode"] == 1, (rc, st["stepper"], e.ctx.last_error())
    rc_h, t_h, v_h, _, st_h = e.tran(span[0], span[1], tran_opts(stepper="host", **kw))
    assert rc_h == 0 and st_h["stepper"] == 1
    print("%s: device %r host %r" % (kind, counts(st), counts(st_h)))
    assert counts(st) == counts(st_h)
    keep = np.concatenate(([True], np.diff(t) > 0))   # a jump is saved on both sides of its time
    rc_o, t_o, v_o, _, _ = o.tran(span[0], span[1], tran_opts(saveat=t[keep], **kw))
    assert rc_o == 0
    err = np.max(np.abs(v[0, keep, 0] - v_o[0]))
    print("%s: max |device - oracle| %.3e V over %d rows" % (kind, err, int(keep.sum())))
    assert err < 1e-6


def test_saveat_rows_of_the_lockstep_kernel_against_the_oracle(E, O):
    """The saveat use of `p_coef` (dense-output weights) on the lock-step kernel: the five-tile array on the grid of the five gate
    times and the batch shape n_comp == 1 with 8 samples, each with one shared step sequence (on a grid the default is own steps).  Both runs and the oracle start from the
    same operating point (the latches are bistable at t = 0)."""
    sv = np.array(DFF_CHECK_TIMES)
    kw = dict(abstol=1e-6, reltol=1e-6, saveat=sv, skip_dc=True)
    ckt = dff_array(5, observe="q")
    e = E(ckt)
    rc, x0, _, _ = e.dc(dc_opts(abstol=1e-14))
    assert rc == 0
    x0 = np.nan_to_num(x0, nan=0.0)
    rc, t, v, _, st = e.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(stepper="device", step_control="shared", dc=dc_opts(x0=x0), **kw))
    assert rc == 0 and st["stepper"] == 2 and st["stepper_mode"] == 1, (rc, st["stepper"], st["stepper_mode"], e.ctx.last_error())
    rc_o, t_o, v_o, _, _ = O(ckt).tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(dc=dc_opts(x0=x0[0]), **kw))
    assert rc_o == 0 and np.array_equal(t, sv)
    err = np.max(np.abs(v[:, :, 0] - v_o))
    print("five tiles on the gate grid: max |device - oracle| %.3e V" % err)
    assert err < 1e-4 * 5.0
    one = dff_array(1, observe="q0")
    e1 = E(one)
    e1.set_samples(8)
    rc, x1, _, _ = e1.dc(dc_opts(abstol=1e-14))
    assert rc == 0
    x1 = np.repeat(np.nan_to_num(x1, nan=0.0)[:1], 8, axis=0)   # every sample from sample 0's state
    rc, t1, v1, _, st1 = e1.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(stepper="device", step_control="shared", dc=dc_opts(x0=x1), **kw))
    assert rc == 0 and st1["stepper"] == 2 and st1["stepper_mode"] == 1 and v1.shape == (1, 5, 8), (rc, st1["stepper_mode"], v1.shape)
    rc_o, _, v1_o, _, _ = O(one).tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(dc=dc_opts(x0=x1[0]), **kw))
    assert rc_o == 0
    err1 = np.max(np.abs(v1[0] - v1_o[0][:, None]))
    print("8 samples on the gate grid: max |device - oracle| %.3e V" % err1)
    assert err1 < 1e-4 * 5.0
