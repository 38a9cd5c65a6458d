"""The linear-algebra path of the device-resident stepper's Newton iteration (cedarsim.jl_amd/csrc/ch_persist.hpp): the gather over
the lane schedule of ch_gather_plan.hpp, the straight-line row loads and lu_solve_block.  Every shape runs the device stepper against
the host stepper of the same engine (one policy, two implementations: equal accepted / rejected / iteration counts) and against the
oracle, with the bounds of tests/test_gpu_lockstep_controller.py for the same circuit kind.  The `[blob]` diagnostic line confirms
that a shape is what it is meant to be:

  shape        nc   devices (slots)   work items   trips T   kernel
  dff3         11   31                70           3         NC 12, paired; three blocks: the last pair has a helper wave
  star12       12   31                46           5         NC 12 (no padded column), paired; hub row and diagonal: 20 sources
  star12_wide  12   34                46           6         NC 12, one wave per block; hub row and diagonal: 23 sources
  star16       16   31                62           4         NC 16, paired; hub row and diagonal: 16 sources
  ring16       16   25                80           2         NC 16, paired; more than 64 items, none above four sources
"""
import re

import numpy as np
import pytest

from cedarsim_jl_amd import PWL, Circuit, dc_opts, tran_opts
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


def blob_line(text):
    """{nc, slots, work, trips} of class 0 from the engine's `[blob]` line"""
    m = re.search(r"\[blob\] class 0: nc (\d+) ndev (\d+) slots (\d+) mat_src \d+ vec_src \d+ work (\d+) blob_ints \d+ trips (\d+)", text)
    assert m, text[-2000:]
    return dict(nc=int(m.group(1)), ndev=int(m.group(2)), slots=int(m.group(3)), work=int(m.group(4)), trips=int(m.group(5)))


DRIVE = PWL([0.0, 0.0, 1e-6, 1.0, 4e-6, 1.0, 5e-6, 0.25, 9e-6, 0.25])


def star(n_leaves, n_extra):
    """A hub behind 1 kOhm from the driven node, n_leaves leaves each behind its own resistor with its own capacitor to ground;
    the first n_extra leaves are also coupled to the hub by a capacitor.  Every element on the hub adds one source to the hub's
    row of F / Q and to its diagonal; values differ from leaf to leaf so that no two rows are equal."""
    c = Circuit()
    c.V("v", "in", 0, dc=0.0, tran=DRIVE)
    c.R("rin", "in", "h", 1e3)
    for i in range(n_leaves):
        c.R("r%d" % i, "h", "l%d" % i, 1e3 * (1.0 + 0.1 * i))
        c.C("c%d" % i, "l%d" % i, 0, 1e-9 * (1.0 + 0.05 * i))
        if i < n_extra:
            c.C("x%d" % i, "h", "l%d" % i, 2e-10 * (1.0 + 0.03 * i))
    c.observe_node("h")
    c.observe_node("l0")
    c.observe_node("l%d" % (n_leaves - 1))
    return c


def ring16():
    """Sixteen nodes on a ring of resistors, opposite nodes coupled by capacitors, node 0 driven through 1 kOhm: 16 rows, 16 diagonals
    and 2 x 24 off-diagonal entries = 80 work items of three or four sources each."""
    c = Circuit()
    c.V("v", "in", 0, dc=0.0, tran=DRIVE)
    c.R("rin", "in", "n0", 1e3)
    for i in range(16):
        c.R("r%d" % i, "n%d" % i, "n%d" % ((i + 1) % 16), 500.0 * (1.0 + 0.07 * i))
    for i in range(8):
        c.C("c%d" % i, "n%d" % i, "n%d" % (i + 8), 1e-9 * (1.0 + 0.1 * i))
    c.observe_node("n0")
    c.observe_node("n5")
    c.observe_node("n8")
    return c


LINEAR_CASES = {
    "star12": (lambda: star(11, 8), dict(nc=12, ndev=31, work=46, trips=5), True),
    "star12_wide": (lambda: star(11, 11), dict(nc=12, ndev=34, work=46, trips=6), False),
    "star16": (lambda: star(15, 0), dict(nc=16, ndev=31, work=62, trips=4), True),
    "ring16": (ring16, dict(nc=16, ndev=25, work=80, trips=2), True),
}


@pytest.mark.parametrize("kind", sorted(LINEAR_CASES))
def test_linear_shapes_device_against_host_and_oracle(E, O, kind, monkeypatch, capfd):
    """Integration tolerances 1e-9 and the 1e-6 V bound are those of the RC cases of test_source_entries_device_against_host_and_oracle
    (linear RC networks on the same drive, every step saved, lock-step)."""
    make, shape, paired = LINEAR_CASES[kind]
    monkeypatch.setenv("CEDARHIP_DEBUG_BLOB", "1")
    ckt = make()
    e, o = E(ckt), O(ckt)
    span = (0.0, 1e-5)
    kw = dict(abstol=1e-9, reltol=1e-9)
    rc, t, v, _, st = e.tran(span[0], span[1], tran_opts(stepper="device", **kw))
    got = blob_line(capfd.readouterr().err)
    print("%s: %r" % (kind, got))
    assert {k: got[k] for k in shape} == shape
    assert (got["slots"] <= 32) == paired
    assert rc == 0 and st["stepper"] == 2 and st["stepper_mode"] == 1, (rc, st["stepper"], st["stepper_mode"], e.ctx.last_error())
    rc_h, t_h, v_h, _, st_h = e.tran(span[0], span[1], tran_opts(stepper="host", **kw))
    assert rc_h == 0 and st_h["stepper"] == 1
    print("%s: device %r host %r" % (kind, counts(st), counts(st_h)))
    assert counts(st) == counts(st_h)
    keep = np.concatenate(([True], np.diff(t) > 0))
    rc_o, t_o, v_o, _, _ = o.tran(span[0], span[1], tran_opts(saveat=t[keep], **kw))
    assert rc_o == 0
    err = np.max(np.abs(v[:, keep, 0] - v_o))
    print("%s: max |device - oracle| %.3e V over %d rows" % (kind, err, int(keep.sum())))
    assert err < 1e-6


def test_three_tiles_device_against_host_and_oracle(E, O, monkeypatch, capfd):
    """dff_array(3) at the bench's tolerance without a saveat grid: counts equal to the host stepper's, the bounds of
    test_five_tiles_lockstep_counts_equal_the_host_steppers; then the gate grid against the oracle from a common operating point
    with the bound of test_saveat_rows_of_the_lockstep_kernel_against_the_oracle."""
    monkeypatch.setenv("CEDARHIP_DEBUG_BLOB", "1")
    ckt = dff_array(3, observe="q")
    e = E(ckt)
    opts = dict(abstol=1e-4, reltol=1e-4, dc=dc_opts(abstol=1e-14))
    rc, t, v, _, st = e.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(**opts))
    got = blob_line(capfd.readouterr().err)
    print("dff3: %r" % got)
    assert (got["nc"], got["work"], got["trips"]) == (11, 70, 3) and got["slots"] <= 32
    assert rc == 0 and st["stepper"] == 2 and st["stepper_mode"] == 1, (rc, st["stepper"], st["stepper_mode"], e.ctx.last_error())
    rc_h, t_h, v_h, _, st_h = e.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(stepper="host", **opts))
    assert rc_h == 0 and st_h["stepper"] == 1
    print("dff3: device %r host %r" % (counts(st), counts(st_h)))
    assert counts(st) == counts(st_h)
    dt, dv = np.max(np.abs(t_h - t)), np.max(np.abs(v_h - v))
    print("max |dt| %.3e s, max |dv| %.3e V, tiles vs tile 0 %.3e V" % (dt, dv, np.max(np.abs(v - v[0:1]))))
    assert dt < 1e-12 and dv < 1e-4
    assert np.max(np.abs(v - v[0:1])) < 1e-9
    sv = np.array(DFF_CHECK_TIMES)
    kw = dict(abstol=1e-6, reltol=1e-6, saveat=sv, skip_dc=True)
    rc, x0, _, _ = e.dc(dc_opts(abstol=1e-14))
    assert rc == 0
    x0 = np.nan_to_num(x0, nan=0.0)
    rc, t2, v2, _, st2 = e.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(stepper="device", step_control="shared", dc=dc_opts(x0=x0), **kw))
    assert rc == 0 and st2["stepper"] == 2 and st2["stepper_mode"] == 1, (rc, st2["stepper"], st2["stepper_mode"], e.ctx.last_error())
    rc_o, t_o, v_o, _, _ = O(ckt).tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(dc=dc_opts(x0=x0[0]), **kw))
    assert rc_o == 0 and np.array_equal(t2, sv)
    err = np.max(np.abs(v2[:, :, 0] - v_o))
    print("three tiles on the gate grid: max |device - oracle| %.3e V" % err)
    assert err < 1e-4 * 5.0
