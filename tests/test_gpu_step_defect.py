"""GPU tests that hold every Newton solver's ACCEPTED STEPS to the exact linear solve, through the public C-ABI alone.

The rest of the suite compares converged answers, and Newton's iteration hides what a hand-written LU gets wrong (a dropped fill-in,
a wrong multiplier in one row of a back substitution, a stale pivot reciprocal, a Schur slot added twice): in an operating point it
only costs iterations, and in a transient a step is accepted after one iteration, so a solve wrong by a relative eps leaves
eps times a tolerance-sized correction in the state.  Here the circuits are LINEAR, the tolerances loose and every step a row:
one Newton step with a fresh factorisation is then the exact solution of the step's variable-step BDF equation, which is written
down from the engine's own saved rows (order of a step = ch_result_dense_points - 1) and G, C, s(t) of the CPU oracle, and the
componentwise backward error w of every saved row (tests/step_defect.py, in longdouble) is held to

    worst w_engine <= K * max(worst w_reference, 2^-53),        and that bound itself <= 1e-12 on every case,

w_reference being the same measure of numpy.linalg.solve on the same history rows.  Each circuit's operating point from zero gets
the same check, and must take the oracle's number of Newton iterations (one solve: a solve wrong at 1e-6 needs a second).  The
cases (tests/step_defect_cases.py) are the smallest shapes at which each solver is a different piece of code; their excitation
condition is checked on the oracle in tests/test_step_defect_reference.py and asserted again here on the engine's rows.

The margin K cannot be derived (static pivot order, FMA, the engine's own reciprocal): it is the next power of two at or above four
times the worst ratio measured on the MI355X, see DESIGN.md 2.7h for the table every test here prints.

Not here: the own-steps mode of the device stepper (PM_OWN).  It only runs on a `saveat` grid, its rows are interpolants of the
steps, and an interpolant satisfies no step equation."""
import os

import numpy as np
import pytest

from cedarsim_jl_amd import dc_opts, tran_opts
from cedarsim_jl_amd.workloads import DFF_TSPAN, dff_array, rc_ladder

import step_defect as sd
import step_defect_cases as sc
from test_gpu_parity import canon
from transens_reference import Replay

pytestmark = pytest.mark.gpu
K = 16.0                     # the worst measured ratio w_engine / max(w_reference, 2^-53) is 3.9
FLOOR = 2.0 ** -53
CAP = 1e-12


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


class environment:
    """Environment switches set around the engine and restored afterwards (as tests/sparse_path_cases.py `run_case` does)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def hold(what, w, wr):
    """Prints the case's line of the table, then asserts the bound."""
    w, wr = float(w), float(wr)
    print("%-34s w_engine %.3e  w_reference %.3e  ratio %8.3f" % (what, w, wr, w / max(wr, FLOOR)))
    # no case may have a bound above 1e-12.  Where K times the reference's own w is above it (numpy's solve is backward stable in
    # the norm, not row by row: 1.2e-12 on the first, tiny steps of the mixed circuit), the cap is the bound.
    assert w <= min(K * max(wr, FLOOR), CAP), (what, w, wr)


def check_rows(what, c, t, v, st, G, C, s, maps=None):
    """One sample's saved rows: times, orders, excitation, the operating point in row 0 and the defect of every step."""
    pts = st["dense_points"]
    assert len(t) == st["naccept"] + 1 == len(pts) and np.all(np.diff(t) > 0), what
    orders = np.maximum(pts - 1, 0)
    assert np.all(orders[1:] >= 1) and np.all(orders[1:] <= np.minimum(5, np.arange(1, len(t)))), (what, orders)
    X = sc.rows_to_mna(c, v)
    cols = sc.unknown_columns(c)
    if maps is not None:      # the CPU-side rule for "unknown" names exactly the node voltages the engine keeps as unknowns
        nu = maps[0]
        assert sorted(m for m in cols if m < c.n_nodes) == [n - 1 for n in range(1, c.n_nodes + 1) if nu[n] >= 0], what
    med, move = sd.excitation(X, cols, c.n_nodes)
    print("%-34s %d steps, orders up to %d, median step %.2e of max|x|, least-moved unknown %.2e" % (what, len(t) - 1, orders.max(), med, move))
    assert med >= 1e-2 and move >= 1e-3, (what, med, move)
    w = sd.step_defects(t, orders, X, G, C, s)
    wr = sd.reference_defects(t, orders, X, G, C, s)
    hold(what + " steps", w.max(), wr.max())
    return X


def check_dc(what, e, o, G, s0):
    """The operating point from zero, full Newton steps: the oracle's iteration count and the defect of G x = s(0)."""
    n = e.n_mna
    rc, x, status, st = e.dc(dc_opts(abstol=1e-10, x0=np.zeros((1, n)), dv_max=0))
    rc_o, x_o, st_o = o.dc(dc_opts(abstol=1e-10, x0=np.zeros(n), dv_max=0))
    assert rc == 0 and rc_o == 0 and st["nrestarts"] == 0, (what, rc, rc_o)
    print("%-34s Newton iterations: engine %d, oracle %d" % (what + " dc", st["nnonliniter"], st_o["nnonliniter"]))
    assert st["nnonliniter"] == st_o["nnonliniter"], what
    hold(what + " dc", sd.dc_defect(x[0], G, s0), sd.dc_reference_defect(G, s0))


RUNS = {}


def run_case(E, O, name):
    """The transient and the operating point of one case of TRAN_CASES; the transient's statistics are kept in RUNS."""
    case = sc.TRAN_CASES[name]
    c = case["build"]()
    o = O(c)
    G, C, s = sd.linear_parts(o)
    with environment(case["env"]):
        e = E(c)
        opts = tran_opts(dtmax=case["dtmax"], stepper=case["force"] or "auto", dc=dc_opts(abstol=1e-12), **case["tol"])
        rc, t, v, xf, st = e.tran(case["span"][0], case["span"][1], opts)
        assert rc == 0, (name, rc, e.ctx.last_error())
        assert (e.info()["path"], st["stepper"], st["stepper_mode"]) == (case["path"], case["stepper"], case["mode"]), (name, e.info()["path"], st["stepper"], st["stepper_mode"])
        X = check_rows(name, c, t, v[:, :, 0], st, G, C, s, e.maps())
        if np.any(s(0.0, 0)):
            hold(name + " row 0 (operating point)", sd.dc_defect(X[0], G, s(0.0, 0)), sd.dc_reference_defect(G, s(0.0, 0)))
        else:   # every source is 0 at t = 0: the operating point is zero, and a backward error relative to zero says nothing.
            # The contract is the residual test's: |G x| < abstol = 1e-12 A through conductances of 1e-3 S and more.
            print("%-34s operating point of a circuit at rest: max|x| = %.3e" % (name + " row 0", np.nanmax(np.abs(X[0]))))
            assert np.nanmax(np.abs(X[0])) <= 1e-12 / 1e-3
        check_dc(name, e, o, G, s(0.0, 0))
    RUNS[name] = st
    return st


# ---- linear circuits ----
@pytest.mark.parametrize("n", sc.MESH_SIZES)
def test_fused_kernel_on_the_host_stepper(E, O, n):
    """newton_block_kernel: the linear dense mesh on both sides of every lu_variant edge (register LU 8 / 12 / 16 / 32, LDS LU above
    32) and at the path's cap of 64 unknowns."""
    e_info = run_case(E, O, "mesh%d" % n)
    assert e_info["naccept"] >= 12


def test_fused_kernel_with_every_linear_element(E, O):
    """An inductor branch, a VCCS, a VCVS and a floating source: three branch currents among the unknowns."""
    run_case(E, O, "mixed")


@pytest.mark.parametrize("name", ["lockstep7", "lockstep12", "lockstep13", "lockstep16", "lockstep7_nopair", "lockstep13_two_blocks"])
def test_device_stepper_in_lock_step(E, O, name):
    """tran_persistent_kernel<12 | 16>: five independent linear blocks of 7 (padded to 12), 12, 13 (padded to 16) and 16 unknowns,
    a lone block in the last workgroup; once without wave pairs and once with two blocks.  The device stepper is forced, so a
    circuit it does not take fails loudly."""
    run_case(E, O, name)


@pytest.mark.parametrize("name", ["tiles80", "two_rail72"])
def test_bordered_form(E, O, name):
    """PM_BORDER: a border of one unknown and of two.  The in-kernel operating point is the t = 0 row."""
    run_case(E, O, name)


@pytest.mark.parametrize("name", ["ladder40_sparse", "mesh65"])
def test_sparse_path(E, O, name):
    """The one-workgroup LU (a forced 40-unknown ladder) and the first mesh that leaves the fused path."""
    run_case(E, O, name)


def test_sparse_path_subtree_and_level_forms(E, O):
    """The two-rail array of 72 tiles untorn, in the subtree form and in the level-synchronous form: equal factorisation counts in
    a different number of launches, so both forms really ran."""
    a, b = run_case(E, O, "two_rail72_subtree"), run_case(E, O, "two_rail72_levels")
    print("subtree / levels: nfactors %d / %d, launches %d / %d" % (a["nfactors"], b["nfactors"], a["n_kernel_launches"], b["n_kernel_launches"]))
    assert a["nfactors"] == b["nfactors"] and a["n_kernel_launches"] != b["n_kernel_launches"]


def test_sparse_path_hub_ladder_of_4200(E):
    """Two-stage passes and a heavy CSR row.  G and C are written down as scipy.sparse matrices (held to the oracle at 40 unknowns
    on the CPU); the run starts from a seeded random state, so every one of the 4201 unknowns moves from the first step on."""
    n, spokes = 4200, 300
    c = sc.hub_ladder(n, spokes)
    G, C, s = sc.hub_ladder_matrices(n, spokes)
    x0 = np.random.default_rng(42).uniform(0.0, 1.0, (1, c.n_mna))
    x0[0, c.mna_index("v", "n0")] = 0.0
    with environment(sc.SPARSE):
        e = E(c)
        rc, t, v, xf, st = e.tran(0.0, 2e-9, tran_opts(dtmax=2.5e-10, skip_dc=True, dc=dc_opts(x0=x0), **sc.LOOSE))
        assert rc == 0 and e.info()["path"] == 2 and e.info()["n_unknowns"] == n + 1 and st["stepper"] == sc.HOST, (rc, e.ctx.last_error())
        assert 8 <= st["naccept"] <= 40
        X = check_rows("hub_ladder4200", c, t, v[:, :, 0], st, G, C, s, e.maps())
        assert np.array_equal(X[0, 1:n + 2], x0[0, 1:n + 2])      # the given start is row 0
        # operating point with the source's dc value at its final 1 V (at the waveform's own 0 V the answer is zero): ONE solve
        c1 = sc.hub_ladder(n, spokes)
        sc.set_wave(c1, "vin", 1.0, c1.sources[0][1])
        rc, x, status, st = E(c1).dc(dc_opts(abstol=1e-10, x0=np.zeros((1, c1.n_mna)), dv_max=0))
    assert rc == 0 and st["nrestarts"] == 0 and st["nnonliniter"] == 1, (rc, st["nnonliniter"])
    hold("hub_ladder4200 dc", sd.dc_defect(x[0], G, s(1.0)), sd.dc_reference_defect(G, s(1.0)))


def test_sparse_path_batch_of_three_ladders(E, O):
    """`ladder40_batch3` of tests/sparse_path_cases.py without a grid: three samples with their own r0, c0, r20, c20, one far
    stiffer; the batch shares one step sequence, and each sample's rows are held to the equations of ITS parameters."""
    c = sc.observe_all(rc_ladder(40))
    names = [("r0", "r"), ("c0", "c"), ("r20", "r"), ("c20", "c")]
    slots = [c.slot(*nm) for nm in names]
    vals = [np.array([1e3, 2.5e3, 1.0]), np.array([1e-12, 3e-12, 1e-15]), np.array([1e3, 4e2, 1e6]), np.array([1e-12, 5e-13, 1e-15])]
    with environment(sc.SPARSE):
        e = E(c)
        e.set_samples(3)
        e.set_params(slots, vals)
        rc, t, v, xf, st = e.tran(0.0, 2e-7, tran_opts(dtmax=2e-8, dc=dc_opts(abstol=1e-12), **sc.LOOSE))
        assert rc == 0 and e.info()["path"] == 2 and st["stepper"] == sc.HOST and v.shape[2] == 3, (rc, e.ctx.last_error())
        maps = e.maps()
    for k in range(3):
        o = O(c)
        for slot, val in zip(slots, vals):
            o.set_param(slot, val[k])
        # (C by a scaling of 2^70: at the default 2^40 the stiff sample's 1 fF beside its 1 S loses three digits of C)
        G, C, s = sd.linear_parts(o, c_scale=2.0 ** 70)
        check_rows("ladder40_batch3 sample %d" % k, c, t, v[:, :, k], st, G, C, s, maps)


# ---- nonlinear circuits ----
@pytest.mark.parametrize("n", sc.DC_MESH_SIZES)
def test_nonlinear_operating_point_takes_the_oracles_iterations(E, O, n):
    """`dense_mesh` with its MOSFETs (fused path to 40 unknowns, sparse path at 70) from the oracle's operating point plus a seeded
    1e-2 V on the unknown nodes, full Newton steps, one pass: a Jacobian or an LU wrong at 1 % turns quadratic convergence into
    linear convergence and adds iterations.  (The count is stable against abstol x 10 and / 10: checked on the CPU.)"""
    c = sc.mos_mesh(n)
    e, o = E(c), O(c)
    assert e.info()["n_unknowns"] == n and e.info()["n_components"] == 1
    nu, nk, bu = e.maps()
    rc, x_op, _ = o.dc(dc_opts(abstol=1e-14))
    assert rc == 0
    unknown = [False] + [bool(nu[k] >= 0) for k in range(1, c.n_nodes + 1)]
    assert unknown == [False] + [c.mna_index("v", nm) in sc.unknown_columns(c) for nm in c.node_names[1:]]   # the CPU test's start
    x0 = canon(c, sc.perturbed_start(c, x_op, unknown), nu)
    rc_o, _, st_o = o.dc(dc_opts(abstol=sc.DC_ABSTOL, x0=x0, dv_max=0, n_restarts=1))
    rc, x, status, st = e.dc(dc_opts(abstol=sc.DC_ABSTOL, x0=x0[None, :], dv_max=0, n_restarts=1))
    print("mesh of %d with MOSFETs: Newton iterations engine %d, oracle %d" % (n, st["nnonliniter"], st_o["nnonliniter"]))
    assert rc == 0 and rc_o == 0 and st["nrestarts"] == 0
    assert e.info()["path"] == (1 if n <= 64 else 2), e.info()        # (the path is decided with the first solve)
    assert st["nnonliniter"] == st_o["nnonliniter"]
    ok = ~np.isnan(x[0])
    assert np.allclose(x[0][ok], x_op[ok], rtol=1e-6, atol=1e-9)


def test_headline_kernel_rows_against_the_converged_newton_of_every_step(E, O):
    """dff_array(5) on the lock-step device stepper at the bench's tolerances, every step a row, every node observed: for each
    step the converged Newton on the engine's own history rows (q(x_j) from the oracle).  Asserted is the contract alone —
    wrms(x_i - x*_i) <= 1.0 in the controller's weights, the integration tolerance itself, and no convergence failure; the figure
    is reported, not tightened: the engine's history charge is the linearised q + C dx and the replay's is q(x_j), a second-order
    difference of the size of Newton's own remainder.  Measured on the MI355X: worst 1.7e-2 over 842 steps, median 1.1e-4
    (DESIGN.md 2.7h)."""
    tol = 1e-4
    c = sc.observe_all(dff_array(5))
    e, o = E(c), O(c)
    rc, t, v, xf, st = e.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(abstol=tol, reltol=tol, dc=dc_opts(abstol=1e-14), stepper="device"))
    assert rc == 0 and (st["stepper"], st["stepper_mode"]) == (sc.DEVICE, sc.LOCKSTEP) and st["nnonlinconvfail"] == 0, (rc, e.ctx.last_error())
    pts = st["dense_points"]
    assert len(t) == st["naccept"] + 1 and np.all(np.diff(t) > 0)
    orders = np.maximum(pts - 1, 0)
    assert np.all(orders[1:] >= 1) and np.all(orders[1:] <= np.minimum(5, np.arange(1, len(t))))
    nu = e.maps()[0]
    cols = np.array([n - 1 for n in range(1, c.n_nodes + 1) if nu[n] >= 0])
    err = sd.newton_replay_errors(Replay(o, c, []), t, orders, sc.rows_to_mna(c, v[:, :, 0]), cols, tol, tol)
    print("dff_array(5), lock-step device stepper, %d steps: worst wrms(x_i - x*_i) = %.3e (step %d), median %.3e"
          % (len(t) - 1, err.max(), int(np.argmax(err)), float(np.median(err[1:]))))
    assert err.max() <= 1.0
