"""GPU tests of the transient parameter sensitivities (ch_tran_sens, direct method on the host stepper's accepted steps).

The yardstick is tests/transens_reference.py: the CPU oracle's residuals, a replay of the variable-coefficient BDF on the accepted
times and orders of the engine's run (order of a step = ch_result_dense_points - 1) in full MNA coordinates, and the s / w recursion
with Richardson-extrapolated partials.  Tolerance: 1e-6 of max_t |s_k| per slot, the project's figure for dc_sens.  Every comparison
prints its measured figure before it asserts."""
import ctypes

import numpy as np
import pytest

from cedarsim_jl_amd import Circuit, CircuitSweep, PULSE, SIN, Sweep, dc_opts, tran_opts, tran_sens
from cedarsim_jl_amd.circuit import CedarError

from test_gpu_ac_noise import amp_circuit
from transens_reference import Replay, lagrange_rows

pytestmark = pytest.mark.gpu
TOL = 1e-6
TIGHT = dict(abstol=1e-12, reltol=1e-9)


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def slot_of(c, name):
    return c.slot(*name) if isinstance(name, tuple) else c.slot(name)


def obs_rows(c):
    """MNA index of every observable, in the order of the result rows."""
    return [o[1] - 1 if o[0] == "v" else c.mna_index("i", c.dev_names[o[1]]) for o in c.obs]


def host(**kw):
    return tran_opts(stepper="host", **kw)


def compare(what, names, sens, ref, tol=TOL):
    """sens, ref: [n_obs][n_par][n_times].  Per slot: max|sens - ref| <= tol * max|ref| over all rows; none of the circuits compared
    here has a row that may be NaN."""
    assert np.all(np.isfinite(sens)), what
    worst = {}
    for k, nm in enumerate(names):
        a, r = sens[:, k, :], ref[:, k, :]
        ok = ~np.isnan(a)
        scale = float(np.max(np.abs(r[ok])))
        err = float(np.max(np.abs(a[ok] - r[ok])))
        worst[str(nm)] = err / scale if scale else err
        print("%s %s: max|s - r| / max|r| = %.3e (max|r| = %.3e)" % (what, nm, worst[str(nm)], scale))
    for k, nm in enumerate(names):
        a, r = sens[:, k, :], ref[:, k, :]
        ok = ~np.isnan(a)
        scale = float(np.max(np.abs(r[ok])))
        assert float(np.max(np.abs(a[ok] - r[ok]))) <= tol * scale, (what, nm, worst[str(nm)])
    return worst


def against_replay(what, E, O, c, names, t0, t1, dc_start=True, point=None, saveat=None, **kw):
    """One engine run without a grid (accepted times and orders), the replay on them, the comparison; with `saveat` a second run on
    that grid against the replay's Lagrange rows.  Returns (engine result of the first run, replay x, replay s)."""
    ids = [slot_of(c, n) for n in names]
    rows = obs_rows(c)
    e = E(c)
    opts = dict(TIGHT)
    opts.update(kw)
    x0 = None if dc_start else np.zeros((1, c.n_mna))
    mk = lambda **more: host(dc=dc_opts(abstol=1e-12, x0=x0), skip_dc=not dc_start, **opts, **more)   # noqa: E731
    rc, t, v, xf, st, sens = e.tran_sens(t0, t1, ids, mk())
    assert rc == 0, e.ctx.last_error()
    pts = st["dense_points"]
    st["path"] = e.info()["path"]
    print("%s: %d accepted steps, highest order %d" % (what, len(t) - 1, int(np.max(pts)) - 1))
    rp = Replay(O(c), c, ids, point)
    if dc_start:
        xs, s0 = rp.dc_start()
    else:
        xs, s0 = np.zeros(rp.n), None
    x, s = rp.run(t, np.maximum(pts - 1, 0), xs, s0)
    lo = 0 if dc_start else 1       # from a given zero start, row 0 is that start: the replay's holds 0 where the engine reports a source's node
    state_err = float(np.max(np.abs(v[:, lo:, 0] - x[lo:, rows].T)))
    print("%s: state mismatch engine / replay max|dx| = %.3e (max|x| = %.3e)" % (what, state_err, float(np.max(np.abs(x)))))
    assert state_err <= TOL * float(np.max(np.abs(x))), (what, state_err)
    ref = np.transpose(s[:, :, rows], (2, 1, 0))
    worst = compare(what, names, sens[:, :, :, 0], ref)
    if saveat is not None:
        rc2, t2, v2, _, st2, sens2 = e.tran_sens(t0, t1, ids, mk(saveat=saveat))
        assert rc2 == 0 and np.array_equal(t2, saveat)
        ref2 = np.transpose(lagrange_rows(t, pts, s[:, :, rows], saveat), (2, 1, 0))
        compare(what + " (saveat)", names, sens2[:, :, :, 0], ref2)
        assert np.max(np.abs(v2[:, :, 0] - lagrange_rows(t, pts, x[:, rows], saveat).T)) <= 1e-6 * max(1.0, float(np.max(np.abs(x))))
    return (rc, t, v, xf, st, sens), x, s, worst


# ---- circuits ----
def divider(observe_branch):
    c = Circuit()
    c.V("v", "vcc", 0, dc=1.0)
    c.R("r1", "vcc", "out", 1.0)
    c.R("r2", "out", 0, 1.0)
    c.observe_all_nodes()
    if observe_branch:
        c.observe_branch("v")
    return c


def rc_circuit():
    c = Circuit()
    c.V("v", "in", 0, dc=0.2, tran=SIN(0.2, 1.0, 1e6))
    c.R("r1", "in", "out", 1e3)
    c.C("c1", "out", 0, 1e-10)
    c.observe_all_nodes()
    return c


def two_pole():
    """Two RC poles, an inductor branch and a VCCS stage, driven by a SIN: every linear element kind on a transient's path."""
    c = Circuit(gmin=1e-9)
    c.V("v1", "in", 0, dc=0.5, tran=SIN(0.5, 0.4, 5e5))
    c.R("r1", "in", "a", 1e3)
    c.C("c1", "a", 0, 2e-10)
    c.R("r2", "a", "b", 2e3)
    c.C("c2", "b", 0, 1e-10)
    c.L("l1", "b", "d", 1e-4)
    c.R("r3", "d", 0, 5e2)
    c.G("g1", "e", 0, "a", 0, gain=1e-3)
    c.R("r4", "e", 0, 1e3)
    c.C("c3", "e", 0, 1e-10)
    c.observe_all_nodes()
    c.observe_branch("l1")
    return c


TWO_POLE_SLOTS = ["r1", "c1", "l1", ("v1", 1), ("r1", "m"), "g1", "gmin"]


def amp_tran():
    """amp_circuit with a SIN on the gate's coupling source and a load capacitor on the second stage."""
    c = amp_circuit()
    i = c.dev_ipar[c.dev_names.index("vin")][0]
    c.sources[i] = (0.0, SIN(0.0, 0.05, 2e6))
    c.C("cload", "o", 0, 2e-12)
    c.observe_all_nodes()
    return c


AMP_SLOTS = ["vdd", "rd", ("m1", "w"), ("nfet_06v0", "vth0"), "temp"]
AMP_SPAN = (0.0, 3e-8)


def rc_ladder(n):
    """n sections of series R and shunt C behind a 1 V source: n unknowns in one block, every value distinct."""
    c = Circuit()
    c.V("v", "n0", 0, dc=1.0)
    for i in range(1, n + 1):
        c.R("rs%d" % i, "n%d" % (i - 1), "n%d" % i, 1e3 * (1.0 + 0.01 * ((7 * i) % 13)))
        c.C("cp%d" % i, "n%d" % i, 0, 1e-12 * (1.0 + 0.01 * ((5 * i) % 11)))
    c.observe_all_nodes()
    return c


# ---- 4. the reference's own test (test/sensitivity.jl) ----
def test_the_reference_divider(E):
    c = divider(observe_branch=False)
    ids = [c.slot("r1"), c.slot("r2"), c.slot("v")]
    e = E(c)
    rc, t, v, xf, st, s = e.tran_sens(0.0, 1e-5, ids, host())
    assert rc == 0 and len(t) >= 2 and s.shape == (2, 3, len(t), 1)
    out, vcc = c.obs.index(("v", c._n("out"))), c.obs.index(("v", c._n("vcc")))
    assert e.maps()[1][c._n("vcc")] >= 0                                  # the source node is a known node here
    assert s[out, 0, :, 0] == pytest.approx(-0.25, rel=1e-9) and s[out, 1, :, 0] == pytest.approx(+0.25, rel=1e-9)
    assert np.all(np.abs(s[out, 0, :, 0] + s[out, 1, :, 0]) <= 1e-9 * 0.25)          # dR1 = -dR2 at every saved time
    assert s[out, 2, :, 0] == pytest.approx(0.5, rel=1e-12)
    assert np.all(s[vcc, 2, :, 0] == 1.0) and np.all(s[vcc, :2, :, 0] == 0.0)        # the known node: exact
    assert v[out, :, 0] == pytest.approx(0.5, rel=1e-12)
    # the source current observed: its branch is kept, its rows are the derivatives of -V/(R1 + R2)
    c = divider(observe_branch=True)
    ids = [c.slot("r1"), c.slot("r2"), c.slot("v")]
    rc, t, v, xf, st, s = E(c).tran_sens(0.0, 1e-5, ids, host())
    iv = c.obs.index(("i", c.dev_names.index("v")))
    assert rc == 0 and np.all(np.isfinite(s))
    assert np.abs(s[iv, 0, :, 0]) == pytest.approx(0.25, rel=1e-9) and np.abs(s[iv, 2, :, 0]) == pytest.approx(0.5, rel=1e-9)
    assert s[c.obs.index(("v", c._n("vcc"))), 2, :, 0] == pytest.approx(1.0, rel=1e-12)
    # the user-facing form
    sol = tran_sens(divider(observe_branch=False), ["r1", "r2", "v"], (0.0, 1e-5))
    assert sol.retcode == "Success" and len(sol.t) >= 2
    assert sol.sens["node_out", "r1"] == pytest.approx(-0.25, rel=1e-9) and sol.sens["out", "r2"] == pytest.approx(0.25, rel=1e-9)
    assert sol.sens["r1.v", "v"] == pytest.approx(0.5, rel=1e-12) and sol["node_out"] == pytest.approx(0.5, rel=1e-12)
    assert sol.sens(0.5e-5, idxs="node_out", par="r1") == pytest.approx(-0.25, rel=1e-9)
    assert sol.sens([0.2e-5, 0.7e-5], idxs=["node_out"], par="r2")[0] == pytest.approx([0.25, 0.25], rel=1e-9)
    with pytest.raises(KeyError):
        sol.sens["out", "nosuch"]


# ---- 5. the state path is ch_tran's on the host stepper, bit for bit ----
@pytest.mark.parametrize("which", ["rc", "amp"])
def test_state_path_is_untouched(E, which):
    c, names, span = (rc_circuit(), ["r1", "c1", ("v", 1)], (0.0, 5e-8)) if which == "rc" else (amp_tran(), AMP_SLOTS, AMP_SPAN)
    ids = [slot_of(c, n) for n in names]
    e = E(c)
    o = lambda: host(dc=dc_opts(abstol=1e-12), **TIGHT)   # noqa: E731
    a = e.tran(span[0], span[1], o())
    b = e.tran_sens(span[0], span[1], ids, o())
    d = e.tran(span[0], span[1], o())
    assert a[0] == 0 and b[0] == 0 and d[0] == 0 and len(a[1]) > 5
    for r in (b, d):   # times, values, final state, dense points
        assert np.array_equal(a[1], r[1]) and np.array_equal(a[2], r[2]) and np.array_equal(a[3], r[3], equal_nan=True)
        assert np.array_equal(a[4]["dense_points"], r[4]["dense_points"])
    for key in ("naccept", "nreject", "nnonlinconvfail", "nnonliniter", "n_step_attempts"):
        assert a[4][key] == b[4][key], key
    assert b[4]["stepper"] == 1 and np.all(np.isfinite(b[5]))
    # on a saveat grid as well
    sv = np.linspace(span[0], span[1], 7)
    a = e.tran(span[0], span[1], host(dc=dc_opts(abstol=1e-12), saveat=sv, **TIGHT))
    b = e.tran_sens(span[0], span[1], ids, host(dc=dc_opts(abstol=1e-12), saveat=sv, **TIGHT))
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3], equal_nan=True)
    assert b[5].shape == (len(c.obs), len(ids), 7, 1)
    # the device stepper is refused, AUTO means the host stepper
    rc, *_ = e.tran_sens(span[0], span[1], ids, tran_opts(stepper="device", **TIGHT))
    assert rc == -6 and "host stepper" in e.ctx.last_error()
    rc, *rest = e.tran_sens(span[0], span[1], ids, tran_opts(dc=dc_opts(abstol=1e-12), **TIGHT))
    assert rc == 0 and rest[3]["stepper"] == 1


# ---- 6. linear circuits against the replay ----
def test_linear_two_pole_against_the_replay(E, O):
    """Measured on the MI355X (max|s - r| / max|r| per slot, free run / saveat grid): see DESIGN.md 2.7d."""
    c = two_pole()
    (rc, t, v, xf, st, sens), x, s, worst = against_replay("two-pole", E, O, c, TWO_POLE_SLOTS, 0.0, 1e-7, saveat=np.linspace(0.0, 1e-7, 14)[1:-1] * 1.003)
    assert int(np.max(st["dense_points"])) - 1 >= 3                       # the run reached order 3
    assert np.max(np.abs(sens[:, TWO_POLE_SLOTS.index("c1")])) > 0.0 and np.max(np.abs(sens[:, TWO_POLE_SLOTS.index("l1")])) > 0.0


# ---- 7. nonlinear against the replay ----
@pytest.fixture(scope="module")
def amp_replay(E, O):
    """The amplifier's run and its replay, computed once and shared."""
    c = amp_tran()
    res, x, s, worst = against_replay("amplifier", E, O, c, AMP_SLOTS, *AMP_SPAN, saveat=np.linspace(AMP_SPAN[0], AMP_SPAN[1], 9)[1:-1] * 1.01)
    return c, res, x, s


def test_amplifier_against_the_replay(amp_replay):
    c, (rc, t, v, xf, st, sens), x, s = amp_replay
    assert rc == 0 and st["stepper"] == 1
    assert np.max(np.abs(sens[c.obs.index(("v", c._n("o"))), AMP_SLOTS.index("rd")])) > 0.0


def test_amplifier_on_the_sparse_path(E, O, amp_replay, monkeypatch):
    c, (rc, t, v, xf, st, sens), x, s = amp_replay
    ids = [slot_of(c, n) for n in AMP_SLOTS]
    monkeypatch.setenv("CEDARHIP_FORCE_SPARSE", "1")
    try:
        e = E(c)
        res = e.tran_sens(AMP_SPAN[0], AMP_SPAN[1], ids, host(dc=dc_opts(abstol=1e-12), **TIGHT))
        path = e.info()["path"]
    finally:
        monkeypatch.delenv("CEDARHIP_FORCE_SPARSE", raising=False)
    assert res[0] == 0 and path == 2
    # the sparse path takes its own steps: its own replay
    rows = obs_rows(c)
    rp = Replay(O(c), c, ids)
    xs, s0 = rp.dc_start()
    pts = res[4]["dense_points"]
    x2, s2 = rp.run(res[1], np.maximum(pts - 1, 0), xs, s0)
    print("sparse amplifier: %d accepted steps, state mismatch %.3e" % (len(res[1]) - 1, np.max(np.abs(res[2][:, :, 0] - x2[:, rows].T))))
    compare("sparse amplifier", AMP_SLOTS, res[5][:, :, :, 0], np.transpose(s2[:, :, rows], (2, 1, 0)))


def test_amplifier_against_differenced_oracle_transients(O, amp_replay):
    """A reported figure, not a bound: the Richardson central difference of two full adaptive Oracle.tran runs on the saveat grid
    beside the engine's frozen-step derivative, with that yardstick's own error estimate |y2 - r|."""
    c, (rc, t, v, xf, st, sens), x, s = amp_replay
    sv = np.linspace(AMP_SPAN[0], AMP_SPAN[1], 9)
    pts = st["dense_points"]
    eng = lagrange_rows(t, pts, np.transpose(sens[:, :, :, 0], (2, 0, 1)), sv)          # [time][obs][par]
    o = O(c)
    k = AMP_SLOTS.index("rd")
    sid = slot_of(c, "rd")
    p = c.dev_par[c.dev_names.index("rd")][0]
    y = []
    for rel in (1e-3, 5e-4):
        runs = []
        for sign in (+1, -1):
            o.set_param(sid, p * (1 + sign * rel))
            rc_o, _, vo, _, _ = o.tran(AMP_SPAN[0], AMP_SPAN[1], tran_opts(dc=dc_opts(abstol=1e-14), saveat=sv, **TIGHT))
            assert rc_o == 0
            runs.append(vo)
        y.append((runs[0] - runs[1]) / (2 * rel * p))
    r = (4 * y[1] - y[0]) / 3
    scale = np.max(np.abs(r))
    print("differenced transients, d/d rd: max|engine - r| / max|r| = %.3e, yardstick's own estimate max|y2 - r| / max|r| = %.3e"
          % (np.max(np.abs(eng[:, :, k].T - r)) / scale, np.max(np.abs(y[1] - r)) / scale))


# ---- 8. shape edges ----
@pytest.mark.parametrize("n", [1, 2, 96, 97])
def test_rc_ladders_at_the_shape_edges(E, O, n):
    c = rc_ladder(n)
    names = sorted({"rs1", "rs%d" % ((n + 1) // 2), "rs%d" % n}, key=lambda s: int(s[2:]))
    assert E(c).info()["n_unknowns"] == n
    # (the run's tolerances only choose the steps: the replay takes the same ones, and a linear circuit has no Newton error)
    span = 1e-10 * n * n if n > 2 else 2e-9
    (rc, t, v, xf, st, sens), x, s, worst = against_replay("ladder(%d)" % n, E, O, c, names, 0.0, span, dc_start=False, abstol=1e-8, reltol=1e-3)
    assert st["path"] == (1 if n <= 2 else 2)
    assert np.max(np.abs(sens)) > 0.0


def test_more_parameters_than_one_chunk_and_launch_accounting(E):
    """96 unknowns hold Kc = 97 columns beside the matrix: 100 multiplier slots (forward differences, one evaluation each) take two
    chunks, and their first 97 columns must be the bits of a 97-slot call.  Per point of the recursion (the start and every accepted
    step) there are 1 + n_forward + 2 n_central evaluation launches and ceil(K / Kc) solve launches."""
    n = 96
    c = rc_ladder(n)
    ids = [c.slot("rs%d" % i, "m") for i in range(1, n + 1)] + [c.slot("cp%d" % i, "m") for i in range(1, 5)]
    assert len(ids) == 100
    e = E(c)
    o = lambda: host(dc=dc_opts(x0=np.zeros((1, c.n_mna))), skip_dc=True, abstol=1e-8, reltol=1e-3)   # noqa: E731
    rc0, t0, v0, xf0, st0 = e.tran(0.0, 2e-7, o())
    rc, t, v, xf, st, s = e.tran_sens(0.0, 2e-7, ids, o())
    rc2, t2, v2, xf2, st2, s2 = e.tran_sens(0.0, 2e-7, ids[:97], o())
    assert rc0 == 0 and rc == 0 and rc2 == 0 and e.info()["path"] == 2 and np.array_equal(t0, t) and np.array_equal(v0, v)
    assert np.array_equal(s[:, :97], s2) and np.all(np.isfinite(s)) and np.any(s[:, 97:] != 0.0)
    points = st["naccept"] + 1
    # (an evaluation on the sparse path is 3 in the engine's launch counter: 2 for its residual pass, 1 for its commit)
    assert st["n_kernel_launches"] - st0["n_kernel_launches"] == points * (3 * (1 + 100) + 2)
    assert st2["n_kernel_launches"] - st0["n_kernel_launches"] == points * (3 * (1 + 97) + 1)
    # fused path, central and forward slots mixed: 2 unknowns, r (central), c (central), a multiplier (forward)
    c = rc_ladder(2)
    ids = [c.slot("rs1"), c.slot("cp2"), c.slot("rs2", "m")]
    e = E(c)
    o = lambda: host(dc=dc_opts(x0=np.zeros((1, c.n_mna))), skip_dc=True, abstol=1e-9, reltol=1e-5)   # noqa: E731
    rc0, _, _, _, st0 = e.tran(0.0, 2e-8, o())
    rc, _, _, _, st, s = e.tran_sens(0.0, 2e-8, ids, o())
    assert rc0 == 0 and rc == 0 and e.info()["path"] == 1
    assert st["n_kernel_launches"] - st0["n_kernel_launches"] == (st["naccept"] + 1) * ((1 + 2 * 2 + 1) + 1)


# ---- 9. batch ----
def test_circuit_sweep_of_three_points(E, O):
    def build(r1=1e3):
        c = Circuit()
        c.V("v", "in", 0, dc=0.2, tran=SIN(0.2, 1.0, 1e6))
        c.R("r1", "in", "out", r1)
        c.C("c1", "out", 0, 1e-10)
        return c

    span, names = (0.0, 5e-8), ["r1", "c1", ("v", 1)]
    r1s = [500.0, 1e3, 2e3]
    cs = CircuitSweep(build, Sweep(r1=r1s))
    sols = tran_sens(cs, names, span, **TIGHT, stepper="host")
    assert len(sols) == 3
    for sol, r1 in zip(sols, r1s):
        assert sol.rc == 0 and sol.params == {"r1": r1}
        c = build(r1)
        c.observe_all_nodes()
        ids = [slot_of(c, n) for n in names]
        rp = Replay(O(c), c, ids)
        xs, s0 = rp.dc_start()
        pts = sol.stats["dense_points"]
        x, s = rp.run(sol.t, np.maximum(pts - 1, 0), xs, s0)
        out = c.mna_index("v", "out")
        got = np.array([[sol.sens["node_out", nm] for nm in names]])
        compare("sweep r1 = %g" % r1, names, got, np.transpose(s[:, :, [out]], (2, 1, 0)))
    # The host stepper keeps ONE step sequence and error norm for the whole batch, so a sample has the bits of a single-sample call
    # where that sequence is its own: three samples at the base point, all from the same given start (a DC solve draws every
    # sample's start vector separately, and the operating points then differ in their last bits)
    c = build()
    c.observe_all_nodes()
    ids = [slot_of(c, n) for n in names]
    e1, e3 = E(c), E(c)
    e3.set_samples(3)
    e3.set_params(ids[:1], [[1e3, 1e3, 1e3]])
    a = e1.tran_sens(span[0], span[1], ids, host(dc=dc_opts(x0=np.zeros((1, c.n_mna))), skip_dc=True, **TIGHT))
    b = e3.tran_sens(span[0], span[1], ids, host(dc=dc_opts(x0=np.zeros((3, c.n_mna))), skip_dc=True, **TIGHT))
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2][:, :, 0], b[2][:, :, 1]) and np.array_equal(a[5][:, :, :, 0], b[5][:, :, :, 1])


def test_independent_blocks_do_not_see_each_other(E):
    c = Circuit()
    for k, f in ((1, 1e6), (2, 3e6)):
        c.V("v%d" % k, "in%d" % k, 0, dc=0.1, tran=SIN(0.1, 1.0, f))
        c.R("r%d" % k, "in%d" % k, "out%d" % k, 1e3)
        c.C("c%d" % k, "out%d" % k, 0, 1e-10 * k)
    c.observe_all_nodes()
    ids = [c.slot("r1"), c.slot("c2"), c.slot("v2", 1)]
    e = E(c)
    rc, t, v, xf, st, s = e.tran_sens(0.0, 3e-8, ids, host(**TIGHT))
    assert rc == 0 and e.info()["n_components"] == 2
    o1, o2 = c.obs.index(("v", c._n("out1"))), c.obs.index(("v", c._n("out2")))
    assert np.all(s[o2, 0] == 0.0) and np.all(s[o1, 1] == 0.0) and np.all(s[o1, 2] == 0.0)      # exactly zero across blocks
    assert np.any(s[o1, 0] != 0.0) and np.any(s[o2, 1] != 0.0) and np.any(s[o2, 2] != 0.0)


# ---- 10. compiled Verilog-A ----
def test_verilog_a_diode(E, O):
    c = Circuit(gmin=1e-12)
    c.V("v1", "in", 0, dc=0.9, tran=SIN(0.9, 0.3, 2e6))
    c.R("r1", "in", "a", 1e3)
    c.VA("d1", "va_diode", ["a", 0], {"IS": 1e-13, "RS": 2.0})
    c.C("c1", "a", 0, 1e-11)
    c.observe_all_nodes()
    names = [("d1", "is"), "r1", "temp"]
    (rc, t, v, xf, st, sens), x, s, worst = against_replay("va diode", E, O, c, names, 0.0, 3e-8)
    assert np.all(sens[c.obs.index(("v", c._n("a"))), 0, -1] < 0.0)


# ---- 11. errors are return codes ----
def test_errors_are_return_codes(E):
    c = Circuit()
    c.V("v", "in", 0, dc=0.0, tran=PULSE(0.0, 1.0, 1e-8, 1e-8, 1e-8, 5e-8))
    c.R("r1", "in", "out", 1e3)
    c.C("c1", "out", 0, 1e-11)
    c.observe_all_nodes()
    r1, amp, td = c.slot("r1"), c.slot("v", 1), c.slot("v", 2)
    e = E(c)

    def still_works():
        rc, t, v, xf, st = e.tran(0.0, 1e-7, host())
        assert rc == 0 and len(t) > 2

    for bad in ([7], [-1], [r1, 99]):
        rc, *_ = e.tran_sens(0.0, 1e-7, bad, host())
        assert rc == -1 and "slot" in e.ctx.last_error()
        still_works()
    r = ctypes.c_void_p()
    assert e.L.ch_tran_sens(e.h, 0.0, 1e-7, host(), 0, None, None, ctypes.byref(r)) == -1          # n_par = 0
    e.L.ch_result_free(r)
    still_works()
    rc, *_ = e.tran_sens(0.0, 1e-7, [r1], host(saveat=np.array([2e-8, 1e-8])))      # not a grid
    assert rc == -1 and "saveat" in e.ctx.last_error()
    still_works()
    rc, *_ = e.tran_sens(0.0, 1e-7, [r1, td], host())
    assert rc == -6 and "slot %d" % td in e.ctx.last_error() and "td" in e.ctx.last_error() and "break point" in e.ctx.last_error()
    still_works()
    rc, t, v, xf, st, s = e.tran_sens(0.0, 1e-7, [r1, amp], host())                  # levels are fine
    assert rc == 0 and np.all(np.isfinite(s)) and np.any(s[:, 1] != 0.0)
    with pytest.raises(CedarError, match="break point"):
        tran_sens(c, ["r1", ("v", 2)], (0.0, 1e-7))
    with pytest.raises(CedarError):
        tran_sens(c, ["nosuchdevice"], (0.0, 1e-7))
