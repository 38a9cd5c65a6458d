"""GPU tests of the waveform measurements end to end: `tran(..., measures=)` / `tran_sens(..., measures=)` on one circuit, on a
CircuitSweep and on the device stepper with its rows kept in HBM, `Solution.measure` after the fact, and `measures=None` leaving a
run as it was.

Two checks per run.  (1) What the engine measured equals the 40-digit yardstick (tests/measure_reference.py) applied to the rows and
sensitivity rows the run returned, under the rule max(1e-12, 32 e_cpu) of tests/measure_cases.py: the measurement layer adds no error
of its own.  (2) Against closed forms of an RC charging from a step (50 % at RC ln 2, 10 % to 90 % in RC ln 9, d/dR = C ln 2,
d/dC = R ln 2) the bound comes from the CPU oracle: its transient at the same tolerances through the yardstick, its error against the
closed form, times 10 because step sequences differ.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

import measure_cases as mc
import measure_reference as mr
from cedarsim_jl_amd import Circuit, CircuitSweep, PWL, Sweep, dc_opts, delay, event, find_at, avg, tran, tran_opts, tran_sens, vmin, when
from cedarsim_jl_amd.measure import EDGES, KINDS, resolve_measures
from cedarsim_jl_amd.workloads import dff_mc_builder, mc_tandem_sweep

pytestmark = pytest.mark.gpu
R1, C1 = 1e3, 1e-12
TOLS = dict(abstol=1e-9, reltol=1e-6)
MEASURES = [when("t50", "out", 0.5, "rise"), delay("t1090", event("out", 0.1, "rise"), event("out", 0.9, "rise"))]


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def rc_from_a_step(r=R1, cap=C1):
    """V = 1 behind R into C, started from v(out) = 0 (u0): v(out) = 1 - exp(-t / RC) exactly."""
    c = Circuit()
    c.V("v1", "in", 0, dc=1.0)
    c.R("r1", "in", "out", r)
    c.C("c1", "out", 0, cap)
    c.observe_node("out")
    u0 = np.zeros(c.n_mna)
    u0[c.mna_index("v", "in")] = 1.0
    return c, u0


def rc_behind_a_ramp(r1=R1):
    """The same RC behind a source that ramps to 1 in 1 ps (a sweep takes no u0): behind the ramp v(out) = 1 - K exp(-t / RC), and K
    cancels in the 10 % to 90 % time: RC ln 9."""
    c = Circuit()
    c.V("v1", "in", 0, tran=PWL([0.0, 0.0, 1e-12, 1.0, 1.0, 1.0]))
    c.R("r1", "in", "out", r1)
    c.C("c1", "out", 0, C1)
    c.observe_node("out")
    return c


def yardstick_specs(ckt, measures):
    """The measures as the yardstick's dicts, through the rows `resolve_measures` picks."""
    names, arr = resolve_measures(ckt, measures)
    inv = {v: k for k, v in EDGES.items()}
    side = lambda s: mr.side(s.row_a, s.row_b, s.scale, s.level, inv.get(s.edge, "cross"), s.count or 1, s.td)   # noqa: E731  (an unused second side is all zero)
    return names, [mr.spec(KINDS[a.kind], side(a.s1), side(a.s2), a.at, a.frm, a.to) for a in arr[:len(names)]]


def rows_of(sol):
    obs = sol.circuit.obs
    y = np.stack([np.asarray(sol._cols[o], float) for o in obs])
    s = np.stack([np.asarray(sol.sens._rows[o], float) for o in obs]) if hasattr(sol, "sens") else None
    pts = sol.stats.get("dense_points")
    return np.asarray(sol.t, float), (pts if pts is not None and len(pts) == len(sol.t) else None), y, s


def check_against_own_rows(what, sol, measures, sens_of=None):
    """Check (1): measures (and derivatives) of `sol` against the yardstick on sol's own rows."""
    t, pts, y, s = rows_of(sol)
    names, specs = yardstick_specs(sol.circuit, measures)
    for k, (name, sp) in enumerate(zip(names, specs)):
        r = mc.reference(sp, t, pts, y, s)
        assert sol.measure_status[name] == r["status"], (what, name, sol.measure_status[name], r["status"])
        ev = mr.errors([sol.measures[name]], [r["value"]], r["vs"])[0]
        es = max(mr.errors([float(x) for x in sens_of[k]], r["sens"], r["ss"])) if sens_of is not None else 0.0
        print("%s %s: scaled error against the yardstick on the run's own rows: value %.3e (allowed %.3e), derivative %.3e (allowed %.3e)" % (what, name, ev, r["tol_v"], es, r["tol_s"]))
        assert ev <= r["tol_v"] and es <= r["tol_s"], (what, name)


def oracle_error(O, ckt, u0, tspan, measures, closed):
    """Relative error per measure of the CPU oracle's transient (same tolerances) through the yardstick against the closed forms."""
    o = tran_opts(skip_dc=u0 is not None, dc=dc_opts(x0=u0), **TOLS) if u0 is not None else tran_opts(**TOLS)
    rc, t, v, _, _ = O(ckt).tran(tspan[0], tspan[1], o)
    assert rc == 0
    names, specs = yardstick_specs(ckt, measures)
    out = {}
    for name, sp in zip(names, specs):
        val, st, _ = mr.measure_mp(sp, t, None, v)
        assert st == 0
        out[name] = abs(float(val) - closed[name]) / closed[name]
    return out


def test_rc_delay_and_its_sensitivities(O):
    c, u0 = rc_from_a_step()
    tspan = (0.0, 5 * R1 * C1)
    sol = tran_sens(c, ["r1", "c1"], tspan, u0=u0, stepper="host", measures=MEASURES, **TOLS)
    assert sol.rc == 0 and sol.measure_status == {"t50": 0, "t1090": 0}
    check_against_own_rows("rc", sol, MEASURES, sol.measure_sens.array)
    closed = {"t50": R1 * C1 * math.log(2), "t1090": R1 * C1 * math.log(9)}
    c_or, _ = rc_from_a_step()
    e_or = oracle_error(O, c_or, u0, tspan, MEASURES, closed)
    for name, k in (("t50", math.log(2)), ("t1090", math.log(9))):
        bound = 10 * e_or[name]
        got = {"value": (sol.measures[name], closed[name]), "d/dR": (sol.measure_sens[name, "r1"], C1 * k), "d/dC": (sol.measure_sens[name, "c1"], R1 * k)}
        for what, (g, want) in got.items():
            err = abs(g - want) / want
            print("rc %s %s: %.9e, closed form %.9e, relative error %.3e; the oracle's own %.3e, allowed %.3e" % (name, what, g, want, err, e_or[name], bound))
            assert err <= bound, (name, what)
    # the same measures after the fact, on the solution's own rows and dense points: the bits of the run's (one sample: the same form)
    again = sol.measure(MEASURES)
    assert again.status == sol.measure_status
    assert all(mc.same_bits(again.values[n], sol.measures[n]) for n in again.values) and mc.same_bits(again.sens.array, sol.measure_sens.array)


def test_every_point_of_a_sweep_gets_its_own_delay(O):
    rs = [500.0, 1e3, 2e3]
    tspan = (0.0, 5 * rs[-1] * C1)
    m = [MEASURES[1]]
    sols = tran(CircuitSweep(rc_behind_a_ramp, Sweep(r1=rs)), tspan, stepper="host", measures=m, **TOLS)
    assert len(sols) == 3
    for sol, r in zip(sols, rs):
        assert sol.rc == 0 and sol.params == {"r1": r} and sol.measure_status == {"t1090": 0}
        check_against_own_rows("sweep r1 = %g" % r, sol, m)
        closed = {"t1090": r * C1 * math.log(9)}
        e_or = oracle_error(O, rc_behind_a_ramp(r), None, tspan, m, closed)["t1090"]
        err = abs(sol.measures["t1090"] - closed["t1090"]) / closed["t1090"]
        print("sweep r1 = %g: 10-90 %% %.9e, closed form %.9e, relative error %.3e; the oracle's own %.3e, allowed %.3e" % (r, sol.measures["t1090"], closed["t1090"], err, e_or, 10 * e_or))
        assert err <= 10 * e_or


def test_device_stepper_rows_are_measured_where_they_are(monkeypatch):
    """64 Monte-Carlo samples of one DFF on the device stepper, saveat grid, q observed: the rows stay in HBM (stats["device_rows"]) and
    ch_result_measure reads them there.  The flip-flop's state at t = 0 is whichever its operating point found; the first edge every
    sample shares is the capture of d = 1: the clock (clkn) falls through 2.5 V at 400.51 ns and q rises a few nanoseconds later.
    One kernel form for both calls (a batch of 64 takes lanes, a single solution the time split; the window sums of the two differ
    in their last bits by design)."""
    monkeypatch.setenv("CEDARHIP_MEASURE_SPLIT", "lanes")
    S, tspan, n_grid = 64, (0.0, 4.5e-7), 901
    measures = [when("tq", "q", 2.5, "rise", td=400e-9), vmin("qmin", "q", 300e-9), find_at("q405", "q", 405.3e-9), avg("qavg", "q", 390e-9, 420.2e-9),
                delay("rise", event("q", 0.5, "rise", td=400e-9), event("q", 4.5, "rise", td=400e-9)), when("never", "q", 9.0)]
    build, _ = dff_mc_builder()
    kw = dict(abstol=1e-5, reltol=1e-5, saveat=np.linspace(tspan[0], tspan[1], n_grid), stepper="device")
    sols = tran(CircuitSweep(build, mc_tandem_sweep(S)), tspan, measures=measures, **kw)
    assert len(sols) == S and all(s.rc == 0 for s in sols)
    st = sols[0].stats
    assert st["stepper"] == 2 and st["device_rows"] is not None and st["device_rows"].shape == (1, n_grid, S), "the rows must still be handed out in HBM"
    tq = np.array([s.measures["tq"] for s in sols])
    print("statuses of tq: %s" % sorted({s.measure_status["tq"] for s in sols}))
    assert all(s.measure_status["tq"] == 0 and s.measure_status["rise"] == 0 and s.measure_status["never"] == 1 and math.isnan(s.measures["never"]) for s in sols)
    print("clock-to-q over %d samples: %.4f ns .. %.4f ns behind the clock's 50 %% point" % (S, (tq.min() - 400.51e-9) * 1e9, (tq.max() - 400.51e-9) * 1e9))
    assert np.all(tq > 400.51e-9) and np.all(tq < 410e-9) and len(set(tq)) > S // 2
    for s in (0, 1, 31, 63):
        check_against_own_rows("dff sample %d" % s, sols[s], measures)
    for sol in sols:
        again = sol.measure(measures)
        assert again.status == sol.measure_status
        assert all(mc.same_bits(again.values[n], sol.measures[n]) for n in again.values), "Solution.measure on the copied rows differs from the run's own measures"


def test_measures_none_is_the_run_it_was():
    c, u0 = rc_from_a_step()
    a = tran(c, (0.0, 3e-9), u0=u0, **TOLS)
    c2, _ = rc_from_a_step()
    b = tran(c2, (0.0, 3e-9), u0=u0, measures=MEASURES, **TOLS)
    assert a.measures == {} and a.measure_status == {} and set(b.measures) == {"t50", "t1090"} and "measures" not in b.stats
    assert mc.same_bits(a.t, b.t) and mc.same_bits(a["out"], b["out"]) and mc.same_bits(a.x_final, b.x_final) and a.rc == b.rc == 0
    build, _ = dff_mc_builder()
    kw = dict(abstol=1e-5, reltol=1e-5, saveat=np.linspace(0.0, 6e-8, 61), stepper="device")
    d0 = tran(build(), (0.0, 6e-8), **kw)
    d1 = tran(build(), (0.0, 6e-8), measures=[vmin("qmin", "q")], **kw)
    assert d0.stats["stepper"] == d1.stats["stepper"] == 2 and d1.measure_status == {"qmin": 0} and d1.measures["qmin"] == float(np.min(d1["q"]))
    assert mc.same_bits(d0.t, d1.t) and mc.same_bits(d0["q"], d1["q"]) and mc.same_bits(np.nan_to_num(d0.x_final), np.nan_to_num(d1.x_final))
    for k in ("naccept", "nreject", "nf", "n_kernel_launches"):
        assert d0.stats[k] == d1.stats[k], k
