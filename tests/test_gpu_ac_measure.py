"""GPU tests of ch_ac_measure end to end: the AC analysis measured where the solve leaves its result (ac_measure, CircuitSweep.ac_measure),
and the noise measures through ch_freq_measure_rows.

  RC low-pass     the -3 dB frequency with d/dR, d/dC against the 40-digit yardstick (tests/fmeasure_reference.py) applied to the rows
                  ch_ac_sens hands back for the same call, under the measure layer's rule max(1e-12, 32 e_cpu) (the gather and the path
                  through HBM are the definition), and against 1/(2 pi R C), -1/(2 pi R^2 C), -1/(2 pi R C^2) within 10 times the
                  yardstick's own discretisation error on the exact H on that grid (computed here); on the fused and on the forced
                  sparse path.
  the amplifier   of tests/test_gpu_ac_sens.py: unity-gain frequency, the phase there and the low-frequency gain with d/d(m1.w), d/d rd,
                  d/d temp against the yardstick on the ch_ac_sens rows; d/d rd against a Richardson central difference of whole
                  ac_measure calls, judged by that difference's own error estimate.
  a sweep, a sample without an operating point (status 5), n_par = 0 against n_par > 0 bit for bit, an invalid spec refused before any
  launch, and the integrated noise against NoiseSensSolution.integrated."""
import math

import mpmath
import numpy as np
import pytest

import fmeasure_cases as fc
import fmeasure_reference as fr
from cedarsim_jl_amd import (CircuitSweep, Sweep, ac_measure, bandwidth, db, dc_opts, fevent, ffind_at, ffind_when, finteg, noise, noise_sens, phase, re,
                             unity_gain_freq)
from cedarsim_jl_amd.acmeasure import mna_rows, resolve_fmeasures
from cedarsim_jl_amd.circuit import CedarError
from test_gpu_ac_noise import amp_circuit
from test_gpu_ac_sens import forced_sparse, rc_cell
from test_gpu_dc_sens import slot_of

pytestmark = pytest.mark.gpu
R1, C1 = 1.3e3, 2.2e-9
RC_F = 10.0 ** np.linspace(2.0, 7.0, 101)     # 20 points per decade around the pole at 55.6 kHz


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return lambda c: EngineCircuit(c, small_signal=True)


def yardstick_specs(c, measures):
    """The reference's spec dicts of `measures` over the MNA rows of `c` (what ch_ac_measure is handed, read back from the ctypes array)."""
    res = resolve_fmeasures(measures, mna_rows(c))
    out = []
    for k in range(len(res.names)):
        sp = res.specs[k]
        sides = [fr.side(sd.row_a, sd.row_b, sd.scale, fr.SIGS[sd.sig], sd.level, {1: "rise", 2: "fall", 3: "cross"}[sd.edge], sd.count, sd.fd, sd.ref_at) for sd in (sp.s1, sp.s2)]
        out.append(fr.spec(fr.KINDS[sp.kind], sides[0], sides[1], ("lin", "log")[sp.xscale], sp.at, sp.frm, sp.to))
    return res, out


def against_the_rows(what, e, c, ids, f, measures, o, S=1):
    """ch_ac_measure against the yardstick on the rows ch_ac_sens hands back for the same call: (value, status, sens) of the measure call."""
    res, specs = yardstick_specs(c, measures)
    rc, val, status, ds, sample_status, st = e.ac_measure(ids, f, res.specs, len(res.names), o)
    assert rc == 0 and not sample_status.any(), e.ctx.last_error()
    rc2, x, _, sens, _, _ = e.ac_sens(ids, f, o)
    assert rc2 == 0
    refs = []
    for s in range(S):
        H = np.ascontiguousarray(np.transpose(x[s]))                        # [n_mna][n_freq]
        dH = np.ascontiguousarray(np.transpose(sens[s], (2, 1, 0)))         # [n_mna][n_par][n_freq]
        H, dH = np.nan_to_num(H, nan=0.0), np.nan_to_num(dH, nan=0.0)       # (eliminated branch currents: no spec names them)
        refs.append(fc.references(specs, f, H, dH, limit=1e-9))
    fc.compare(what, specs, lambda s: refs[s], val, status, ds, len(ids))
    return val, status, ds, st


def rc_measures():
    return [bandwidth("bw", "b", ref_at=float(RC_F[0]))]


def test_rc_bandwidth_on_both_paths(E, monkeypatch):
    c = rc_cell(R1, C1)
    ids = [slot_of(c, "r1"), slot_of(c, "c1")]
    o = dc_opts(abstol=1e-12, x0=np.zeros((1, c.n_mna)))
    # the yardstick's own discretisation error on the exact H = 1 / (1 + j f / fc) on this grid, for the value and both derivatives
    with mpmath.workdps(40):
        R, Cc, two_pi = mpmath.mpf(R1), mpmath.mpf(C1), 2 * mpmath.pi
        fcut = 1 / (two_pi * R * Cc)
        H = [[1 / (1 + 1j * mpmath.mpf(float(x)) / fcut) for x in RC_F]]
        dH = [[[-1j * two_pi * mpmath.mpf(float(x)) * Cc * h * h for x, h in zip(RC_F, H[0])], [-1j * two_pi * mpmath.mpf(float(x)) * R * h * h for x, h in zip(RC_F, H[0])]]]
        sp = fr.spec("when", fr.side(0, sig="db", level=-3.0103, edge="fall", fd=float(RC_F[0]), ref_at=float(RC_F[0])))
        v, st, d = fr.measure_mp([float(x) for x in RC_F], H, dH, sp)
        closed = [fcut, -fcut / R, -fcut / Cc]
        assert st == 0
        disc = [float(abs(a - b)) for a, b in zip([v] + d, closed)]
        closed = [float(x) for x in closed]
    print("discretisation error of the yardstick on the exact H: value %.3e Hz (%.2e of fc), d/dR %.3e, d/dC %.3e" % (disc[0], disc[0] / closed[0], disc[1], disc[2]))

    def check(what):
        e = E(c)
        val, status, ds, st = against_the_rows(what, e, c, ids, RC_F, rc_measures(), o)
        got = [val[0, 0], ds[0, 0, 0], ds[0, 1, 0]]
        print(what, "bandwidth %.9e Hz (1/(2 pi R C) = %.9e), d/dR %.9e (%.9e), d/dC %.9e (%.9e)" % (got[0], closed[0], got[1], closed[1], got[2], closed[2]))
        for g, cl, dd in zip(got, closed, disc):
            assert abs(g - cl) <= 10.0 * dd, (what, g, cl, dd)
        return e.info()["path"]

    assert check("RC, fused") == 1
    assert forced_sparse(monkeypatch, lambda: check("RC, sparse")) == 2


AMP_PARAMS = [("m1", "w"), "rd", "temp"]
AMP_F = 10.0 ** np.linspace(2.0, 9.0, 71)


def amp_measures():
    ug = fevent(db("o"), 0.0, "fall")
    return [unity_gain_freq("fug", "o"), ffind_when("ph", phase("o"), ug), ffind_at("a0", db("o"), 1e4)]


def test_amplifier_measures_against_the_yardstick_on_the_ac_sens_rows(E):
    c = amp_circuit()
    ids = [slot_of(c, p) for p in AMP_PARAMS]
    e = E(c)
    val, status, ds, st = against_the_rows("amplifier", e, c, ids, AMP_F, amp_measures(), dc_opts(abstol=1e-12))
    print("amplifier: unity gain at %.6e Hz, phase there %.4f deg, gain at 10 kHz %.4f dB" % tuple(val[:, 0]))
    assert np.all(status == 0) and np.all(np.isfinite(ds))


def test_amplifier_d_rd_against_a_richardson_difference_of_whole_calls():
    """d(measure)/d rd from central differences of two pairs of whole ac_measure calls at relative steps h and 2h, extrapolated:
    r = (4 D(h) - D(2h)) / 3, whose own error estimate is |D(h) - D(2h)| / 3 (the correction it applies).  On top of that, ch_ac_sens's
    derivatives are pinned to 1e-6 of a row's largest entry by its own tests and the event's division by the slope may cost an order:
    the floor is 1e-5 of the derivative's scale."""
    measures = amp_measures()

    def at(rd):
        c = amp_circuit()
        c.dev_par[c.dev_names.index("rd")][0] = rd
        sol = ac_measure(c, measures, AMP_F, abstol=1e-13)
        assert all(v == 0 for v in sol.measure_status.values())
        return np.array([sol.measures[m.name] for m in measures])

    c = amp_circuit()
    rd = float(c.dev_par[c.dev_names.index("rd")][0])
    sol = ac_measure(c, measures, AMP_F, params=["rd"], abstol=1e-13)
    h = 1e-3
    d1 = (at(rd * (1 + h)) - at(rd * (1 - h))) / (2 * h * rd)
    d2 = (at(rd * (1 + 2 * h)) - at(rd * (1 - 2 * h))) / (4 * h * rd)
    r, est = (4 * d1 - d2) / 3, np.abs(d1 - d2) / 3
    for k, m in enumerate(measures):
        got = sol.measure_sens[m.name, "rd"]
        print("%s: d/d rd %.9e, Richardson %.9e, its estimate %.2e, difference %.2e" % (m.name, got, r[k], est[k], abs(got - r[k])))
        assert abs(got - r[k]) <= est[k] + 1e-5 * abs(r[k]), (m.name, got, r[k], est[k])


def test_a_three_point_sweep_equals_its_single_calls():
    rs = [500.0, 1.3e3, 4e3]
    cs = CircuitSweep(lambda r1=1e3: rc_cell(r1, C1), Sweep(r1=rs))
    ms = rc_measures() + [ffind_at("g5", db("b"), 1e5), ffind_at("p5", phase("b"), 1e5)]
    sols = cs.ac_measure(ms, RC_F, params=["r1", "c1"], abstol=1e-12)
    assert len(sols) == 3
    for sol, p in zip(sols, cs):
        one = ac_measure(rc_cell(p["r1"], C1), ms, RC_F, params=["r1", "c1"], abstol=1e-12)
        assert sol.params == p and sol.rc == 0
        for m in ms:
            assert sol.measure_status[m.name] == one.measure_status[m.name] == 0
            assert math.isclose(sol.measures[m.name], one.measures[m.name], rel_tol=1e-12)
            for par in ("r1", "c1"):
                assert math.isclose(sol.measure_sens[m.name, par], one.measure_sens[m.name, par], rel_tol=1e-9, abs_tol=1e-300)
        assert abs(sol.measures["bw"] - 1.0 / (2 * math.pi * p["r1"] * C1)) < 2e-3 / (2 * math.pi * p["r1"] * C1)


def test_a_sample_without_an_operating_point_has_status_5_and_the_others_are_served(E):
    c = rc_cell()
    c.I("i1", "n", 0, dc=1e-3)
    c.R("rn", "n", 0, 1e3)
    names = ["rn", "r1", "c1"]
    ids = [slot_of(c, nm) for nm in names]
    res = resolve_fmeasures(rc_measures() + [ffind_at("g", db("b"), 1e5)], mna_rows(c))
    o = dict(abstol=1e-12, n_restarts=2, maxiters=5)
    e = E(c)
    e.set_samples(2)
    e.set_params(ids[:1], [[1e3, math.inf]])
    rc, val, status, ds, sample_status, st = e.ac_measure(ids, RC_F, res.specs, 2, dc_opts(**o))
    assert rc == -3 and sample_status[0] == 0 and sample_status[1] != 0
    assert np.all(status[:, 1] == 5) and np.isnan(val[:, 1]).all() and np.isnan(ds[:, :, 1]).all()
    assert np.all(status[:, 0] == 0) and np.isfinite(val[:, 0]).all()
    e1 = E(c)
    rc1, val1, status1, ds1, _, _ = e1.ac_measure(ids, RC_F, res.specs, 2, dc_opts(**o))
    assert rc1 == 0 and fc.same_bits(val1[:, 0], val[:, 0]) and fc.same_bits(ds1[:, :, 0], ds[:, :, 0])


def test_without_parameters_the_values_are_those_of_the_call_with_parameters(E):
    c = amp_circuit()
    ids = [slot_of(c, p) for p in AMP_PARAMS]
    res = resolve_fmeasures(amp_measures(), mna_rows(c))
    e = E(c)
    o = dc_opts(abstol=1e-12)
    rc0, val0, status0, ds0, ss0, st0 = e.ac_measure([], AMP_F, res.specs, len(res.names), o)
    rc1, val1, status1, ds1, ss1, st1 = e.ac_measure(ids, AMP_F, res.specs, len(res.names), o)
    assert rc0 == 0 and rc1 == 0 and ds0 is None and not ss0.any()
    assert fc.same_bits(val0, val1) and np.array_equal(status0, status1) and np.all(status0 == 0)
    assert st0["n_kernel_launches"] < st1["n_kernel_launches"]


def test_an_invalid_spec_is_refused_with_its_index_before_any_launch(E):
    c = rc_cell()
    ids = [slot_of(c, "r1")]
    good = rc_measures()[0]
    res = resolve_fmeasures([good, good._replace(name="bw2")], mna_rows(c))
    e = E(c)
    o = dc_opts(abstol=1e-12)
    res.specs[1].s1.row_a = c.n_mna                  # a row out of range
    rc, val, status, ds, ss, st = e.ac_measure(ids, RC_F, res.specs, 2, o)
    assert rc == -1 and "measure 1" in e.ctx.last_error() and "row out of range" in e.ctx.last_error() and st["n_kernel_launches"] == 0
    res.specs[1].s1.row_a = 0
    res.specs[0].s1.count = 0
    rc, *_ , st = e.ac_measure([], RC_F, res.specs, 2, o)
    assert rc == -1 and "measure 0" in e.ctx.last_error() and st["n_kernel_launches"] == 0
    res.specs[0].s1.count = 1
    g = RC_F.copy()
    g[5] = g[4]
    assert e.ac_measure(ids, g, res.specs, 2, o)[0] == -1 and "strictly increasing" in e.ctx.last_error()
    assert e.ac_measure(ids, RC_F, res.specs, 2, o)[0] == 0
    with pytest.raises(CedarError, match="unknown node"):
        ac_measure(c, [bandwidth("bw", "nosuchnode", 1e2)], RC_F)
    with pytest.raises(CedarError, match="defined twice"):
        ac_measure(c, [good, good], RC_F)


def test_integrated_noise_is_the_solutions_own_trapezoid_sum():
    """finteg of the PSD row over the whole grid is the trapezoid rule in Hz over the same rows as NoiseSensSolution.integrated: equal
    to rounding — 100 terms, each product and sum rounded once: within 1e-13 of the sum of the terms' magnitudes."""
    c = rc_cell(R1, C1)
    w = 2.0 * math.pi * RC_F
    ns = noise_sens(c, ["r1", "c1"], abstol=1e-12)
    m = ns.measure([finteg("vn2", re("b"))], w)
    assert m.status["vn2"] == 0
    psd = ns.psd("b", w)
    mass = float(np.sum(0.5 * (np.abs(psd[1:]) + np.abs(psd[:-1])) * np.diff(RC_F)))
    assert abs(m.values["vn2"] - ns.integrated("b", w)) <= 1e-13 * mass
    for par in ("r1", "c1"):
        d = ns.sens("b", par, w)
        mass = float(np.sum(0.5 * (np.abs(d[1:]) + np.abs(d[:-1])) * np.diff(RC_F)))
        assert abs(m.sens["vn2", par] - ns.integrated_sens("b", par, w)) <= 1e-13 * mass, par
    plain = noise(rc_cell(R1, C1), abstol=1e-12).measure([finteg("vn2", re("b"), frm=1e3, to=1e6), ffind_at("spot", re("b"), 1e4)], w)
    assert plain.status == {"vn2": 0, "spot": 0} and plain.sens is None and 0.0 < plain.values["vn2"] < ns.integrated("b", w)
