"""GPU tests of the loop-gain (stability) analysis: loop_gain / ch_loop_gain, its sensitivities and its measures.

Linear loops against the CPU yardstick of loopgain_reference.py (numpy stamps, every solve refined at 40 digits, pinned by
test_loopgain_reference.py) at the shape edges of loopgain_solve_kernel: 4 unknowns (the bare loop), 64, 96 (the LDS limit) and 97 (the
global workspace, on the forced sparse path).  The error of T is |T - T_ref| / max(1, max|T_ref|) under smallsignal_cases.tolerance(e_cpu)
= max(1e-12, 32 e_cpu), e_cpu the same error of T formed from plain LAPACK solves; a case with e_cpu > 1e-11 is refused.  The same
tolerance holds T against T formed in numpy from two existing ac() runs (the probe at |ac| = 1; an explicit `I 0 x ac=1`), which also
pins the sign of the current-injection right-hand side.  dT/dp: against the yardstick's analytic values under
acsens_reference.tolerance(e_cpu), e_cpu the error of the engine's method in numpy (loopgain_reference.fd_loop_gain_sens); errors are
relative, per frequency and parameter (loopgain_reference.sens_errors).
A BSIM4 amplifier in feedback through the probe: T against two ac() runs, dT/dp against Richardson central differences of that two-run
T (the existing AC kernels, never loop_gain itself) at the steps and under the admission and tolerance test_gpu_ac_sens.py grants its
amplifier: steps 2e-5 / 1e-5, own estimate <= 1e-7, tolerance 1e-6.
Measures on "T", a sweep, a sample without an operating point, and the refusals."""
import copy
import math

import numpy as np
import pytest

import acsens_reference as AR
import fmeasure_cases as fc
import fmeasure_reference as fr
import loopgain_reference as LG
import smallsignal_cases as cases
from cedarsim_jl_amd import (Circuit, CircuitSweep, Sweep, acdec, dc_opts, gain_margin, loop_gain, phase_margin, unity_gain_freq)
from cedarsim_jl_amd.acmeasure import resolve_fmeasures
from cedarsim_jl_amd.batch import _loop_gain_rows
from cedarsim_jl_amd.circuit import CedarError

from test_gpu_ac_noise import gf180_models

pytestmark = pytest.mark.gpu
PROBE = LG.PROBE
SIZES = [4, 64, 96, 97]
F3 = np.array([0.0, 1e6, 1e10])


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return lambda c: EngineCircuit(c, small_signal=True)


def opts(c, samples=1):
    """abstol 1e-12 and a zero start: a linear circuit is solved by one Newton step, the same for every sample index."""
    return dc_opts(abstol=1e-12, x0=np.zeros((samples, c.n_mna)))


def forced_sparse(monkeypatch, fn):
    monkeypatch.setenv("CEDARHIP_FORCE_SPARSE", "1")
    try:
        return fn()
    finally:
        monkeypatch.delenv("CEDARHIP_FORCE_SPARSE", raising=False)


def dev(c, name=PROBE):
    return c.dev_names.index(name)


def run_T(E, c, freqs, o=None):
    e = E(c)
    rc, T, _, _, _, _, status, st = e.loop_gain(dev(c), freqs, opts=o or opts(c))
    assert rc == 0 and not status.any(), e.ctx.last_error()
    return T[0], e.info()


# ---- shape edges ----
@pytest.mark.parametrize("n", SIZES)
def test_T_at_every_shape_edge(E, monkeypatch, n):
    """Measured on the MI355X (e_cpu / GPU error, tolerance 1e-12 each): 4 unknowns 1.1e-15 / 7.8e-16, 64: 3.3e-15 / 6.9e-15,
    96: 2.9e-15 / 4.5e-16, 97: 4.9e-15 / 1.9e-15 (the table of DESIGN.md 2.7i)."""
    c, T_ref, e_cpu, tol = LG.shape_case(n)
    if n == 97:
        T, info = forced_sparse(monkeypatch, lambda: run_T(E, c, cases.FREQS))
        assert info["path"] == 2
    else:
        T, info = run_T(E, c, cases.FREQS)
        assert info["path"] == (1 if n <= 64 else 2)
    assert info["n_unknowns"] == n and info["n_components"] == 1
    err = LG.errors(T, T_ref)
    print("loop(%d): e_cpu %.2e, GPU error %.2e, tolerance %.2e" % (n, e_cpu, err, tol))
    assert not np.isnan(T).any() and err <= tol, (n, err, tol)
    if n == 4:   # the same LDS kernel, G and C arriving through the sparse path's dense expansion
        T2, info2 = forced_sparse(monkeypatch, lambda: run_T(E, c, cases.FREQS))
        assert info2["path"] == 2 and LG.errors(T2, T_ref) <= tol
        assert abs(T[0] - 2.0) <= tol                       # the DC loop gain of the bare loop
        Tr, _ = run_T(E, LG.loop(reverse=True), cases.FREQS[:1])
        assert abs(Tr[0] + 0.4) <= tol                      # the reversed probe: the reverse loop gain


# ---- agreement with the family ----
def two_run_T(E, c, freqs, o=None, engines=None):
    """T and u formed in numpy from two ac() runs: the probe at |ac| = 1, and the probe at 0 V with an explicit `I 0 x ac=1` (its
    branch current observed, so that it stays an unknown).  engines: reuse (e_v, e_i, rx, ri)."""
    if engines is None:
        cv = copy.deepcopy(c)
        ci = copy.deepcopy(c)
        x = c.dev_node[dev(c)][0]
        ci.source_ac = [0.0] * len(ci.source_ac)
        ci.I("iinj_x", 0, x, dc=0.0, ac=1.0)
        ci.observe_branch(PROBE)
        engines = (E(cv), E(ci), x - 1, c.mna_index("i", PROBE))
    ev, ei, rx, ri = engines
    rc1, xv, _ = ev.ac(freqs, o or opts(c))
    rc2, xi, _ = ei.ac(freqs, o or opts(c))
    assert rc1 == 0 and rc2 == 0, (ev.ctx.last_error(), ei.ctx.last_error())
    u = xv[0][:, rx] - xi[0][:, ri]
    return u / (1.0 - u), u, engines


@pytest.mark.parametrize("n", [4, 96])
def test_T_agrees_with_two_ac_runs(E, n):
    c, T_ref, e_cpu, tol = LG.shape_case(n)
    T, _ = run_T(E, c, cases.FREQS)
    T2, u2, _ = two_run_T(E, c, cases.FREQS)
    u = T / (1.0 + T)
    eT, eu = LG.errors(T, T2), LG.errors(u, u2)
    print("loop(%d) against two ac() runs: T %.2e, u = V2 - I1 %.2e, tolerance %.2e" % (n, eT, eu, tol))
    assert eT <= tol and eu <= tol
    assert LG.errors(T2, T_ref) <= tol      # (the two-run T is itself within the tolerance of the yardstick: the sign of b_i is the ac() family's)


# ---- sensitivities, linear ----
def sens_names(c, n):
    names = ["r1", "r2", "ro", "co", "cg", "gm"]
    if n > 4:
        tail = [nm for nm in c.dev_names if nm.startswith("t") and not nm.startswith("trt")]
        names += [tail[int(round(j))] for j in np.linspace(0, len(tail) - 1, 6)]
    return names


_SENS = {}


def sens_case(n):
    if n not in _SENS:
        c = LG.loop(n - 4)
        names = sens_names(c, n)
        ids = [c.slot(nm) for nm in names]
        slots = [c.slots[i] for i in ids]
        T, dT, _ = LG.loop_gain(c, F3, slots=slots)
        e_cpu = float(LG.sens_errors(LG.fd_loop_gain_sens(c, F3, slots), dT).max())
        _SENS[n] = (c, names, ids, T, dT, e_cpu, AR.tolerance(e_cpu))
    return _SENS[n]


@pytest.mark.parametrize("n", [4, 96, 97])
def test_linear_sensitivities(E, monkeypatch, n):
    c, names, ids, T_ref, dT_ref, e_cpu, tol = sens_case(n)

    def run():
        e = E(c)
        rc, T, dT, _, _, _, status, st = e.loop_gain(dev(c), F3, ids, opts=opts(c))
        assert rc == 0 and not status.any(), e.ctx.last_error()
        # chunked and single-parameter calls: the same bits
        half = len(ids) // 2
        parts = [e.loop_gain(dev(c), F3, ids[:half], opts=opts(c))[2], e.loop_gain(dev(c), F3, ids[half:], opts=opts(c))[2]]
        assert np.array_equal(np.ascontiguousarray(np.concatenate(parts, axis=2)).view(np.float64), dT.view(np.float64))
        for k in (0, len(ids) - 1):
            one = e.loop_gain(dev(c), F3, ids[k:k + 1], opts=opts(c))[2]
            assert np.array_equal(np.ascontiguousarray(one[:, :, 0]).view(np.float64), np.ascontiguousarray(dT[:, :, k]).view(np.float64))
        rc0, T0 = e.loop_gain(dev(c), F3, opts=opts(c))[:2]
        assert rc0 == 0 and np.array_equal(T0.view(np.float64), T.view(np.float64))     # T does not depend on the parameters asked for
        return T[0], dT[0], e.info()

    T, dT, info = forced_sparse(monkeypatch, run) if n == 97 else run()
    assert info["n_unknowns"] == n
    err = LG.sens_errors(dT, dT_ref)
    print("loop(%d) dT/dp: e_cpu %.2e, tolerance %.2e; GPU errors (worst frequency) %s; at %g Hz alone %.1e" % (
        n, e_cpu, tol, ", ".join("%s %.1e" % (nm, x) for nm, x in zip(names, err.max(axis=0))), F3[-1], err[-1].max()))
    assert LG.errors(T, T_ref) <= cases.tolerance(LG.shape_case(n)[2])
    assert not np.isnan(dT).any() and err.max() <= tol, (names[int(np.argmax(err.max(axis=0)))], err.max(), tol)


# ---- sensitivities, MOSFET ----
AMP_PARAMS = ["rd", ("m1", "w"), "temp"]
AMP_FREQS = np.array([1e2, 1e4, 1e6, 1e7, 1e8])
STEPS = (2e-5, 1e-5)
TOL, ADMIT = 1e-6, 1e-7


def feedback_amp():
    """The amplifier of test_gpu_ac_noise.amp_circuit (its cards, its bias) with its AC input taken from its own output: the probe o -> in
    closes the loop through the coupling capacitor, which keeps the bias where the open amplifier has it."""
    c = Circuit(gmin=1e-12)
    c.temp = 40.0
    m = gf180_models()
    n = c.add_model(*m["nfet_06v0"])
    p = c.add_model(*m["pfet_06v0"])
    c.V("vdd", "vdd", 0, dc=5.0)
    c.V(PROBE, "o", "in", dc=0.0, ac=1.0)
    c.C("cin", "in", "g", 1e-9)
    c.R("rb1", "vdd", "g", 300e3, m=2.0)
    c.R("rb2", "g", 0, 100e3)
    c.M("m1", "d", "g", "s", 0, n, 2e-6, 6e-7)
    c.R("rd", "vdd", "d", 20e3)
    c.R("rs", "s", 0, 1e3)
    c.C("cs", "s", 0, 1e-9)
    c.M("m2", "o", "d", "vdd", "vdd", p, 4e-6, 5e-7)
    c.R("ro", "o", 0, 50e3)
    c.C("co", "o", 0, 1e-12)
    return c


def slot_of(c, name):
    return c.slot(*name) if isinstance(name, tuple) else c.slot(name)


def base_value(c, slot):
    kind, a, b = c.slots[slot]
    return c.temp if kind == 5 else c.dev_par[a][b]


def test_mosfet_amplifier_against_differences_of_two_run_T(E):
    """Measured on the MI355X: T against the two runs 1.8e-16 (bound 1e-12); the yardstick's own estimates rd 4.8e-08, m1.w 3.1e-08, temp 2.4e-09;
    errors of dT/dp: rd 1.3e-09 .. 1.6e-09, m1.w 1.1e-09 .. 1.1e-08, temp 1.0e-09 .. 5.5e-08.  With the state term dropped (a local
    edit, checked once) d/d rd is off by 1.0 .. 1.2 times the yardstick: this test is what proves the bias shift is there."""
    c = feedback_amp()
    ids = [slot_of(c, nm) for nm in AMP_PARAMS]
    o = dc_opts(abstol=1e-13)
    e = E(c)
    rc, T, dT, _, _, _, status, st = e.loop_gain(dev(c), AMP_FREQS, ids, opts=o)
    assert rc == 0 and not status.any(), e.ctx.last_error()
    T, dT = T[0], dT[0]
    T2, _, engines = two_run_T(E, c, AMP_FREQS, o)
    eT = LG.errors(T, T2)
    print("amplifier: T against two ac() runs %.2e; |T| = %s" % (eT, " ".join("%.3g" % abs(t) for t in T)))
    # the project's rule; there is no CPU yardstick for a BSIM4 circuit, so e_cpu = 0 and the bound is the rule's floor, 1e-12: the
    # three engines solve the same operating point from the same start with the same seed, and G, C are the same dumps
    assert eT <= cases.tolerance(0.0)
    for k, nm in enumerate(AMP_PARAMS):
        p = base_value(c, ids[k])
        y = []
        for rel in STEPS:
            h = rel * abs(p)
            pair = []
            for sign in (+1, -1):
                for eng in engines[:2]:
                    eng.set_params([ids[k]], [[p + sign * h]])
                pair.append(two_run_T(E, c, AMP_FREQS, o, engines)[0])
            y.append((pair[0] - pair[1]) / (2.0 * h))
        for eng in engines[:2]:
            eng.set_params([ids[k]], [[p]])
        r = (4.0 * y[1] - y[0]) / 3.0
        est = np.abs(y[1] - r) / np.abs(r)
        err = np.abs(dT[:, k] - r) / np.abs(r)
        print("amplifier d/d%s: yardstick's own estimate %.1e, GPU error %s" % (nm, est.max(), " ".join("%.1e" % x for x in err)))
        assert est.max() <= ADMIT, "slot %r refused: the yardstick's own estimate is %.2e" % (nm, est.max())
        assert err.max() <= TOL, (nm, err)


# ---- measures ----
MEAS_F = acdec(10, 1e5, 1e10)
MEAS_PARAMS = ["r2", "cg", "gm", ("cg", "m")]


def loop_measures():
    return [unity_gain_freq("fug", "T"), phase_margin("pm", "T"), gain_margin("gm_db", "T")]


def yardstick_specs(measures):
    res = resolve_fmeasures(measures, _loop_gain_rows)
    out = []
    for k in range(len(res.names)):
        sp = res.specs[k]
        sides = [fr.side(sd.row_a, sd.row_b, sd.scale, fr.SIGS[sd.sig], sd.level, {1: "rise", 2: "fall", 3: "cross"}[sd.edge], sd.count, sd.fd, sd.ref_at) for sd in (sp.s1, sp.s2)]
        out.append(fr.spec(fr.KINDS[sp.kind], sides[0], sides[1], ("lin", "log")[sp.xscale], sp.at, sp.frm, sp.to))
    return res, out


def test_measures_on_T_with_their_sensitivities(E):
    """unity_gain_freq, phase_margin and gain_margin of the three-pole loop (DC loop gain 30) with d/d r2, d/d cg, d/d gm and d/d (cg's
    multiplier), under the rule of the ch_ac_measure tests (fmeasure_cases.compare: max(1e-12, 32 e_cpu) of the measure's scale,
    statuses exactly): the measure kernel against the 40-digit yardstick (fmeasure_reference.measure_mp) on the rows the same call
    hands back — the path through HBM is the definition — and the values, with the derivative in cg's multiplier, against the
    yardstick fed the rows of loopgain_reference.  That slot's difference is exact (the stamp is linear in it, the step 1), so its
    rows carry no truncation error of a central difference (5.8e-11 for r2, above the rule's floor); gm's is exact as well, but
    dT/dgm = T/gm leaves the phase where it is, and the rule has no scale for a derivative that is identically zero.
    Independently of the call's own rows: the dT rows of all four slots against dT_ref under acsens_reference.tolerance(e_cpu), and
    every measure's derivative in r2, cg, gm and cg's multiplier against the yardstick fed the reference rows, relative to the
    yardstick's figure, under acsens_reference.tolerance(e_cpu) with e_cpu measured on the CPU for that measure (at most 5.5e-11:
    tolerance 1.8e-09)."""
    c = LG.loop(three_pole=True)
    ids = [slot_of(c, nm) for nm in MEAS_PARAMS]
    res, specs = yardstick_specs(loop_measures())
    e = E(c)
    rc, T, dT, val, status, ds, sample_status, st = e.loop_gain(dev(c), MEAS_F, ids, res.specs, len(res.names), opts(c))
    assert rc == 0 and not sample_status.any() and np.all(status == 0), (e.ctx.last_error(), status)
    H = np.ascontiguousarray(T[0][None, :])                                    # [1 row][n_freq]
    dH = np.ascontiguousarray(np.transpose(dT[0])[None, :, :])                 # [1 row][n_par][n_freq]
    own = fc.references(specs, MEAS_F, H, dH, limit=1e-9)
    fc.compare("loop gain, own rows", specs, lambda s: own, val, status, ds, len(ids))
    slots = [c.slots[i] for i in ids]
    T_ref, dT_ref, T_l = LG.loop_gain(c, MEAS_F, slots=slots)
    dT_fd = LG.fd_loop_gain_sens(c, MEAS_F, slots)
    e_rows = float(LG.sens_errors(dT_fd, dT_ref).max())
    err_rows = LG.sens_errors(dT[0], dT_ref)
    print("three-pole loop rows: T %.2e; dT/dp e_cpu %.2e, tolerance %.2e, GPU %s" % (
        LG.errors(T[0], T_ref), e_rows, AR.tolerance(e_rows), " ".join("%.1e" % x for x in err_rows.max(axis=0))))
    assert LG.errors(T[0], T_ref) <= cases.tolerance(LG.errors(T_l, T_ref))
    assert err_rows.max() <= AR.tolerance(e_rows)
    # values and every derivative against the yardstick fed the reference rows.  Values, and the derivative in cg's multiplier, under
    # the rule of fmeasure_cases.compare; every derivative also relative to the yardstick's own figure under
    # acsens_reference.tolerance(e_cpu), e_cpu the same error of the float64 measure on the rows of the method in numpy
    # (fd_loop_gain_sens, T from LAPACK): the rows of r2 and cg carry the truncation and rounding of a central difference.
    k_m = MEAS_PARAMS.index(("cg", "m"))
    H_ref, dH_ref = np.ascontiguousarray(T_ref[None, :]), np.ascontiguousarray(np.transpose(dT_ref)[None, :, :])
    want = fc.references(specs, MEAS_F, H_ref, np.ascontiguousarray(dH_ref[:, k_m:k_m + 1, :]), limit=1e-9)
    fc.compare("loop gain, reference rows", specs, lambda s: want, val, status, np.ascontiguousarray(ds[:, k_m:k_m + 1, :]), 1)
    H_l, dH_fd = np.ascontiguousarray(T_l[None, :]), np.ascontiguousarray(np.transpose(dT_fd)[None, :, :])
    for k, sp in enumerate(specs):
        vm, stm, dm = fr.measure_mp(MEAS_F, H_ref, dH_ref, sp)
        vf, stf, df = fr.measure_f64(MEAS_F, H_l, dH_fd, sp)
        assert stm == 0 and stf == 0
        dm = np.array([float(x) for x in dm])
        e_cpu = float(np.max(np.abs(np.array([float(x) for x in df]) - dm) / np.abs(dm)))
        err = np.abs(ds[k, :, 0] - dm) / np.abs(dm)
        print("%s: d/d(r2, cg, gm, cg.m) against the reference rows: e_cpu %.2e, tolerance %.2e, GPU %s" % (
            res.names[k], e_cpu, AR.tolerance(e_cpu), " ".join("%.1e" % x for x in err)))
        assert err.max() <= AR.tolerance(e_cpu), (res.names[k], err)
    v2, d2 = res.apply(val.copy(), ds.copy())
    print("three-pole loop: unity gain at %.6e Hz, phase margin %.4f deg, gain margin %.4f dB; d(pm)/d(r2, cg, gm, cg.m) = %s" % (
        v2[0, 0], v2[1, 0], v2[2, 0], " ".join("%.4e" % x for x in d2[1, :, 0])))
    # the public surface hands out the same figures
    sol = loop_gain(c, PROBE, MEAS_F, params=MEAS_PARAMS, measures=loop_measures(), abstol=1e-12)
    assert sol.rc == 0 and sol.measure_status == {"fug": 0, "pm": 0, "gm_db": 0}
    assert math.isclose(sol.measures["pm"], v2[1, 0], rel_tol=1e-9) and math.isclose(sol.measure_sens["pm", "cg"], d2[1, 1, 0], rel_tol=1e-6)
    assert np.allclose(sol.T, T[0], rtol=1e-9, atol=0.0) and np.allclose(sol.sens["r2"], dT[0][:, 0], rtol=1e-6, atol=0.0) and np.array_equal(sol.freqs, MEAS_F)
    with pytest.raises(CedarError, match="\"T\""):
        loop_gain(c, PROBE, MEAS_F, measures=[phase_margin("pm", "o")])


# ---- batch ----
def test_a_sweep_of_cg_and_a_sample_without_an_operating_point(E):
    cgs = [1e-13, 2e-13, 8e-13]
    f = cases.FREQS[2:6]

    def build(cg=LG.CG):
        c = LG.loop()
        c.dev_par[c.dev_names.index("cg")][0] = cg
        return c

    ms = [unity_gain_freq("fug", "T", xscale="lin")]
    sols = loop_gain(CircuitSweep(build, Sweep(cg=cgs)), PROBE, f, params=["r2", "cg"], measures=ms, abstol=1e-12)
    assert len(sols) == 3
    one = loop_gain(build(cgs[1]), PROBE, f, params=["r2", "cg"], measures=ms, abstol=1e-12)
    for sol, cg in zip(sols, cgs):
        slots = [(1, sol.circuit.dev_names.index("r2"), 0), (1, sol.circuit.dev_names.index("cg"), 0)]
        T_ref, dT_ref, T_l = LG.loop_gain(build(cg), f, slots=slots)
        e_cpu = float(LG.sens_errors(LG.fd_loop_gain_sens(build(cg), f, slots), dT_ref).max())
        assert sol.rc == 0 and sol.params == {"cg": cg} and LG.errors(sol.T, T_ref) <= cases.tolerance(LG.errors(T_l, T_ref))
        assert LG.sens_errors(sol.sens.array, dT_ref).max() <= AR.tolerance(e_cpu)
    # the sweep's point equals its own single call (the existing sweep tests' figure), and at the engine sample 1 of the batch has
    # the bits of a one-sample call
    assert np.allclose(sols[1].T, one.T, rtol=1e-12, atol=0.0) and np.allclose(sols[1].sens.array, one.sens.array, rtol=1e-12, atol=0.0)
    assert math.isclose(sols[1].measures["fug"], one.measures["fug"], rel_tol=1e-12) and sols[1].measure_status == one.measure_status
    cb = build()
    ids_b = [cb.slot("cg"), cb.slot("r2")]
    res_b = resolve_fmeasures(ms, _loop_gain_rows)
    eb = E(cb)
    eb.set_samples(3)
    eb.set_params(ids_b[:1], [cgs])
    rcb, Tb, dTb, vb, sb, dsb, stb, _ = eb.loop_gain(dev(cb), f, ids_b, res_b.specs, 1, opts(cb, 3))
    e1b = E(cb)
    e1b.set_params(ids_b[:1], [[cgs[1]]])
    rc1b, T1b, dT1b, v1b, s1b, ds1b, _, _ = e1b.loop_gain(dev(cb), f, ids_b, res_b.specs, 1, opts(cb))
    assert rcb == 0 and rc1b == 0 and not stb.any()
    assert np.array_equal(np.ascontiguousarray(Tb[1]).view(np.float64), T1b[0].view(np.float64)) and np.array_equal(np.ascontiguousarray(dTb[1]).view(np.float64), dT1b[0].view(np.float64))
    assert fc.same_bits(vb[:, 1], v1b[:, 0]) and np.array_equal(sb[:, 1], s1b[:, 0]) and fc.same_bits(dsb[:, :, 1], ds1b[:, :, 0])
    # a sample whose DC fails (an infinite resistor leaves a current source on a node nothing else holds): status and NaN, the others served
    c = LG.loop()
    c.I("i1", "n", 0, dc=1e-3)
    c.R("rn", "n", 0, 1e3)
    ids = [c.slot("rn"), c.slot("r2")]
    res = resolve_fmeasures(ms, _loop_gain_rows)
    o = dict(abstol=1e-12, n_restarts=2, maxiters=5)
    e = E(c)
    e.set_samples(3)
    e.set_params(ids[:1], [[1e3, math.inf, 2e3]])
    rc, T, dT, val, status, ds, sample_status, st = e.loop_gain(dev(c), f, ids, res.specs, 1, dc_opts(**o))
    assert rc == -3 and sample_status[0] == 0 and sample_status[1] != 0 and sample_status[2] == 0
    assert np.isnan(T[1]).all() and np.isnan(dT[1]).all() and status[0, 1] == 5 and np.isnan(val[0, 1]) and np.isnan(ds[0, :, 1]).all()
    e1 = E(c)
    rc1, T1, dT1, val1, status1, ds1, _, _ = e1.loop_gain(dev(c), f, ids, res.specs, 1, dc_opts(**o))
    assert rc1 == 0
    for s in (0, 2):
        assert np.array_equal(T[s].view(np.float64), T1[0].view(np.float64)) and status[0, s] == 0 and fc.same_bits(val[0, s], val1[0, 0])
    assert np.array_equal(np.ascontiguousarray(dT[0][:, 1]).view(np.float64), np.ascontiguousarray(dT1[0][:, 1]).view(np.float64))


# ---- refusals ----
def test_refusals_name_the_probe_and_run_no_dc_solve(E):
    f = np.array([1e3, 1e6])
    c = LG.loop()
    c.V("vdd", "h", 0, dc=1.0)
    c.R("rh", "h", "o", 1e6)
    c.V("vh", "h", "o2", dc=0.0)           # a second source whose + node is held by vdd
    c.R("rh2", "o2", 0, 1e3)
    c.V("vg", 0, "o3", dc=0.0)             # ... and one whose + node is ground
    c.R("rh3", "o3", 0, 1e3)
    ids = [c.slot(PROBE, "m"), c.slot("r2")]
    o = opts(c)

    def refused(e, code, text, probe, slot_ids=(), specs=None, n_meas=0, freqs=f):
        rc, T, dT, val, status, ds, sample_status, st = e.loop_gain(probe, freqs, slot_ids, specs, n_meas, o)
        msg = e.ctx.last_error()
        assert rc == code and text in msg and ("probe: device %d" % probe) in msg, (rc, msg)
        # no DC solve ran: the driver publishes the statistics of every call that reached the operating point, however it ends
        # (iterations, evaluations and dc_seconds of the DC solve included), so a refusal placed behind it would show here
        assert st["nnonliniter"] == 0 and st["nf"] == 0 and st["n_kernel_launches"] == 0 and st["dc_seconds"] == 0.0, st
        assert np.isnan(T).all()

    e = E(c)
    refused(e, -1, "not a voltage source", dev(c, "r1"))
    refused(e, -1, "not a voltage source", dev(c, "gm"))
    refused(e, -1, "+ node", dev(c, "vh"))
    refused(e, -1, "+ node", dev(c, "vg"))
    refused(e, -6, "multiplier", dev(c), ids)
    refused(e, -1, "slot", dev(c), [99])
    refused(e, -1, "frequenc", dev(c), freqs=np.array([1e3, -1.0]))
    res = resolve_fmeasures([unity_gain_freq("fug", "T")], _loop_gain_rows)
    res.specs[0].s1.row_a = 1               # there is one row: 0 = T
    refused(e, -1, "measure 0", dev(c), specs=res.specs, n_meas=1)
    rc = e.loop_gain(dev(c), f, ids[1:], opts=o)[0]
    assert rc == 0, e.ctx.last_error()      # the same circuit is served once the call is valid
    # without its AC magnitude the probe is a 0 V wire: merged away, its branch current eliminated
    from cedarsim_jl_amd.engine import EngineCircuit
    e2 = EngineCircuit(LG.loop(), small_signal=False)
    refused(e2, -1, "eliminated", dev(c))
    # more than 4096 coupled unknowns: refused before the DC solve (an RC ladder of 4200 sections behind the loop)
    big = LG.loop()
    for i in range(4200):
        big.R("rl%d" % i, "o" if i == 0 else "l%d" % (i - 1), "l%d" % i, 1e3)
        big.C("cl%d" % i, "l%d" % i, 0, 1e-12)
    e3 = E(big)
    rc, T, dT, val, status, ds, sample_status, st = e3.loop_gain(dev(big), f, opts=dc_opts(abstol=1e-12))
    assert rc == -6 and "4096" in e3.ctx.last_error() and ("probe: device %d" % dev(big)) in e3.ctx.last_error() and st["nf"] == 0
    with pytest.raises(CedarError, match="unknown probe"):
        loop_gain(LG.loop(), "nosuchprobe", f)
    with pytest.raises(CedarError, match="not a voltage source"):
        loop_gain(LG.loop(), "r1", f)


def test_the_circuit_is_left_alone(E):
    """ch_dc before and after a loop-gain call with parameters gives the same bits: nothing writes the circuit's tables."""
    c = feedback_amp()
    ids = [slot_of(c, nm) for nm in AMP_PARAMS]
    e = E(c)
    o = dc_opts(abstol=1e-12)
    rc0, x0, _, _ = e.dc(o)
    rc = e.loop_gain(dev(c), AMP_FREQS[:2], ids, opts=o)[0]
    rc1, x1, _, _ = e.dc(o)
    assert rc0 == 0 and rc == 0 and rc1 == 0 and np.array_equal(x0.view(np.uint64), x1.view(np.uint64))
