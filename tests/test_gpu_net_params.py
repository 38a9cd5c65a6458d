"""GPU tests of the N-port network analysis: net_params / ch_net_params, its sensitivities and its measures.

Linear networks against the CPU yardstick of netparams_reference.py (numpy stamps, every solve refined at 40 digits, the combination
into S and Z in mpmath; pinned by test_netparams_reference.py) at the shape edges of netparams_solve_kernel: the bilateral VCCS stage
with 5 unknowns and 2 ports (fused, and the forced sparse path) and with 64, eight ports on an R-C star with 96 unknowns (the LDS
limit) and 97 (the global workspace, forced sparse), and a one-port of 2 unknowns.  Per kind the error is max|X - X_ref| / max|X_ref|
over the grid and the entries under smallsignal_cases.tolerance(e_cpu) = max(1e-12, 32 e_cpu), e_cpu the same error of the kind formed
from plain LAPACK solves in numpy; a case with e_cpu > 1e-11 is refused.  The same tolerance holds Yp against Yp formed in numpy from P
existing ac() runs (one port at |ac| = 1, the others at 0 with their currents observed), which pins the rule of the right-hand sides
and the sign.  dS, dY, dZ at 0, 1 MHz and 10 GHz against the yardstick's analytic values under acsens_reference.tolerance(e_cpu), e_cpu
the error of the engine's method in numpy (netparams_reference.fd_net_sens) by the rule of loopgain_reference.sens_errors, the entries
of a matrix taken with the frequencies.
A BSIM4 amplifier as a two-port (port 1 carries the gate bias): S against the ac() construction, dS/dp against Richardson central
differences of that construction at the steps and under the admission and tolerance test_gpu_ac_sens.py grants its amplifier: steps
2e-5 / 1e-5, own estimate <= 1e-7, tolerance 1e-6.  Measures on "s21" of a Butterworth low-pass, a sweep, a sample without an
operating point, a series-only network, and the refusals."""
import copy
import math

import numpy as np
import pytest

import acsens_reference as AR
import fmeasure_cases as fc
import fmeasure_reference as fr
import netparams_reference as NP
import smallsignal_cases as cases
from cedarsim_jl_amd import Circuit, CircuitSweep, Sweep, acdec, bandwidth, db, dc_opts, net_params
from cedarsim_jl_amd.acmeasure import net_rows, resolve_fmeasures
from cedarsim_jl_amd.circuit import CedarError

from test_gpu_ac_noise import gf180_models

pytestmark = pytest.mark.gpu
F3 = np.array([0.0, 1e6, 1e10])
SHAPES = [("stage", 5), ("stage", 64), ("star8", 96), ("star8", 97), ("one",)]


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


def devs(c, ports):
    return [c.dev_names.index(p) for p in ports]


def run_values(E, c, ports, z0, freqs, o=None):
    e = E(c)
    rc, X, _, _, _, _, status, st = e.net_params(devs(c, ports), z0, freqs, opts=o or opts(c))
    assert rc == 0 and not status.any(), e.ctx.last_error()
    return {k: v[0] for k, v in X.items()}, e.info()


# ---- shape edges ----
@pytest.mark.parametrize("key", SHAPES, ids=lambda k: "-".join(str(x) for x in k))
def test_values_at_every_shape_edge(E, monkeypatch, key):
    """Measured on the MI355X (e_cpu / GPU error for S, Y, Z; tolerance 1e-12 each): stage(5) 3.3e-16 / 2.2e-16, 1.4e-16 / 1.3e-19,
    4.2e-16 / 2.8e-16; stage(64) 3.3e-16 / 2.2e-16, 2.7e-19 / 2.1e-18, 7.2e-16 / 7.2e-16; star8(96) 6.7e-16 / 3.3e-16, 2.0e-16 / 2.0e-16,
    3.0e-16 / 2.0e-16; star8(97) 4.4e-16 / 4.7e-16, 2.0e-16 / 2.0e-16, 4.0e-16 / 6.0e-16; the one-port 2.2e-16 / 1.1e-16, 2.8e-19 / 0,
    1.8e-16 / 1.8e-16 (the table of DESIGN.md 2.7k)."""
    c, ports, z0, ref, e_cpu, tol = NP.shape_case(key)
    n = {"one": 2}.get(key[0], key[-1])
    if n == 97:
        X, info = forced_sparse(monkeypatch, lambda: run_values(E, c, ports, z0, cases.FREQS))
        assert info["path"] == 2
    else:
        X, info = run_values(E, c, ports, z0, cases.FREQS)
        assert info["path"] == (1 if n <= 64 else 2)
    assert info["n_unknowns"] == n and info["n_components"] == 1
    for kd in NP.KINDS:
        err = NP.errors(X[kd], ref[kd])
        print("%s %s: e_cpu %.2e, GPU error %.2e, tolerance %.2e" % (key, kd, e_cpu[kd], err, tol[kd]))
        assert not np.isnan(X[kd]).any() and err <= tol[kd], (key, kd, err, tol[kd])
    if key == ("stage", 5):   # the same LDS kernel, G and C arriving through the sparse path's dense expansion
        X2, info2 = forced_sparse(monkeypatch, lambda: run_values(E, c, ports, z0, cases.FREQS))
        assert info2["path"] == 2
        for kd in NP.KINDS:
            assert NP.errors(X2[kd], ref[kd]) <= tol[kd]
    if key == ("one",):
        assert abs(X["Y"][0, 0, 0] - 1.0 / 80.0) <= tol["Y"] / 80.0      # Y11 = +1/R at DC: the current entering the network counts


# ---- agreement with the family ----
def ac_engines(E, c, ports):
    """One engine per port: that port at |ac| = 1, the others at 0 with their branch currents observed (so that they stay unknowns)."""
    out = []
    for p in ports:
        d = copy.deepcopy(c)
        d.source_ac = [0.0] * len(d.source_ac)
        d.source_ac[d.dev_ipar[d.dev_names.index(p)][0]] = 1.0
        for q in ports:
            d.observe_branch(q)
        out.append(E(d))
    return out


def yp_from_ac_runs(c, ports, freqs, o, engines):
    """Yp[n_freq][P][P] in numpy from P ac() runs: Yp[j][k] = -(the current of port j in run k)."""
    rows = NP.port_rows(c, ports)
    Yp = np.zeros((len(freqs), len(ports), len(ports)), dtype=np.complex128)
    for k, e in enumerate(engines):
        rc, x, _ = e.ac(freqs, o)
        assert rc == 0, e.ctx.last_error()
        Yp[:, :, k] = -x[0][:, rows]
    return Yp


@pytest.mark.parametrize("key", [("stage", 5), ("star8", 96)], ids=lambda k: "-".join(str(x) for x in k))
def test_Y_agrees_with_P_ac_runs(E, key):
    """Measured on the MI355X (tolerance 1e-12): stage(5) Y 1.3e-22, S 2.5e-16; star8(96) Y 6.2e-18, S 7.8e-16."""
    c, ports, z0, ref, e_cpu, tol = NP.shape_case(key)
    X, _ = run_values(E, c, ports, z0, cases.FREQS)
    Y2 = yp_from_ac_runs(c, ports, cases.FREQS, opts(c), ac_engines(E, c, ports))
    S2 = np.array([NP.s_of_y_np(y, z0) for y in Y2])
    eY, eS = NP.errors(X["Y"], Y2), NP.errors(X["S"], S2)
    print("%s against %d ac() runs: Y %.2e (tolerance %.2e), S %.2e (tolerance %.2e)" % (key, len(ports), eY, tol["Y"], eS, tol["S"]))
    assert eY <= tol["Y"] and eS <= tol["S"]
    assert NP.errors(Y2, ref["Y"]) <= tol["Y"]      # (the ac() construction is itself within the tolerance of the yardstick)


# ---- sensitivities, linear ----
SENS_NAMES = {("stage", 5): ["rin", "rg", "cg", "gm", "ro", "co", "rf", "cf"], ("star8", 96): ["ra1", "ca3", "rsh8", "rm"], ("star8", 97): ["ra1", "ca3", "rsh8", "rm"]}
_SENS = {}


def sens_case(key):
    if key not in _SENS:
        c, ports, z0 = NP.shape_case(key)[:3]
        names = list(SENS_NAMES[key])
        if key[0] == "star8":      # ... and two elements of the tail: its first inductor and an element half way down
            tail = [nm for nm in c.dev_names if nm.startswith("t") and not nm.startswith("trt")]
            names += [tail[1], tail[len(tail) // 2]]
        ids = [c.slot(nm) for nm in names]
        slots = [c.slots[i] for i in ids]
        ref = NP.net_params(c, ports, z0, F3, slots=slots)
        fd = NP.fd_net_sens(c, ports, z0, F3, slots)
        e_cpu = {kd: float(NP.sens_errors(fd["d" + kd], ref["d" + kd]).max()) for kd in NP.KINDS}
        _SENS[key] = (c, ports, z0, names, ids, ref, e_cpu, {kd: AR.tolerance(e) for kd, e in e_cpu.items()})
    return _SENS[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


@pytest.mark.parametrize("key", sorted(SENS_NAMES), ids=lambda k: "-".join(str(x) for x in k))
def test_linear_sensitivities(E, monkeypatch, key):
    """Measured on the MI355X (S / Y / Z): stage(5) e_cpu 3.5e-10 / 3.3e-10 / 4.0e-10, tolerance 1.1e-08 / 1.1e-08 / 1.3e-08, GPU worst
    3.5e-10 / 3.3e-10 / 4.0e-10 (rf); star8(96) and star8(97) e_cpu 8.0e-11 / 7.5e-11 / 6.1e-09, tolerance 2.6e-09 / 2.4e-09 / 2.0e-07, GPU
    worst 1.1e-10 / 7.5e-11 / 1.7e-08 (ca3)."""
    c, ports, z0, names, ids, ref, e_cpu, tol = sens_case(key)
    pd = devs(c, ports)

    def run():
        e = E(c)
        rc, X, dX, _, _, _, status, st = e.net_params(pd, z0, F3, ids, opts=opts(c))
        assert rc == 0 and not status.any(), e.ctx.last_error()
        # chunked and single-parameter calls: the same bits
        half = len(ids) // 2
        parts = [e.net_params(pd, z0, F3, ids[:half], opts=opts(c))[2], e.net_params(pd, z0, F3, ids[half:], opts=opts(c))[2]]
        for kd in NP.KINDS:
            assert np.array_equal(bits(np.concatenate([parts[0][kd], parts[1][kd]], axis=2)), bits(dX[kd])), kd
        for k in (0, len(ids) - 1):
            one = e.net_params(pd, z0, F3, ids[k:k + 1], opts=opts(c))[2]
            for kd in NP.KINDS:
                assert np.array_equal(bits(one[kd][:, :, 0]), bits(dX[kd][:, :, k])), kd
        rc0, X0 = e.net_params(pd, z0, F3, opts=opts(c))[:2]
        assert rc0 == 0
        for kd in NP.KINDS:
            assert np.array_equal(bits(X0[kd]), bits(X[kd])), kd       # the values do not depend on the parameters asked for
        rcs, Xs, dXs = e.net_params(pd, z0, F3, ids, opts=opts(c), kinds="S")[:3]
        assert rcs == 0 and list(Xs) == ["S"] and np.array_equal(bits(Xs["S"]), bits(X["S"])) and np.array_equal(bits(dXs["S"]), bits(dX["S"]))   # ... nor on the kinds
        return {k: v[0] for k, v in X.items()}, {k: v[0] for k, v in dX.items()}, e.info()

    X, dX, info = forced_sparse(monkeypatch, run) if key[-1] == 97 else run()
    assert info["n_unknowns"] == key[-1]
    for kd in NP.KINDS:
        err = NP.sens_errors(dX[kd], ref["d" + kd])
        print("%s d%s/dp: e_cpu %.2e, tolerance %.2e; GPU errors %s" % (key, kd, e_cpu[kd], tol[kd], ", ".join("%s %.1e" % (nm, x) for nm, x in zip(names, err))))
        assert not np.isnan(dX[kd]).any() and err.max() <= tol[kd], (kd, names[int(np.argmax(err))], err.max(), tol[kd])
        assert NP.errors(X[kd], ref[kd]) <= cases.tolerance(NP.errors(ref[kd + "_l"], ref[kd]))


# ---- a series-only two-port: Yp is singular, which is no failure ----
def test_series_only_two_port(E):
    c, ports = NP.series_r(50.0)
    f = np.array([0.0, 1e6, 1e9])
    ref = NP.net_params(c, ports, 50.0, f, want_z=False)
    e = E(c)
    rc, X, _, _, _, _, status, st = e.net_params(devs(c, ports), [50.0, 50.0], f, opts=opts(c))
    assert rc == 0 and not status.any(), e.ctx.last_error()      # rc 0: the fail flag of the complex solves is not set
    for kd in "SY":
        assert NP.errors(X[kd][0], ref[kd]) <= cases.tolerance(NP.errors(ref[kd + "_l"], ref[kd]))
    assert abs(X["S"][0, 0, 0, 0] - 1.0 / 3.0) <= 1e-12 and abs(X["S"][0, 0, 1, 0] - 2.0 / 3.0) <= 1e-12 and abs(X["Y"][0, 0, 0, 0] - 0.02) <= 1e-12


# ---- MOSFET ----
AMP_PARAMS = ["rd", ("m1", "w"), "temp"]
AMP_FREQS = np.array([1e2, 1e4, 1e6, 1e7, 1e8])
AMP_PORTS = ("vp1", "vp2")
STEPS = (2e-5, 1e-5)
TOL, ADMIT = 1e-6, 1e-7


def amp_two_port():
    """The amplifier of test_gpu_ac_noise.amp_circuit (its cards, its load) as a two-port: port 1 drives the gate and carries its bias
    as its DC value (2 V, what the divider of the original gives), port 2 sits at the output through a coupling capacitor."""
    c = Circuit(gmin=1e-12)
    c.temp = 40.0
    m = gf180_models()
    n = c.add_model(*m["nfet_06v0"])
    p = c.add_model(*m["pfet_06v0"])
    c.V("vdd", "vdd", 0, dc=5.0)
    c.V("vp1", "g", 0, dc=2.0, ac=1.0)
    c.M("m1", "d", "g", "s", 0, n, 2e-6, 6e-7)
    c.R("rd", "vdd", "d", 20e3)
    c.R("rs", "s", 0, 1e3)
    c.C("cs", "s", 0, 1e-9)
    c.M("m2", "o", "d", "vdd", "vdd", p, 4e-6, 5e-7)
    c.R("ro", "o", 0, 50e3)
    c.C("co", "o", 0, 1e-12)
    c.C("cout", "o", "p2", 1e-9)
    c.V("vp2", "p2", 0, dc=0.0, ac=1.0)
    return c


def slot_of(c, name):
    return c.slot(*name) if isinstance(name, tuple) else c.slot(name)


def base_value(c, slot):
    kind, a, b = c.slots[slot]
    return c.temp if kind == 5 else c.dev_par[a][b]


def test_mosfet_amplifier_against_differences_of_the_ac_construction(E):
    """Errors are per frequency, max over the entries of |dS - r| against the largest entry of r (the entries of one matrix share a
    scale, as the rows of a group do in acsens_reference.scaled_errors).  Measured on the MI355X: S against the ac() construction
    2.2e-16 (bound 1e-12); the yardstick's own estimates rd 4.8e-08, m1.w 3.2e-08, temp 3.5e-08; errors of dS/dp: rd 1.3e-09 .. 1.8e-09,
    m1.w 1.1e-09 .. 8.2e-09, temp 1.2e-09 .. 6.0e-08."""
    c = amp_two_port()
    z0 = [50.0, 50.0]
    ids = [slot_of(c, nm) for nm in AMP_PARAMS]
    o = dc_opts(abstol=1e-13)
    e = E(c)
    rc, X, dX, _, _, _, status, st = e.net_params(devs(c, AMP_PORTS), z0, AMP_FREQS, ids, opts=o, kinds="S")
    assert rc == 0 and not status.any(), e.ctx.last_error()
    S, dS = X["S"][0], dX["S"][0]
    engines = ac_engines(E, c, AMP_PORTS)

    def s_from_ac():
        return np.array([NP.s_of_y_np(y, z0) for y in yp_from_ac_runs(c, AMP_PORTS, AMP_FREQS, o, engines)])

    eS = NP.errors(S, s_from_ac())
    print("amplifier: S against the ac() construction %.2e; |S21| = %s" % (eS, " ".join("%.3g" % abs(t) for t in S[:, 1, 0])))
    # the project's rule; there is no CPU yardstick for a BSIM4 circuit, so e_cpu = 0 and the bound is the rule's floor, 1e-12: the
    # engines solve the same operating point from the same start with the same seed, and G, C are the same dumps
    assert eS <= cases.tolerance(0.0)
    for k, nm in enumerate(AMP_PARAMS):
        p = base_value(c, ids[k])
        y = []
        for rel in STEPS:
            h = rel * abs(p)
            pair = []
            for sign in (+1, -1):
                for eng in engines:
                    eng.set_params([ids[k]], [[p + sign * h]])
                pair.append(s_from_ac())
            y.append((pair[0] - pair[1]) / (2.0 * h))
        for eng in engines:
            eng.set_params([ids[k]], [[p]])
        r = (4.0 * y[1] - y[0]) / 3.0
        top = np.abs(r).max(axis=(1, 2))
        est = np.abs(y[1] - r).max(axis=(1, 2)) / top
        err = np.abs(dS[:, k] - r).max(axis=(1, 2)) / top
        print("amplifier dS/d%s: yardstick's own estimate %.1e, GPU error %s" % (nm, est.max(), " ".join("%.1e" % x for x in err)))
        assert est.max() <= ADMIT, "slot %r refused: the yardstick's own estimate is %.2e" % (nm, est.max())
        assert err.max() <= TOL, (nm, err)


# ---- measures ----
BW_FC = 1e8
BW_RSER = 0.1       # ohms in series with the inductor: a lossless ladder between two ideal port sources has no DC operating point
MEAS_F = acdec(40, 1e6, 1e9)
MEAS_PARAMS = ["c1", "c3", "l2"]


def yardstick_specs(measures, P):
    res = resolve_fmeasures(measures, net_rows(P))
    out = []
    for k in range(len(res.names)):
        sp = res.specs[k]
        sides = [fr.side(sd.row_a, sd.row_b, sd.scale, fr.SIGS[sd.sig], sd.level, {1: "rise", 2: "fall", 3: "cross"}[sd.edge], sd.count, sd.fd, sd.ref_at) for sd in (sp.s1, sp.s2)]
        out.append(fr.spec(fr.KINDS[sp.kind], sides[0], sides[1], ("lin", "log")[sp.xscale], sp.at, sp.frm, sp.to))
    return res, out


def rows_of(S, dS, P):
    """The rows of kind S as the measures number them (kind * P^2 + j * P + k; Y and Z left zero): H[3 P^2][n_freq], dH[3 P^2][n_par][n_freq]."""
    nf, n_par = S.shape[0], dS.shape[1]
    H, dH = np.zeros((3 * P * P, nf), dtype=np.complex128), np.zeros((3 * P * P, n_par, nf), dtype=np.complex128)
    H[:P * P] = S.reshape(nf, P * P).T
    dH[:P * P] = np.transpose(dS.reshape(nf, n_par, P * P), (2, 1, 0))
    return H, dH


def test_bandwidth_of_a_butterworth_with_its_sensitivities(E):
    """bandwidth("bw", "s21") of the third-order Butterworth low-pass is its corner fc (the yardstick's figure on the grid of 40 points
    per decade lies within 1e-4 of it: fc is a grid point, the measure interpolates 20 log10 |S21| linearly in log10 f, and the 0.1 ohm
    in series with the inductor, without which the circuit has no DC operating point, moves the corner by 3 parts in 1e7), with d/d c1,
    d/d c3, d/d l2.  Under
    the rule of the ch_ac_measure tests (2.7g: max(1e-12, 32 e_cpu) of the measure's scale, statuses exactly): the measure kernel
    against the 40-digit yardstick on the rows the same call hands back, and against the yardstick fed the rows of
    netparams_reference, e_cpu there the float64 measure on the rows of the engine's method in numpy (fd_net_sens, S from LAPACK).
    Measured on the MI355X: own rows 1.1e-16 (values), 7.0e-16 (derivatives); reference rows bw 2.6e-15 / 2.9e-14 (e_cpu 9.4e-15 /
    1.4e-13), the 1 dB bandwidth 4.5e-15 / 1.6e-14 (e_cpu 8.2e-15 / 7.0e-14); bw = 9.999997122e+07 Hz."""
    c, ports = NP.butterworth(50.0, BW_FC, rser=BW_RSER)
    ids = [c.slot(nm) for nm in MEAS_PARAMS]
    ms = [bandwidth("bw", "s21", ref_at=MEAS_F[0]), bandwidth("bw1db", db("S21", scale=2.0), ref_at=MEAS_F[0], drop_db=1.0)]
    res, specs = yardstick_specs(ms, 2)
    e = E(c)
    rc, X, dX, val, status, ds, sample_status, st = e.net_params(devs(c, ports), [50.0, 50.0], MEAS_F, ids, res.specs, len(res.names), opts(c), kinds="S")
    assert rc == 0 and not sample_status.any() and np.all(status == 0), (e.ctx.last_error(), status)
    H, dH = rows_of(X["S"][0], dX["S"][0], 2)
    own = fc.references(specs, MEAS_F, H, dH, limit=1e-9)
    fc.compare("network parameters, own rows", specs, lambda s: own, val, status, ds, len(ids))
    slots = [c.slots[i] for i in ids]
    ref = NP.net_params(c, ports, 50.0, MEAS_F, slots=slots, want_z=False)
    fd = NP.fd_net_sens(c, ports, 50.0, MEAS_F, slots, want_z=False)
    H_ref, dH_ref = rows_of(ref["S"], ref["dS"], 2)
    H_l, dH_fd = rows_of(ref["S_l"], fd["dS"], 2)
    for k, sp in enumerate(specs):
        vm, stm, dm = fr.measure_mp(MEAS_F, H_ref, dH_ref, sp)
        vf, stf, df = fr.measure_f64(MEAS_F, H_l, dH_fd, sp)
        assert stm == 0 and stf == 0
        vs, ss = fc.scales(sp, MEAS_F, H_ref, dH_ref)
        ev_cpu, es_cpu = fc.figure_errors(sp, vf, df, vm, dm, vs, ss)
        ev, es = fc.figure_errors(sp, float(val[k, 0]), [float(x) for x in ds[k, :, 0]], vm, dm, vs, ss)
        print("%s against the reference rows: value %.2e (e_cpu %.2e), derivatives %.2e (e_cpu %.2e); value %.9e Hz, d/d(c1, c3, l2) = %s" % (
            res.names[k], ev, ev_cpu, es, es_cpu, val[k, 0], " ".join("%.4e" % x for x in ds[k, :, 0])))
        assert max(ev_cpu, es_cpu) <= 1e-9, "mis-designed case"
        assert ev <= max(1e-12, 32.0 * ev_cpu) and es <= max(1e-12, 32.0 * es_cpu), (res.names[k], ev, es)
    assert abs(float(own[0]["value"]) - BW_FC) <= 1e-4 * BW_FC and abs(val[0, 0] - BW_FC) <= 1e-4 * BW_FC
    # In the continuum d(bw)/dp = -(dg/dp) / (dg/df) with g = 20 log10 |S21| gives -fc / (6 C) per capacitor and -2 fc / (3 L) for the
    # inductor (scaling all three by a scales the corner by 1/a: the shares add up to 1).  The measure differentiates its own linear
    # interpolant in (log10 f, dB): the secant slope over one grid interval, 1/40 decade, differs from the tangent by at most
    # g'' d / (2 g') = (90 / ln 10) (ln 10 / 40) / (2 * 30 / ln 10) = 8.7 % at the corner, hence the 10 %.
    share = {"c1": 1.0 / 6.0, "c3": 1.0 / 6.0, "l2": 2.0 / 3.0}
    want = [-share[nm] * BW_FC / c.dev_par[c.dev_names.index(nm)][0] for nm in MEAS_PARAMS]
    assert np.allclose(ds[0, :, 0], want, rtol=0.1, atol=0.0), (ds[0, :, 0], want)
    # the public surface hands out the same figures
    sol = net_params(c, ports, MEAS_F, z0=50.0, params=MEAS_PARAMS, measures=ms, abstol=1e-12)
    assert sol.rc == 0 and sol.measure_status == {"bw": 0, "bw1db": 0} and sol.ports == ports and np.array_equal(sol.z0, [50.0, 50.0])
    assert math.isclose(sol.measures["bw"], val[0, 0], rel_tol=1e-9) and math.isclose(sol.measure_sens["bw", "c3"], ds[0, 1, 0], rel_tol=1e-6)
    assert np.allclose(sol.S, X["S"][0], rtol=1e-9, atol=1e-15) and np.allclose(sol.sens_S["l2"], dX["S"][0][:, 2], rtol=1e-6, atol=0.0) and np.array_equal(sol.freqs, MEAS_F)
    assert np.array_equal(sol.s(2, 1), sol.S[:, 1, 0]) and sol.Y.shape == sol.Z.shape == (len(MEAS_F), 2, 2)
    assert NP.errors(sol.S, ref["S"]) <= cases.tolerance(NP.errors(ref["S_l"], ref["S"]))
    # (the series resistance costs |S21|^2 at most 2 rser / z0 = 4e-3 of the lossless closed form, which test_netparams_reference.py
    # pins to 1e-12: the insertion loss of rser between two z0)
    assert np.max(np.abs(np.abs(sol.s(2, 1)) ** 2 - 1.0 / (1.0 + (MEAS_F / BW_FC) ** 6))) <= 2.0 * BW_RSER / 50.0
    with pytest.raises(CedarError, match="s21"):
        net_params(c, ports, MEAS_F, measures=[bandwidth("bw", "p2", ref_at=1e6)])


# ---- batch ----
def test_a_sweep_of_cf_and_a_sample_without_an_operating_point(E):
    cfs = [2e-14, 5e-14, 2e-13]
    f = cases.FREQS[2:6]
    ports = ("vp1", "vp2")

    def build(cf=5e-14):
        c = NP.stage(5)[0]
        c.dev_par[c.dev_names.index("cf")][0] = cf
        return c

    ms = [bandwidth("bw", "y21", ref_at=f[0], xscale="lin")]
    sols = net_params(CircuitSweep(build, Sweep(cf=cfs)), ports, f, z0=NP.Z0_STAGE, params=["rg", "cf"], measures=ms, abstol=1e-12)
    assert len(sols) == 3
    one = net_params(build(cfs[1]), ports, f, z0=NP.Z0_STAGE, params=["rg", "cf"], measures=ms, abstol=1e-12)
    for sol, cf in zip(sols, cfs):
        c = build(cf)
        slots = [(1, c.dev_names.index("rg"), 0), (1, c.dev_names.index("cf"), 0)]
        ref = NP.net_params(c, ports, NP.Z0_STAGE, f, slots=slots)
        fd = NP.fd_net_sens(c, ports, NP.Z0_STAGE, f, slots)
        assert sol.rc == 0 and sol.params == {"cf": cf}
        for kd, X, dX in (("S", sol.S, sol.sens_S), ("Y", sol.Y, sol.sens_Y), ("Z", sol.Z, sol.sens_Z)):
            assert NP.errors(X, ref[kd]) <= cases.tolerance(NP.errors(ref[kd + "_l"], ref[kd]))
            assert NP.sens_errors(dX.array, ref["d" + kd]).max() <= AR.tolerance(float(NP.sens_errors(fd["d" + kd], ref["d" + kd]).max()))
    # the sweep's point equals its own single call
    assert np.allclose(sols[1].S, one.S, rtol=1e-12, atol=0.0) and np.allclose(sols[1].sens_Z.array, one.sens_Z.array, rtol=1e-12, atol=0.0)
    assert sols[1].measure_status == one.measure_status and (math.isclose(sols[1].measures["bw"], one.measures["bw"], rel_tol=1e-12) or one.measure_status["bw"] != 0)
    # a sample whose DC fails (an infinite resistor leaves a current source on a node nothing else holds): status and NaN, the others served
    c = NP.stage(5)[0]
    c.I("i1", "nx", 0, dc=1e-3)
    c.R("rn", "nx", 0, 1e3)
    ids = [c.slot("rn"), c.slot("rg")]
    res = resolve_fmeasures([bandwidth("bw", "s21", ref_at=f[0], xscale="lin")], net_rows(2))
    o = dict(abstol=1e-12, n_restarts=2, maxiters=5)
    pd = devs(c, ports)
    e = E(c)
    e.set_samples(3)
    e.set_params(ids[:1], [[1e3, math.inf, 2e3]])
    rc, X, dX, val, status, ds, sample_status, st = e.net_params(pd, NP.Z0_STAGE, f, ids, res.specs, 1, dc_opts(**o))
    assert rc == -3 and sample_status[0] == 0 and sample_status[1] != 0 and sample_status[2] == 0
    e1 = E(c)
    rc1, X1, dX1, val1, status1, ds1, _, _ = e1.net_params(pd, NP.Z0_STAGE, f, ids, res.specs, 1, dc_opts(**o))
    assert rc1 == 0
    assert status[0, 1] == 5 and np.isnan(val[0, 1]) and np.isnan(ds[0, :, 1]).all()
    for kd in NP.KINDS:
        assert np.isnan(X[kd][1]).all() and np.isnan(dX[kd][1]).all()
        for s in (0, 2):
            assert np.array_equal(bits(X[kd][s]), bits(X1[kd][0])) and np.array_equal(bits(dX[kd][s][:, 1]), bits(dX1[kd][0][:, 1]))
    for s in (0, 2):
        assert status[0, s] == status1[0, 0] and fc.same_bits(val[0, s], val1[0, 0])


# ---- refusals ----
def test_refusals_name_the_port_and_run_no_dc_solve(E):
    f = np.array([1e3, 1e6])
    c, ports = NP.stage(5)
    c.V("vdd", "h", 0, dc=1.0)              # an ordinary source: no port
    c.R("rh", "h", "n", 1e6)
    ids = [c.slot("vp2", "m"), c.slot("rg")]
    o = opts(c)
    pd = devs(c, ports)

    def refused(e, code, text, port_devs, named=None, z0=None, slot_ids=(), specs=None, n_meas=0, freqs=f):
        rc, X, dX, val, status, ds, sample_status, st = e.net_params(port_devs, z0 or [50.0] * len(port_devs), freqs, slot_ids, specs, n_meas, o)
        msg = e.ctx.last_error()
        assert rc == code and text in msg and "ch_net_params" in msg, (rc, msg)
        if named is not None:
            assert ("port %d (device %d)" % (named + 1, port_devs[named])) in msg, msg
        # no DC solve ran: the driver publishes the statistics of every call that reached the operating point, however it ends
        assert st["nnonliniter"] == 0 and st["nf"] == 0 and st["n_kernel_launches"] == 0 and st["dc_seconds"] == 0.0, st
        assert all(np.isnan(v).all() for v in X.values())

    e = E(c)
    refused(e, -1, "not a voltage source", [pd[0], c.dev_names.index("rg")], named=1)
    refused(e, -1, "not a voltage source", [c.dev_names.index("gm"), pd[1]], named=0)
    refused(e, -1, "twice", [pd[0], pd[0]], named=1)
    refused(e, -1, "port 2", [pd[0], c.dev_names.index("vdd")], named=1)        # (a DC source: folded into a known node, or without |ac| = 1)
    refused(e, -1, "no port carries", [pd[0]])                                  # vp2 is driven but is no port of the call
    refused(e, -1, "reference impedance", pd, named=1, z0=(50.0, 0.0))
    refused(e, -1, "reference impedance", pd, named=0, z0=(math.inf, 50.0))
    refused(e, -1, "between 1 and 8", pd * 5)
    refused(e, -6, "multiplier", pd, named=1, slot_ids=ids)
    refused(e, -1, "slot", pd, slot_ids=[99])
    refused(e, -1, "frequenc", pd, freqs=np.array([1e3, -1.0]))
    res = resolve_fmeasures([bandwidth("bw", "s21", ref_at=1e3)], net_rows(2))
    res.specs[0].s1.row_a = 12              # two ports have the rows 0 .. 11
    refused(e, -1, "measure 0", pd, specs=res.specs, n_meas=1)
    rc = e.net_params(pd, (50.0, 75.0), f, ids[1:], opts=o)[0]
    assert rc == 0, e.ctx.last_error()      # the same circuit is served once the call is valid
    # a port with a multiplier other than 1
    c2 = NP.stage(5)[0]
    c2.dev_mult[c2.dev_names.index("vp2")] = 2.0
    refused(E(c2), -1, "multiplier must be 1", pd, named=1)
    # without its AC magnitude a port is a 0 V wire to ground: its node is known, its branch current eliminated
    c3 = NP.stage(5)[0]
    c3.source_ac[c3.dev_ipar[pd[1]][0]] = 0.0
    refused(E(c3), -1, "eliminated", pd, named=1)
    # ports in separate blocks (two networks that share nothing but ground)
    c4 = Circuit()
    for j in (1, 2):
        c4.V("vp%d" % j, "p%d" % j, 0, dc=0.0, ac=1.0)
        c4.R("ra%d" % j, "p%d" % j, "q%d" % j, 100.0)
        c4.R("rb%d" % j, "q%d" % j, 0, 100.0)
    refused(E(c4), -6, "another block", devs(c4, ports), named=1)
    # more than 4096 coupled unknowns: refused before the DC solve (an RC ladder of 4200 sections behind the stage)
    big = NP.stage(5)[0]
    for i in range(4200):
        big.R("rl%d" % i, "n" if i == 0 else "l%d" % (i - 1), "l%d" % i, 1e3)
        big.C("cl%d" % i, "l%d" % i, 0, 1e-12)
    e5 = E(big)
    rc, X, dX, val, status, ds, sample_status, st = e5.net_params(devs(big, ports), (50.0, 50.0), f, opts=dc_opts(abstol=1e-12))
    assert rc == -6 and "4096" in e5.ctx.last_error() and "ch_net_params" in e5.ctx.last_error() and st["nf"] == 0
    with pytest.raises(CedarError, match="unknown port"):
        net_params(NP.stage(5)[0], ("vp1", "nosuchport"), f)
    with pytest.raises(CedarError, match="not a voltage source"):
        net_params(NP.stage(5)[0], ("vp1", "rg"), f)
    with pytest.raises(CedarError, match="reference impedances"):
        net_params(NP.stage(5)[0], ports, f, z0=(50.0, 75.0, 100.0))


def test_the_circuit_is_left_alone(E):
    """ch_dc after a network-parameter call with parameters gives the bits it gives after a plain ch_dc in its place: nothing writes
    the circuit's tables.  (A second ch_dc of the same engine need not repeat the first one's last bits: it starts where the first
    ended.)"""
    c = amp_two_port()
    ids = [slot_of(c, nm) for nm in AMP_PARAMS]
    o = dc_opts(abstol=1e-12)
    ea, eb = E(c), E(c)
    rca0, xa0, _, _ = ea.dc(o)
    rc = ea.net_params(devs(c, AMP_PORTS), [50.0, 75.0], AMP_FREQS[:2], ids, opts=o)[0]
    rca1, xa1, _, _ = ea.dc(o)
    rcb0, xb0, _, _ = eb.dc(o)
    rcb, _, _, _ = eb.dc(o)
    rcb1, xb1, _, _ = eb.dc(o)
    assert rca0 == 0 and rc == 0 and rca1 == 0 and rcb0 == 0 and rcb == 0 and rcb1 == 0
    assert np.array_equal(xa0.view(np.uint64), xb0.view(np.uint64)) and np.array_equal(xa1.view(np.uint64), xb1.view(np.uint64))
