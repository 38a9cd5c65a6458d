"""GPU tests of the AC parameter sensitivities (ch_ac_sens, direct method).

Linear circuits: against the analytic yardstick of acsens_reference.py (numpy stamps, every solve refined at 40 digits) at the shape
edges of acsens_solve_kernel — 64 | 65: fused path | sparse path, 96 | 97: LDS | global workspace, 256 | 257: a second trip of the
256-thread loops.  Errors are per frequency and parameter, scaled by max|dx/dp_k| within the node rows and the branch rows apart;
the bound is max(1e-10, 32 e_cpu), e_cpu being the error of the SAME METHOD in numpy (differences of the numpy stamps at sens_step's
steps, LAPACK solves) against the yardstick, worst over the case; a case with e_cpu > 1e-7 is refused (acsens_reference.tolerance).

Nonlinear circuits: against Richardson-extrapolated central differences of full Oracle.ac solves (oracle DC at abstol 1e-12) at
relative steps 1e-3 and 5e-4; tolerance 1e-6 of max|dx/dp_k| per frequency (the figure of test_gpu_dc_sens.py); a slot whose own
estimate max|y2 - r| / max|r| exceeds 1e-7 is refused.  For the amplifier that yardstick admits temp and co at the lower frequencies
only (test_amplifier_matches_the_oracle_yardstick pins which); every slot and frequency is compared against a yardstick with finer
steps that passes the same rule (test_amplifier_matches_a_finer_yardstick).  Figures in both docstrings and in DESIGN.md 2.7c."""
import math

import numpy as np
import pytest

import acsens_reference as AR
import smallsignal_cases as cases
import smallsignal_reference as SR
from cedarsim_jl_amd import Circuit, CircuitSweep, Sweep, ac_sens, dc_opts, mag_phase_sens
from cedarsim_jl_amd.circuit import CedarError, DEV_C, DEV_L, DEV_R, DEV_VCCS, DEV_VCVS

from test_gpu_ac_noise import amp_circuit
from test_gpu_dc_sens import base_value, slot_of

pytestmark = pytest.mark.gpu

F3 = np.array([0.0, 1e6, 1e10])
F2 = np.array([0.0, 1e6])
FL = np.array([0.0, 1e3, 1e6])    # from 97 unknowns up.  Not 1e12 Hz as in FREQS_LARGE: the response 30 sections down the ladder is 1e-100 of the
                                  # source there, its derivatives lie below anything a double-precision x can carry (e_cpu up to 1e9)


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return lambda c: EngineCircuit(c, small_signal=True)


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def opts(c, samples=1):
    """abstol 1e-12 and a zero start: a linear circuit is solved by one Newton step, the same for every sample index."""
    return dc_opts(abstol=1e-12, x0=np.zeros((samples, c.n_mna)))


def forced_sparse(monkeypatch, fn):
    monkeypatch.setenv("CEDARHIP_FORCE_SPARSE", "1")
    try:
        return fn()
    finally:
        monkeypatch.delenv("CEDARHIP_FORCE_SPARSE", raising=False)


def element_names(c):
    """Every R, C, L and controlled-source gain of the circuit, in device order — but for the series resistors rt<i> of a ladder's
    trailing RC sections.  At 0 Hz they feed capacitors alone: the voltage across them is zero, or the little a controlled source
    leaves there, and -dY/dR x is then a difference of two nearly equal node voltages that double precision resolves to 1e-6 at
    best (measured with the numpy version of the method: e_cpu = 2.3e-6 for rt1 of ladder(64)).  By the rule of this file such a
    parameter is mis-designed (e_cpu > 1e-7), so it is not among the cases."""
    return [nm for nm, k in zip(c.dev_names, c.dev_kind) if k in (DEV_R, DEV_C, DEV_L, DEV_VCCS, DEV_VCVS) and not nm.startswith("rt")]


def spread(names, count):
    return [names[int(round(j))] for j in np.linspace(0, len(names) - 1, min(count, len(names)))]


# ---- the linear yardstick, computed once per case ----
_REF = {}
UNRESOLVED = 1e-20     # of the row's largest entry: the 40-digit refinement stops at 1e-25 of it


def group_errors(x, want, groups, floor):
    """Scaled error of one sensitivity row, group by group (SR.scaled_error's scaling).  A group the yardstick resolves as exactly
    zero must be exactly zero.  A group whose yardstick lies below UNRESOLVED of the row's largest entry is identically zero in exact
    arithmetic (the branch currents of a ladder at 0 Hz with respect to a resistor that only a controlled source feeds): what the
    yardstick holds there is its own rounding, so the group is held to the absolute bound floor[g] instead — 1e-8 of the smallest
    resolved max|dx/dp| of that group among the case's parameters at that frequency, the rule of smallsignal_cases.zero_slot_bound."""
    top = np.max(np.abs(want))
    worst = 0.0
    for gi, g in enumerate(groups):
        g = np.asarray(g, dtype=int)
        if g.size == 0:
            continue
        scale, err = np.max(np.abs(want[g])), np.max(np.abs(x[g] - want[g]))
        if scale == 0.0:
            worst = max(worst, 0.0 if err == 0.0 else np.inf)
        elif scale <= UNRESOLVED * top:
            worst = max(worst, 0.0 if np.max(np.abs(x[g])) <= floor[gi] else np.inf)
        else:
            worst = max(worst, err / scale)
    return float(worst)


def linear_reference(key, c, names, freqs, groups=None):
    """{want[f][k][n_mna], e[f][k], e_cpu, tol, floor[f][g]} of a case."""
    key = (key, tuple(names), tuple(float(f) for f in freqs))
    if key in _REF:
        return _REF[key]
    slots = [c.slots[slot_of(c, nm)] for nm in names]
    groups = groups or SR.unit_groups(c)
    want, e, floors = [], [], []
    for f in freqs:
        w = 2.0 * np.pi * f
        _, s = AR.ac_sens(c, slots, w)
        _, g = AR.fd_ac_sens(c, slots, w)
        floor = []
        for grp in groups:
            grp = np.asarray(grp, dtype=int)
            m = [np.max(np.abs(s[k][grp])) for k in range(len(names)) if grp.size and np.max(np.abs(s[k][grp])) > UNRESOLVED * np.max(np.abs(s[k]))]
            floor.append(1e-8 * min(m) if m else 0.0)
        want.append(s)
        floors.append(floor)
        e.append([group_errors(g[k], s[k], groups, floor) for k in range(len(names))])
    e_cpu = float(np.max(e))
    out = dict(want=np.array(want), e=np.array(e), e_cpu=e_cpu, tol=AR.tolerance(e_cpu), floor=floors, groups=groups)
    out["want"].setflags(write=False)
    _REF[key] = out
    return out


def check_linear(what, sens, r, freqs, names):
    """sens[n_freq][n_par][n_mna] against the yardstick; returns the worst scaled error."""
    assert sens.shape == r["want"].shape and not np.isnan(sens).any(), what
    worst = 0.0
    for fi in range(len(freqs)):
        for k in range(len(names)):
            err = group_errors(sens[fi][k], r["want"][fi][k], r["groups"], r["floor"][fi])
            assert err <= r["tol"], (what, freqs[fi], names[k], err, r["tol"])
            worst = max(worst, err)
    print("%s: %d parameters x %d frequencies: GPU error %.2e, e_cpu %.2e, tolerance %.2e" % (what, len(names), len(freqs), worst, r["e_cpu"], r["tol"]))
    return worst


def run(e, c, names, freqs, o=None):
    ids = [slot_of(c, nm) for nm in names]
    return e.ac_sens(ids, freqs, o or opts(c, e.n_samples))


# ---- 1. linear shape edges ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 96])
def test_every_element_of_a_ladder_up_to_96_unknowns(E, monkeypatch, n):
    """acsens_solve_kernel<64>, all elements as parameters (133 at 96 unknowns: fifteen panels of nine columns), one of them alone,
    and — where ch_ac does both — the fused path and the forced sparse path.  Two frequencies at 96 unknowns keep the 40-digit
    yardstick of 133 parameters within seconds."""
    c = cases.ladder(n)
    names, f = element_names(c), (F2 if n == 96 else F3)
    ids = [slot_of(c, nm) for nm in names]        # declared before the engine circuit is built
    r = linear_reference(("ladder", n), c, names, f)
    e = E(c)
    rc, x, ds, s, status, st = run(e, c, names, f)
    info = e.info()
    assert rc == 0, e.ctx.last_error()
    assert info["n_unknowns"] == n and info["path"] == (1 if n <= 64 else 2)
    check_linear("ladder(%d)" % n, s[0], r, f, names)
    # at 0 Hz a capacitance or an inductance does not enter Y at all: exactly 0 + 0j
    for k, nm in enumerate(names):
        if c.dev_kind[c.dev_names.index(nm)] in (DEV_C, DEV_L):
            assert not s[0][0][k].any(), nm
    # one parameter alone: the bits of its column in the full call
    k1 = len(names) // 2
    rc1, x1, ds1, s1, _, _ = run(E(c), c, [names[k1]], f)
    assert rc1 == 0 and np.array_equal(s1[0][:, 0], s[0][:, k1]) and np.array_equal(x1, x)
    if n <= 64:
        def again():
            e2 = E(c)
            return run(e2, c, names, f) + (e2.info(),)
        rc2, x2, ds2, s2, _, _, info2 = forced_sparse(monkeypatch, again)
        assert rc2 == 0 and info2["path"] == 2 and info2["n_unknowns"] == n
        check_linear("ladder(%d) forced sparse" % n, s2[0], r, f, names)


@pytest.mark.parametrize("n", [97, 256, 257])
def test_ladders_on_the_global_workspace(E, n):
    """acsens_solve_kernel<256>: 36 parameters spread over the elements (two panels: 32 + 4), one alone.  Not all 360 elements: the
    40-digit yardstick of a 257-unknown system costs 50 ms per parameter and frequency."""
    c = cases.ladder(n)
    names, f = spread(element_names(c), 36), FL
    ids = [slot_of(c, nm) for nm in names]
    r = linear_reference(("ladder", n), c, names, f)
    e = E(c)
    rc, x, ds, s, status, st = run(e, c, names, f)
    assert rc == 0, e.ctx.last_error()
    assert e.info()["n_unknowns"] == n and e.info()["path"] == 2
    check_linear("ladder(%d)" % n, s[0], r, f, names)
    for k, nm in enumerate(names):
        if c.dev_kind[c.dev_names.index(nm)] in (DEV_C, DEV_L):
            assert not s[0][0][k].any(), nm
    k1 = 17
    rc1, x1, ds1, s1, _, _ = run(E(c), c, [names[k1]], f)
    assert rc1 == 0 and np.array_equal(s1[0][:, 0], s[0][:, k1])


PIVOT_CASES = [("low", cases.FREQS[:2], {"rl", "gy1", "gy2", "cp", "rm"}), ("high", cases.FREQS[2:], {"rl"})]


def pivot_names(c, without):
    return [nm for nm in element_names(c) if nm not in without]


def test_pivoting_circuit(E):
    """pivot_torture, every element but those whose derivative is structurally zero or nearly so — where -dY x is a difference of
    node voltages that are equal in exact arithmetic, and the numpy version of the method is itself off by more than 1e-7 (measured:
    rl, which closes a loop of two inductors and carries no current below the GHz range, at every frequency; at 0 Hz and 1 mHz
    also the gyrator gains, cp and rm, which hang on capacitors and inductors alone there).  0 Hz and 1 mHz are the frequencies
    at which seven rows have a zero or 1e-8 diagonal."""
    c = cases.pivot_torture()
    for tag, f, without in PIVOT_CASES:
        names = pivot_names(c, without)
        ids = [slot_of(c, nm) for nm in names]
    for tag, f, without in PIVOT_CASES:
        names = pivot_names(c, without)
        r = linear_reference(("pivot", tag), c, names, f)
        e = E(c)
        rc, x, ds, s, status, st = run(e, c, names, f)
        assert rc == 0, e.ctx.last_error()
        check_linear("pivot_torture " + tag, s[0], r, f, names)


# ---- 2. independent blocks, three samples ----
def test_blocks_do_not_see_each_other(E):
    c = cases.blocks()
    names = ["ur", "vr1", "wl", "xrs3", "yc7", "yrs2"]     # one element of every block (two of the last)
    owner = [0, 1, 2, 3, 4, 4]
    ids = [slot_of(c, nm) for nm in names]
    f = F3
    sw_ids, sw_vals = c.sweep
    e = E(c)
    e.set_samples(3)
    e.set_params(sw_ids, sw_vals)
    rc, x, ds, s, status, st = run(e, c, names, f)
    assert rc == 0, e.ctx.last_error()
    assert e.info()["n_components"] == 5
    rows = {k: [c.mna_index("v", nm) for nm in c.block_nodes[k]] + [c.mna_index("i", nm) for nm in c.block_branches[k]] for k in range(5)}
    for smp in range(3):
        for k, own in enumerate(owner):
            for b in range(5):
                if b != own:
                    assert not s[smp][:, k, rows[b]].any(), (smp, names[k], b)     # exactly 0 + 0j
        assert not s[smp][:, :, rows[0]].any() and not x[smp][:, rows[0]].any()  # the undriven block
    # sample 1 against the yardstick at its own values, and bit for bit against a one-sample call
    c1 = cases.at_params(c, {sw_ids[0]: sw_vals[0][1], sw_ids[1]: sw_vals[1][1]})
    r = linear_reference("blocks-s1", c1, names, f, cases.block_groups(c1))
    check_linear("blocks, sample 1", s[1], r, f, names)
    e1 = E(c)
    e1.set_samples(1)
    e1.set_params(sw_ids, [[v[1]] for v in sw_vals])
    rc1, x1, ds1, s1, _, _ = run(e1, c, names, f)
    assert rc1 == 0 and np.array_equal(s1[0], s[1]) and np.array_equal(x1[0], x[1]) and np.array_equal(ds1[0], ds[1], equal_nan=True)


# ---- 3. nonlinear: the oracle yardstick ----
AMP_SLOTS = ["rd", "vdd", ("rb1", "m"), ("m1", "w"), ("m1", "l"), ("nfet_06v0", "vth0"), "temp", "co"]
AMP_FREQS = np.array([1e2, 1e4, 1e6, 1e7, 1e8])     # across the input high-pass (kHz) and the output pole (MHz)
ORA = dict(abstol=1e-12)


def ac_yardstick(O, c, slots, freqs, steps=None, abstol=1e-12):
    """d x_ac / d p [n_freq][n_slots][n_mna] from the oracle alone: central differences of full Oracle.ac solves (each with its own
    operating point, oracle DC at `abstol`) at two relative steps — 1e-3 and 5e-4 unless steps[slot] says otherwise —
    Richardson-extrapolated r = (4 y2 - y1) / 3.  Returns (r, est[n_slots][n_freq], x, xdc): est is the yardstick's own estimate
    max|y2 - r| / max|r|, which `admit` holds to 1e-7."""
    o = O(c)
    rc, xb, _ = o.dc(dc_opts(abstol=abstol))
    assert rc == 0

    def solve():
        rc, x = o.ac(freqs, dc_opts(x0=xb, abstol=abstol))
        assert rc == 0
        return x

    x0 = solve()
    out, est = [], []
    for s in slots:
        p = base_value(c, s)
        assert math.isfinite(p) and p != 0.0
        y = []
        for rel in (steps or {}).get(s, (1e-3, 5e-4)):
            h = rel * abs(p)
            o.set_param(s, p + h)
            xp = solve()
            o.set_param(s, p - h)
            xm = solve()
            y.append((xp - xm) / (2.0 * h))
        o.set_param(s, p)
        r = (4.0 * y[1] - y[0]) / 3.0
        est.append([np.max(np.abs(y[1][fi] - r[fi])) / np.max(np.abs(r[fi])) for fi in range(len(freqs))])
        out.append(r)
    r = np.transpose(np.array(out), (1, 0, 2))
    r.setflags(write=False)
    return r, np.array(est), x0, xb


def admit(names, freqs, est):
    """A slot whose yardstick does not know itself to 1e-7 is refused — loudly."""
    print("yardstick's own estimates: " + ", ".join("%s %.1e" % (nm, e.max()) for nm, e in zip(names, est)))
    for nm, e in zip(names, est):
        assert e.max() <= 1e-7, "slot %r refused: the yardstick's own estimate is %.2e at %g Hz" % (nm, e.max(), freqs[int(np.argmax(e))])


def assert_close_ac(s, r, names, freqs, what, tol=1e-6, admitted=None):
    """per frequency and slot: max|s - r| <= tol * max|r| over the MNA rows the engine reports; returns the errors [n_slots].
    admitted[n_slots][n_freq]: the (slot, frequency) pairs the yardstick is admitted for (None: all)."""
    worst = np.zeros(len(names))
    for fi in range(len(freqs)):
        for k in range(len(names)):
            if admitted is not None and not admitted[k][fi]:
                continue
            ok = ~np.isnan(s[fi][k])
            assert ok.any()
            scale = np.max(np.abs(r[fi][k][ok]))
            err = np.max(np.abs(s[fi][k][ok] - r[fi][k][ok]))
            assert err <= tol * scale, (what, names[k], freqs[fi], err / scale)
            worst[k] = max(worst[k], err / scale)
    seen = [admitted is None or any(admitted[k]) for k in range(len(names))]
    print(what + ": " + ", ".join("%s %s" % (nm, "%.2e" % w if ok else "refused") for nm, w, ok in zip(names, worst, seen)))
    return worst


FINE = (2e-5, 1e-5)
AMP_FINE_STEPS = {nm: ((2e-4, 1e-4) if nm == "co" else FINE) for nm in AMP_SLOTS}


@pytest.fixture(scope="module")
def amp(O):
    """The amplifier with its slots declared and a yardstick that passes its own admission: oracle DC at abstol 1e-14 and the steps
    2e-5 / 1e-5 (2e-4 / 1e-4 for co, whose derivative at 100 Hz is 1e-7 of the others' and drowns in rounding at the smaller
    step).  Measured on the CPU: estimates 1e-12 .. 7.6e-8, the extrapolated values of two successive step pairs agree to 2e-9."""
    c = amp_circuit()
    ids = [slot_of(c, nm) for nm in AMP_SLOTS]
    r, est, x0, xb = ac_yardstick(O, c, ids, AMP_FREQS, {i: AMP_FINE_STEPS[nm] for i, nm in zip(ids, AMP_SLOTS)}, abstol=1e-14)
    admit(AMP_SLOTS, AMP_FREQS, est)
    return c, ids, r, x0, xb


def both_paths(E, monkeypatch, c, ids, r, names, what, admitted=None):
    e = E(c)
    rc, x, ds, s, status, st = e.ac_sens(ids, AMP_FREQS, dc_opts(abstol=1e-12))
    assert rc == 0, e.ctx.last_error()
    assert e.info()["path"] != 2
    assert_close_ac(s[0], r, names, AMP_FREQS, what + ", fused path", admitted=admitted)

    def again():
        e2 = E(c)
        return e2.ac_sens(ids, AMP_FREQS, dc_opts(abstol=1e-12)) + (e2.info(),)
    rc2, x2, ds2, s2, _, _, info2 = forced_sparse(monkeypatch, again)
    assert rc2 == 0 and info2["path"] == 2
    assert_close_ac(s2[0], r, names, AMP_FREQS, what + ", sparse path", admitted=admitted)


# (slot, frequency) pairs of AMP_SLOTS x AMP_FREQS at which the yardstick with steps 1e-3 / 5e-4 knows itself to 1e-7
COARSE_ADMITTED = {"temp": [1e2, 1e4, 1e6, 1e8], "co": [1e2, 1e4, 1e6]}


def test_amplifier_matches_the_oracle_yardstick(E, O, monkeypatch):
    """The yardstick with the steps 1e-3 and 5e-4, oracle DC at abstol 1e-12, own estimate <= 1e-7 per slot and frequency,
    tolerance 1e-6.  The amplifier's response is too curved in most of its parameters for those steps.  Measured with the oracle
    alone, max|y2 - r| / max|r| at 100 Hz, 10 kHz, 1 MHz, 10 MHz, 100 MHz:
        rd 1.9e-5 .. 4.6e-5, vdd 8.2e-5 .. 1.9e-4, rb1.m 4.1e-5 .. 7.6e-5, m1.w 1.3e-5 .. 2.8e-5, m1.l 5.3e-6 .. 2.1e-5,
        vth0 1.4e-5 .. 3.1e-5: refused at every frequency;
        temp 1.9e-8, 1.9e-8, 7.1e-8, 2.5e-7, 7.9e-8: refused at 10 MHz;   co 3.3e-9, 3.3e-11, 5.4e-9, 1.7e-7, 2.5e-7: refused from 10 MHz.
    The refusals are not silent: the test asserts that exactly the pairs of COARSE_ADMITTED pass the rule — a pair that starts or
    stops passing fails the test — and compares the engine on those.  The refused slots, rd and vdd with their bias shift among
    them, are compared in test_amplifier_matches_a_finer_yardstick, whose steps pass the same rule for every slot and frequency."""
    c = amp_circuit()
    ids = [slot_of(c, nm) for nm in AMP_SLOTS]
    r, est, x0, xb = ac_yardstick(O, c, ids, AMP_FREQS)
    for nm, e in zip(AMP_SLOTS, est):
        print("yardstick's own estimates, %s: %s" % (nm, " ".join("%.1e" % v for v in e)))
    want = np.array([[f in COARSE_ADMITTED.get(nm, []) for f in AMP_FREQS] for nm in AMP_SLOTS])
    assert np.array_equal(est <= 1e-7, want), (est <= 1e-7)
    both_paths(E, monkeypatch, c, ids, r, AMP_SLOTS, "amplifier, steps 1e-3 / 5e-4", admitted=want)


def test_amplifier_matches_a_finer_yardstick(E, amp, monkeypatch):
    """Tolerance 1e-6 as above, against the admitted yardstick of the `amp` fixture.  Measured on the MI355X, the same on both paths:
    rd 4.5e-10, vdd 5.7e-10, rb1.m 7.8e-10, m1.w 6.5e-10, m1.l 7.8e-10, vth0 7.8e-10, temp 8.9e-10, co 5.6e-8."""
    c, ids, r, x0, xb = amp
    both_paths(E, monkeypatch, c, ids, r, AMP_SLOTS, "amplifier, finer yardstick")


def test_the_explicit_term_alone_misses_the_yardstick(O, amp):
    """With the oracle alone: Y^-1 (-dY/dp|x* x), the formula WITHOUT the bias shift, is off by more than 100 tolerances for rd and
    vdd — so a result within tolerance proves that the state term is there.  G = J(alpha0 = 0), C = J(alpha0 = 1) - G from
    Oracle.eval at the fixed operating point; dY/dp by central differences through Oracle.set_param at that same point."""
    c, ids, r, x0, xb = amp
    o = O(c)
    xop = np.nan_to_num(xb)

    def gc():
        _, _, g = o.eval(xop, 0.0, 0.0, 0)
        _, _, g1 = o.eval(xop, 0.0, 1.0, 0)
        return g, g1 - g

    g0, c0 = gc()
    for k, nm in enumerate(AMP_SLOTS[:2]):
        p = base_value(c, ids[k])
        h = 1e-4 * abs(p)
        o.set_param(ids[k], p + h)
        gp, cp = gc()
        o.set_param(ids[k], p - h)
        gm, cm = gc()
        o.set_param(ids[k], p)
        for fi, f in enumerate(AMP_FREQS):
            w = 2.0 * np.pi * f
            y = g0 + 1j * w * c0
            dy = ((gp - gm) + 1j * w * (cp - cm)) / (2.0 * h)
            s_exp = np.linalg.solve(y, -dy @ x0[fi])
            miss = np.max(np.abs(s_exp - r[fi][k])) / np.max(np.abs(r[fi][k]))
            assert miss > 100 * 1e-6, (nm, f, miss)


def test_verilog_a_slot(E, O):
    """The diode of test_verilog_a_parameter_slots behind a resistor, an AC magnitude on the source: IS moves the small-signal
    conductance through the operating point AND explicitly."""
    c = Circuit(gmin=1e-12)
    c.V("v1", "in", 0, dc=1.5, ac=1.0)
    c.R("r1", "in", "a", 1e3)
    c.VA("d1", "va_diode", ["a", 0], {"IS": 1e-13, "RS": 2.0})
    names = [("d1", "is")]
    ids = [slot_of(c, nm) for nm in names]
    f = np.array([1e3, 1e8])
    r, est, _, _ = ac_yardstick(O, c, ids, f)
    admit(names, f, est)          # 9.0e-8 at both frequencies
    e = E(c)
    rc, x, ds, s, status, st = e.ac_sens(ids, f, dc_opts(abstol=1e-12))
    assert rc == 0, e.ctx.last_error()
    assert_close_ac(s[0], r, names, f, "diode")


# ---- 4. frequency chunks ----
def test_two_frequency_chunks(E):
    """chunk_ladder: 302 unknowns, 2 samples x 400 frequencies, 3 parameters: the workspace cap admits 362 frequencies per launch.
    The second launch's results are those of a call on its frequencies alone, bit for bit; two frequencies (one per launch)
    against the yardstick."""
    c = cases.chunk_ladder()
    names = ["r8", "c150", "r299"]
    ids = [slot_of(c, nm) for nm in names]
    cut = 362

    def engine():
        e = E(c)
        e.set_samples(cases.CHUNK_SAMPLES)
        e.set_params([c.sweep[0]], [c.sweep[1]])
        return e
    e = engine()
    rc, x, ds, s, status, st = run(e, c, names, c.freqs)
    assert rc == 0, e.ctx.last_error()
    assert e.info()["n_unknowns"] == 302 and not np.isnan(s).any()
    rc2, x2, ds2, s2, _, _ = run(engine(), c, names, c.freqs[cut:])
    assert rc2 == 0 and np.array_equal(s2, s[:, cut:]) and np.array_equal(x2, x[:, cut:])
    fi = [cut - 1, cut]
    for smp in range(cases.CHUNK_SAMPLES):
        cs = cases.at_params(c, {c.sweep[0]: c.sweep[1][smp]})
        r = linear_reference(("chunk", smp), cs, names, c.freqs[fi])
        check_linear("chunk_ladder sample %d" % smp, s[smp][fi], r, c.freqs[fi], names)


# ---- 5. consistency with the other entry points; nothing moved ----
def test_consistent_with_ch_dc_sens_and_ch_ac_and_leaves_the_circuit_alone(E, amp):
    c, ids, r, x0, xb = amp
    o = dc_opts(abstol=1e-12)
    e = E(c)
    rc_a, xdc_a, _, _ = e.dc(o)
    rc_b, xac_b, _ = e.ac(AMP_FREQS, o)
    rc, x, ds, s, status, st = e.ac_sens(ids, AMP_FREQS, o)
    rc_c, xdc_c, _, _ = e.dc(o)
    rc_d, xac_d, _ = e.ac(AMP_FREQS, o)
    rc_e, xs, sd, _, _ = e.dc_sens(ids, o)
    assert rc_a == 0 and rc_b == 0 and rc == 0 and rc_c == 0 and rc_d == 0 and rc_e == 0
    assert np.array_equal(xdc_a, xdc_c, equal_nan=True) and np.array_equal(xac_b, xac_d, equal_nan=True)
    assert np.array_equal(x, xac_b, equal_nan=True)          # x_ac_out: the bits of ch_ac
    assert np.array_equal(ds, sd, equal_nan=True)            # dc_sens_out: the bits of ch_dc_sens
    assert np.any(ds != 0.0) and status[0] == 0


# ---- 6. errors and failures ----
def rc_cell(r=1.3e3, cap=2.2e-9):
    c = Circuit()
    c.V("vin", "a", 0, dc=0.0, ac=1.0)
    c.R("r1", "a", "b", r)
    c.C("c1", "b", 0, cap)
    return c


def test_errors_are_return_codes(E):
    c = rc_cell()
    ids = [c.slot("r1")]
    e = E(c)
    o = opts(c)
    f = np.array([1e3])
    for bad in ([7], [-1], [ids[0], 99]):
        rc = e.ac_sens(bad, f, o)[0]
        assert rc == -1 and "slot" in e.ctx.last_error()
    for bad_f in ([-1.0], [1e3, math.nan], [math.inf]):
        rc = e.ac_sens(ids, np.array(bad_f), o)[0]
        assert rc == -1 and "frequenc" in e.ctx.last_error()
    import ctypes as C
    i32 = (C.c_int32 * 1)(ids[0])
    ff = (C.c_double * 1)(1e3)
    out = (C.c_double * (2 * c.n_mna))()
    assert e.L.ch_ac_sens(e.h, o, 0, i32, None, 1, ff, None, None, out, None, None) == -1      # n_par = 0
    assert e.L.ch_ac_sens(e.h, o, 1, i32, None, 1, ff, None, None, None, None, None) == -1     # no output array
    assert e.L.ch_ac_sens(e.h, o, 1, i32, None, 0, ff, None, None, out, None, None) == -1      # no frequency
    assert e.L.ch_ac_sens(e.h, o, 1, i32, None, 1, ff, None, None, out, None, None) == 0       # the optional outputs may be NULL
    with pytest.raises(CedarError):
        ac_sens(c, ["nosuchdevice"])


def test_a_failed_sample_is_reported_and_the_others_are_served(E):
    """Sample 1 has no operating point (an infinite resistor leaves a current source on a node nothing else holds): NaN rows and
    its ch_dc status; sample 0 has the bits of a one-sample call."""
    c = rc_cell()
    c.I("i1", "n", 0, dc=1e-3)
    c.R("rn", "n", 0, 1e3)
    names = ["rn", "r1", "c1"]
    ids = [slot_of(c, nm) for nm in names]
    f = np.array([0.0, 1e5])
    o = dict(abstol=1e-12, n_restarts=2, maxiters=5)
    e = E(c)
    e.set_samples(2)
    e.set_params(ids[:1], [[1e3, math.inf]])
    rc, x, ds, s, status, st = e.ac_sens(ids, f, dc_opts(**o))
    assert rc == -3 and status[0] == 0 and status[1] != 0
    b, a = c.mna_index("v", "b"), c.mna_index("v", "a")
    assert np.isnan(s[1][:, :, b]).all() and np.isnan(x[1][:, b]).all() and np.isnan(ds[1][:, b]).all()
    e1 = E(c)
    rc1, x1, ds1, s1, status1, _ = e1.ac_sens(ids, f, dc_opts(**o))
    assert rc1 == 0 and np.array_equal(s1[0], s[0]) and np.array_equal(x1[0], x[0])
    w = 2.0 * np.pi * f[1]
    h = 1.0 / (1.0 + 1j * w * 1.3e3 * 2.2e-9)
    assert abs(s[0][1][1][b] - (-1j * w * 2.2e-9 * h * h)) <= 1e-9 * abs(w * 2.2e-9 * h * h)


# ---- 7. the Python surface ----
def test_circuit_sweep_and_mag_phase(E):
    """ac_sens(CircuitSweep) over four points: each point equals its own single call and the closed forms of the RC low-pass,
    dH/dR = -jwC H^2 and dH/dC = -jwR H^2; mag_phase_sens of them against a finite difference of |H| and arg H in R."""
    cap = 2.2e-9
    rs = [500.0, 1.3e3, 4e3, 2e4]
    cs = CircuitSweep(lambda r1=1e3: rc_cell(r1, cap), Sweep(r1=rs))
    sols = ac_sens(cs, ["r1", "c1"], abstol=1e-12)
    assert len(sols) == 4
    w = 2.0 * np.pi * np.array([1e3, 5e4, 2e6])
    for sol, p in zip(sols, cs):
        r1 = p["r1"]
        h = 1.0 / (1.0 + 1j * w * r1 * cap)
        assert np.allclose(sol.freqresp("b", w), h, rtol=1e-12, atol=0.0)
        dr, dc = sol.sens("b", "r1", w), sol.sens("b", "c1", w)
        assert np.allclose(dr, -1j * w * cap * h * h, rtol=1e-9, atol=0.0) and np.allclose(dc, -1j * w * r1 * h * h, rtol=1e-9, atol=0.0)
        assert not sol.sens("a", "r1", w).any() and sol.op.params == p and sol.op.rc == 0
        assert abs(sol.dc_sens["b", "r1"]) <= 1e-15 and sol.dc_sens.rc == 0     # no DC current through r1 (a randomised start: not exactly 0)
        one = ac_sens(rc_cell(r1, cap), ["r1", "c1"], abstol=1e-12)
        assert np.allclose(one.sens("b", "r1", w), dr, rtol=1e-12, atol=0.0) and np.allclose(one.sens("b", "c1", w), dc, rtol=1e-12, atol=0.0)
        dmag, dph = mag_phase_sens(sol.freqresp("b", w), dr)
        d = 1e-5 * r1
        hp, hm = 1.0 / (1.0 + 1j * w * (r1 + d) * cap), 1.0 / (1.0 + 1j * w * (r1 - d) * cap)
        assert np.allclose(dmag, (np.abs(hp) - np.abs(hm)) / (2 * d), rtol=1e-7, atol=0.0)
        assert np.allclose(dph, (np.angle(hp) - np.angle(hm)) / (2 * d), rtol=1e-7, atol=0.0)
    with pytest.raises(KeyError):
        sols[0].sens("b", "vin", w)
