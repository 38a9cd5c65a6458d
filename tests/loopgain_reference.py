"""A CPU yardstick for the loop-gain (stability) analysis, on top of smallsignal_reference.py (numpy stamps of the full MNA system,
every solve refined at 40 digits) and acsens_reference.py (analytic derivative stamps).  It shares nothing with the engine.

The probe is a voltage source `vprobe x y` in the loop wire, x (+) facing the side the loop signal arrives from.  Two excitations of
Y(w) = G + jwC, every other AC excitation off:
    v-run: v_x - v_y = 1, keep V2 = v_x;      i-run: probe at 0 V, unit current INTO node x (as `I 0 x ac=1`), keep I1 = i_p,
    u = V2 - I1,   T = u / (1 - u),   dT/dp = (du/dp) / (1 - u)^2,   du/dp = e_x^T dx_v/dp - e_ip^T dx_i/dp,   Y dx/dp = -(dY/dp) x.
The combination into T and dT runs in mpmath on the refined solutions; results are rounded to complex128 at the end.

Also here: the circuits of the tests (the loop of the issue, bare or with a passive R-L-C tail on node o, its three-pole version, the
ideal unilateral loop) and the independent definitions T is pinned against (the return ratio of the VCCS on the closed wire, the
two-port expression)."""
import copy

import mpmath
import numpy as np

import acsens_reference as AR
import smallsignal_cases as cases
import smallsignal_reference as SR
from cedarsim_jl_amd import Circuit

GM, RO, CO, R1, R2, CG = 2e-3, 5e3, 1e-12, 7e3, 3e3, 2e-13
PROBE = "vprobe"


def loop(tail_unknowns=0, reverse=False, three_pole=False):
    """The test loop: a VCCS gm from y pulling current out of o; Ro || Co at o; R1 from o to x; the probe x -> y; R2 || Cg at y.  Its DC
    loop gain is gm * Ro * R2 / (Ro + R1 + R2) = 2 exactly (bare).  4 unknowns: o, x, y and the probe's current.
    tail_unknowns: a passive R-L-C tail (smallsignal_cases._rlc_sections) hung on node o adds exactly that many unknowns.
    reverse: the probe is y -> x.  three_pole: two more RC lags between o and R1 (buffered by unity VCVS), so that the phase falls
    through -180 degrees: the loop the measures are taken on, with gm = 0.02 (a DC loop gain of 0.02 * 5e3 * 0.3 = 30)."""
    c = Circuit()
    c.G("gm", "o", 0, "y", 0, gain=0.02 if three_pole else GM)
    c.R("ro", "o", 0, RO)
    c.C("co", "o", 0, CO)
    src = "o"
    if three_pole:
        c.E("e1", "b1", 0, "o", 0, gain=1.0)
        c.R("rp1", "b1", "p1", 1e3)
        c.C("cp1", "p1", 0, 2e-12)
        c.E("e2", "b2", 0, "p1", 0, gain=1.0)
        c.R("rp2", "b2", "p2", 1e3)
        c.C("cp2", "p2", 0, 5e-13)
        c.E("e3", "b3", 0, "p2", 0, gain=1.0)
        src = "b3"
    c.R("r1", src, "x", R1)
    if reverse:
        c.V(PROBE, "y", "x", dc=0.0, ac=1.0)
    else:
        c.V(PROBE, "x", "y", dc=0.0, ac=1.0)
    c.R("r2", "y", 0, R2)
    c.C("cg", "y", 0, CG)
    if tail_unknowns:
        k, trailing = divmod(tail_unknowns, 3)
        cases._rlc_sections(c, np.random.default_rng(4000 + tail_unknowns), "t", "o", k, trailing)
    return c


def unilateral(gain):
    """An ideal unilateral loop: nothing but the probe at y (infinite impedance), an ideal -A from y at x.  T = A."""
    c = Circuit()
    c.E("ea", "x", 0, "y", 0, gain=-float(gain))
    c.V(PROBE, "x", "y", dc=0.0, ac=1.0)
    return c


def probe_rows(c, probe=PROBE):
    """(MNA row of v_x, MNA row of the probe's branch current)."""
    i = c.dev_names.index(probe)
    return c.dev_node[i][0] - 1, c.mna_index("i", probe)


def excitations(c, omega, probe=PROBE):
    """(Y, b_v, b_i): the probe at 1 V with every other excitation off; a unit current into node x with the probe at 0 V."""
    d = copy.copy(c)
    d.source_ac = [0.0] * len(c.source_ac)
    d.source_ac[c.dev_ipar[c.dev_names.index(probe)][0]] = 1.0
    Y, bv = SR.mna(d, omega)
    bi = np.zeros_like(bv)
    bi[probe_rows(c, probe)[0]] = 1.0
    return Y, bv, bi


def loop_gain(c, freqs_hz, probe=PROBE, slots=()):
    """(T[n_freq], dT[n_freq][n_slots], T_lapack[n_freq]): the yardstick, and T formed in plain double precision from LAPACK solves
    (whose error against the yardstick is the e_cpu of the GPU tests).  slots: (kind, a, b) entries of Circuit.slots."""
    rx, ri = probe_rows(c, probe)
    T, dT, Tl = [], [], []
    for f in freqs_hz:
        w = 2.0 * np.pi * float(f)
        Y, bv, bi = excitations(c, w, probe)
        _, xv, _ = SR.solve(Y, bv)
        _, xi, _ = SR.solve(Y, bi)
        lv, li = np.linalg.solve(Y, bv), np.linalg.solve(Y, bi)
        ul = lv[rx] - li[ri]
        Tl.append(ul / (1.0 - ul))
        with mpmath.workdps(SR.MP_DIGITS):
            u = xv[rx] - xi[ri]
            T.append(complex(u / (1 - u)))
            row = []
            for slot in slots:
                dY, db = AR.derivative_stamp(c, slot, w)
                assert not db.any(), "a loop-gain slot must not move a right-hand side"
                du = mpmath.mpc(0)
                for x, r, sign in ((xv, rx, 1), (xi, ri, -1)):
                    if dY.any():
                        rhs = np.array([complex(-mpmath.fsum(SR._mpc(dY[q, j]) * x[int(j)] for j in np.nonzero(dY[q])[0])) for q in range(len(bv))])
                        _, dx, _ = SR.solve(Y, rhs)
                        du += sign * dx[r]
                row.append(complex(du / (1 - u) ** 2))
            dT.append(row)
    return np.array(T), np.array(dT, dtype=np.complex128).reshape(len(freqs_hz), len(slots)), np.array(Tl)


def return_ratio(c, freqs_hz, vccs="gm"):
    """The return ratio of the VCCS on the CLOSED wire (the probe is a 0 V short): the VCCS is taken out, a unit current is driven the
    way its output drives it, and -gm * (its controlling voltage) comes back."""
    k = c.dev_names.index(vccs)
    a, b, p, q = c.dev_node[k][:4]
    g = c.dev_par[k][0] * c.dev_mult[k]
    d = copy.deepcopy(c)
    d.dev_par[k][0] = 0.0
    out = []
    for f in freqs_hz:
        Y, _ = SR.mna(d, 2.0 * np.pi * float(f))
        rhs = np.zeros(Y.shape[0], dtype=np.complex128)
        if a:
            rhs[a - 1] -= 1.0     # a unit current leaves node a and enters node b
        if b:
            rhs[b - 1] += 1.0
        _, x, _ = SR.solve(Y, rhs)
        with mpmath.workdps(SR.MP_DIGITS):
            vc = (x[p - 1] if p else mpmath.mpc(0)) - (x[q - 1] if q else mpmath.mpc(0))
            out.append(complex(-g * vc))
    return np.array(out)


def two_port(c, freqs_hz, probe=PROBE):
    """Tian's loop gain from the two-port the rest of the circuit presents at (x, y), [i_x; i_y] = Yp [v_x; v_y], currents INTO the
    rest of the circuit: T = (y12 - y21) / (y11 + y22 + 2 y21).  Yp = I V^-1 from the two runs (`two_port_matrix`)."""
    out = []
    for f in freqs_hz:
        yp = two_port_matrix(c, f, probe)
        out.append((yp[0, 1] - yp[1, 0]) / (yp[0, 0] + yp[1, 1] + 2.0 * yp[1, 0]))
    return np.array(out)


def two_port_matrix(c, f, probe=PROBE, inject_at_y=False):
    """Yp at one frequency.  The probe's current i_p flows from x through it to y: it leaves the rest of the circuit at x and enters it
    at y.  inject_at_y: the unit current of the i-run goes into y instead of x (the same Yp comes out)."""
    i = c.dev_names.index(probe)
    x, y = c.dev_node[i][0] - 1, c.dev_node[i][1] - 1
    ri = c.mna_index("i", probe)
    Y, bv, bi = excitations(c, 2.0 * np.pi * float(f), probe)
    if inject_at_y:
        bi = np.zeros_like(bi)
        bi[y] = 1.0
    sv, _, _ = SR.solve(Y, bv)
    si, _, _ = SR.solve(Y, bi)
    V = np.array([[sv[x], si[x]], [sv[y], si[y]]])
    inj = (0.0, 1.0) if inject_at_y else (1.0, 0.0)
    I = np.array([[-sv[ri], inj[0] - si[ri]], [sv[ri], inj[1] + si[ri]]])
    return I @ np.linalg.inv(V)


def errors(T, ref):
    """|T - T_ref| / max(1, max|T_ref|), the worst frequency."""
    return float(np.max(np.abs(np.asarray(T) - np.asarray(ref))) / max(1.0, float(np.max(np.abs(ref)))))


_CACHE = {}


def shape_case(n):
    """(circuit, T_ref[n_freq], e_cpu, tolerance) of the loop with exactly n unknowns in the probe's block, over smallsignal_cases.FREQS,
    computed once per process.  tolerance: smallsignal_cases.tolerance(e_cpu) = max(1e-12, 32 e_cpu); e_cpu > 1e-11 is refused."""
    if n not in _CACHE:
        c = loop(n - 4)
        T, _, Tl = loop_gain(c, cases.FREQS)
        e_cpu = errors(Tl, T)
        assert e_cpu <= cases.E_CPU_MAX, "mis-designed case: e_cpu = %.3e at %d unknowns" % (e_cpu, n)
        T.setflags(write=False)
        _CACHE[n] = (c, T, e_cpu, cases.tolerance(e_cpu))
    return _CACHE[n]


def fd_loop_gain_sens(c, freqs_hz, slots, probe=PROBE):
    """dT[n_freq][n_slots] by the ENGINE'S METHOD in numpy double precision: dY from differences of the numpy stamps at sens_step's
    steps (acsens_reference.step_of), plain LAPACK solves, two adjoint vectors, two bilinear forms per slot.  Its error against the
    yardstick is the e_cpu the tolerance of the sensitivity tests derives from."""
    rx, ri = probe_rows(c, probe)
    out = []
    for f in freqs_hz:
        w = 2.0 * np.pi * float(f)
        Y, bv, bi = excitations(c, w, probe)
        xv, xi = np.linalg.solve(Y, bv), np.linalg.solve(Y, bi)
        ex, ei = np.zeros(len(bv), dtype=np.complex128), np.zeros(len(bv), dtype=np.complex128)
        ex[rx], ei[ri] = 1.0, 1.0
        lx, li = np.linalg.solve(Y.T, ex), np.linalg.solve(Y.T, ei)
        u = xv[rx] - xi[ri]
        row = []
        for slot in slots:
            central, h = AR.step_of(c, slot)
            Yp, _ = SR.mna(AR._moved(c, slot, h), w)
            Ym = SR.mna(AR._moved(c, slot, -h), w)[0] if central else Y
            dY = (Yp - Ym) / (2.0 * h if central else h)
            row.append((-(lx @ (dY @ xv)) + li @ (dY @ xi)) / (1.0 - u) ** 2)
        out.append(row)
    return np.array(out, dtype=np.complex128).reshape(len(freqs_hz), len(slots))


UNRESOLVED, ZERO_BOUND = 1e-12, 1e-8


def sens_errors(dT, ref):
    """[n_freq][n_par]: |dT - ref| / |ref| per frequency and parameter (one row, so test_gpu_ac_sens's scaling by the row's largest entry
    is the relative error).  Where the reference is exactly zero (a capacitance at 0 Hz) the value must be exactly zero.  Where it lies
    below UNRESOLVED = 1e-12 of the parameter's largest |dT/dp| on the grid (a tail element sections away from the loop at 10 GHz: the
    response has decayed by tens of orders) no double-precision solve owes it relative digits — a normwise backward-stable LU carries
    entries that far below the solution's largest only to eps times the condition number — so the value is held to the absolute
    bound ZERO_BOUND = 1e-8 of that largest instead, the rule of test_gpu_ac_sens.group_errors."""
    dT, ref = np.asarray(dT), np.asarray(ref)
    out = np.zeros(ref.shape)
    for k in range(ref.shape[1]):
        top = float(np.max(np.abs(ref[:, k])))
        for f in range(ref.shape[0]):
            err, scale = abs(dT[f, k] - ref[f, k]), abs(ref[f, k])
            if scale == 0.0:
                out[f, k] = 0.0 if err == 0.0 else np.inf
            elif scale <= UNRESOLVED * top:
                out[f, k] = 0.0 if abs(dT[f, k]) <= ZERO_BOUND * top else np.inf
            else:
                out[f, k] = err / scale
    return out
