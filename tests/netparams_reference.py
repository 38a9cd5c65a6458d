"""A CPU yardstick for the N-port network analysis, on top of smallsignal_reference.py (numpy stamps of the full MNA system, every
solve refined at 40 digits) and acsens_reference.py (analytic derivative stamps).  It shares nothing with the engine.

Ports are voltage sources `vpJ a b`, numbered in the order given.  Y(w) = G + jwC, every non-port AC excitation off; run k puts 1 V on
port k and 0 V on the others.  A source's branch current flows from + through the source to -, so the current entering the network
at port j is -i_pj:
    Yp[j][k] = -x_k[row_i(j)],   y = sqrt(z0) Yp sqrt(z0),   S = (I - y)(I + y)^-1,   Z = Yp^-1,
    dYp[j][k]/dp = -dx_k/dp[row_i(j)] with Y dx_k/dp = -(dY/dp) x_k (the direct method: one refined solve per slot and port),
    dS/dp = -1/2 (I + S)(sqrt(z0) dYp/dp sqrt(z0))(I + S),   dZ/dp = -Z (dYp/dp) Z.
The combination into S, Z and their derivatives runs in mpmath on the refined solutions; results are rounded to complex128 at the end.

Also here: the circuits of the tests and the error rules."""
import copy

import mpmath
import numpy as np

import acsens_reference as AR
import loopgain_reference as LG
import smallsignal_cases as cases
import smallsignal_reference as SR
from cedarsim_jl_amd import Circuit

KINDS = "SYZ"


# ---- circuits ----
def series_r(r=50.0):
    """A series resistor between two ports, nothing to ground: S11 = 1/3, S21 = 2/3 at z0 = r = 50; Yp = [[1, -1], [-1, 1]] / r is
    singular, so Z does not exist."""
    c = Circuit()
    c.V("vp1", "p1", 0, dc=0.0, ac=1.0)
    c.V("vp2", "p2", 0, dc=0.0, ac=1.0)
    c.R("rs", "p1", "p2", r)
    return c, ("vp1", "vp2")


def star3(r=50.0 / 3.0):
    """Three resistors of z0 / 3 in a star: the matched resistive power splitter, Sjj = 0, Sjk = 1/2."""
    c = Circuit()
    for j in (1, 2, 3):
        c.V("vp%d" % j, "p%d" % j, 0, dc=0.0, ac=1.0)
        c.R("r%d" % j, "p%d" % j, "m", r)
    return c, ("vp1", "vp2", "vp3")


RIN, GM, RO = 2e3, 5e-3, 8e3


def unilateral():
    """Rin at port 1, a VCCS gm (controlled by port 1) pulling its current out of port 2's node, Ro at port 2:
    Yp = [[1/Rin, 0], [gm, 1/Ro]]."""
    c = Circuit()
    c.V("vp1", "p1", 0, dc=0.0, ac=1.0)
    c.V("vp2", "p2", 0, dc=0.0, ac=1.0)
    c.R("rin", "p1", 0, RIN)
    c.G("gm", "p2", 0, "p1", 0, gain=GM)
    c.R("ro", "p2", 0, RO)
    return c, ("vp1", "vp2")


def butterworth(z0=50.0, fc=1e8, rser=0.0):
    """Third-order Butterworth low-pass between two ports of z0: shunt C = 1 / (z0 wc), series L = 2 z0 / wc, shunt C.
    |S21|^2 = 1 / (1 + (f / fc)^6); lossless and reciprocal: S^H S = I, S = S^T.  rser > 0 puts that resistance in series with the
    inductor: without it the inductor shorts the two ideal port sources at DC, a source-inductor loop whose operating point has a
    singular Jacobian (the numpy stamps do not mind, an engine does)."""
    wc = 2.0 * np.pi * fc
    c = Circuit()
    c.V("vp1", "p1", 0, dc=0.0, ac=1.0)
    c.V("vp2", "p2", 0, dc=0.0, ac=1.0)
    c.C("c1", "p1", 0, 1.0 / (z0 * wc))
    c.L("l2", "p1", "x" if rser > 0.0 else "p2", 2.0 * z0 / wc)
    if rser > 0.0:
        c.R("rser", "x", "p2", rser)
    c.C("c3", "p2", 0, 1.0 / (z0 * wc))
    return c, ("vp1", "vp2")


def stage(n=5):
    """The VCCS stage with an internal node, a bilateral two-port with exactly n >= 5 unknowns (p1, n, p2 and the two port
    currents; a passive R-L-C tail of smallsignal_cases._rlc_sections on the internal node adds the rest): Rin at port 1, Rg from
    port 1 to the internal node n with Cg to ground, the VCCS gm controlled by n pulling current out of port 2, Ro || Co at port 2,
    and Rf || Cf from n to port 2 (feedback: no entry of Yp is structurally zero)."""
    c = Circuit()
    c.V("vp1", "p1", 0, dc=0.0, ac=1.0)
    c.V("vp2", "p2", 0, dc=0.0, ac=1.0)
    c.R("rin", "p1", 0, RIN)
    c.R("rg", "p1", "n", 300.0)
    c.C("cg", "n", 0, 2e-13)
    c.G("gm", "p2", 0, "n", 0, gain=GM)
    c.R("ro", "p2", 0, RO)
    c.C("co", "p2", 0, 1e-12)
    c.R("rf", "n", "p2", 2e4)
    c.C("cf", "n", "p2", 5e-14)
    if n > 5:
        k, trailing = divmod(n - 5, 3)
        cases._rlc_sections(c, np.random.default_rng(5000 + n), "t", "n", k, trailing)
    return c, ("vp1", "vp2")


Z0_STAGE = (50.0, 75.0)
Z0_STAR8 = (50.0, 75.0, 25.0, 100.0, 50.0, 60.0, 30.0, 120.0)


def star8(n=17):
    """Eight ports on a resistive-capacitive star with exactly n >= 17 unknowns (eight port nodes, the centre, eight port currents; a
    tail on the centre adds the rest): port j reaches the centre m through R_j || C_j and has a shunt R to ground; the centre has
    R || C to ground."""
    rng = np.random.default_rng(8008)
    c = Circuit()
    for j in range(1, 9):
        c.V("vp%d" % j, "p%d" % j, 0, dc=0.0, ac=1.0)
        c.R("ra%d" % j, "p%d" % j, "m", cases._logu(rng, 20.0, 200.0))
        c.C("ca%d" % j, "p%d" % j, "m", cases._logu(rng, 1e-13, 1e-12))
        c.R("rsh%d" % j, "p%d" % j, 0, cases._logu(rng, 100.0, 1e3))
    c.R("rm", "m", 0, 150.0)
    c.C("cm", "m", 0, 1e-12)
    if n > 17:
        k, trailing = divmod(n - 17, 3)
        cases._rlc_sections(c, np.random.default_rng(8000 + n), "t", "m", k, trailing)
    return c, tuple("vp%d" % j for j in range(1, 9))


def one_port():
    """The smallest circuit: one port on R || C, two unknowns.  Y11 = 1/R + jwC."""
    c = Circuit()
    c.V("vp1", "p1", 0, dc=0.0, ac=1.0)
    c.R("r1", "p1", 0, 80.0)
    c.C("c1", "p1", 0, 1e-12)
    return c, ("vp1",)


# ---- the yardstick ----
def port_rows(c, ports):
    """MNA row of every port's branch current."""
    return [c.mna_index("i", p) for p in ports]


def excitations(c, ports, omega):
    """(Y, B[n][P]): every port at 1 V with every other excitation off gives b, the sum of the P excitations; column k is b's entry
    in port k's branch row, alone."""
    d = copy.copy(c)
    d.source_ac = [0.0] * len(c.source_ac)
    for p in ports:
        d.source_ac[c.dev_ipar[c.dev_names.index(p)][0]] = 1.0
    Y, b = SR.mna(d, omega)
    rows = port_rows(c, ports)
    B = np.zeros((len(b), len(ports)), dtype=np.complex128)
    for k, r in enumerate(rows):
        B[r, k] = b[r]
    return Y, B


def _mp_matrix(rows):
    return mpmath.matrix([[v for v in r] for r in rows])


def _to_np(M, P):
    return np.array([[complex(M[i, j]) for j in range(P)] for i in range(P)])


def s_of_y_np(Yp, z0):
    """S of one Yp in plain double precision (numpy)."""
    rz = np.sqrt(np.asarray(z0, dtype=np.float64))
    y = rz[:, None] * Yp * rz[None, :]
    I = np.eye(len(rz))
    return (I - y) @ np.linalg.inv(I + y)


def convert_sens_np(S, Z, dYp, z0):
    rz = np.sqrt(np.asarray(z0, dtype=np.float64))
    I = np.eye(len(rz))
    dS = -0.5 * (I + S) @ (rz[:, None] * dYp * rz[None, :]) @ (I + S)
    return dS, (-Z @ dYp @ Z if Z is not None else np.full_like(dYp, np.nan))


def net_params(c, ports, z0, freqs_hz, slots=(), want_z=True):
    """The yardstick: a dict with S, Y, Z [n_freq][P][P], dS, dY, dZ [n_freq][n_slots][P][P] and S_l, Y_l, Z_l, the values formed in
    plain double precision from LAPACK solves (their error against the yardstick is the e_cpu of the GPU tests).
    slots: (kind, a, b) entries of Circuit.slots.  want_z=False leaves Z, dZ, Z_l as NaN (a singular Yp)."""
    P = len(ports)
    z0 = [float(v) for v in (np.repeat(z0, P) if np.ndim(z0) == 0 else z0)]
    rows = port_rows(c, ports)
    out = {k: [] for k in ("S", "Y", "Z", "dS", "dY", "dZ", "S_l", "Y_l", "Z_l")}
    nan = np.full((P, P), np.nan + 0j)
    for f in freqs_hz:
        w = 2.0 * np.pi * float(f)
        Y, B = excitations(c, ports, w)
        X = [SR.solve(Y, B[:, k])[1] for k in range(P)]
        xl = np.linalg.solve(Y, B)
        Yl = -xl[rows, :]
        Sl, Zl = s_of_y_np(Yl, z0), np.linalg.inv(Yl) if want_z else nan
        out["Y_l"].append(Yl), out["S_l"].append(Sl), out["Z_l"].append(Zl)
        with mpmath.workdps(SR.MP_DIGITS):
            rz = [mpmath.sqrt(mpmath.mpf(v)) for v in z0]
            Yp = _mp_matrix([[-X[k][rows[j]] for k in range(P)] for j in range(P)])
            D = mpmath.diag(rz)
            I = mpmath.eye(P)
            y = D * Yp * D
            S = (I - y) * mpmath.inverse(I + y)
            Z = mpmath.inverse(Yp) if want_z else None
            out["Y"].append(_to_np(Yp, P)), out["S"].append(_to_np(S, P)), out["Z"].append(_to_np(Z, P) if want_z else nan)
            dS_f, dY_f, dZ_f = [], [], []
            for slot in slots:
                dYm, db = AR.derivative_stamp(c, slot, w)
                assert not db.any(), "a network-parameter slot must not move a right-hand side"
                dYp = mpmath.zeros(P, P)
                if dYm.any():
                    for k in range(P):
                        rhs = np.array([complex(-mpmath.fsum(SR._mpc(dYm[q, j]) * X[k][int(j)] for j in np.nonzero(dYm[q])[0])) for q in range(Y.shape[0])])
                        if rhs.any():
                            dx = SR.solve(Y, rhs)[1]
                            for j in range(P):
                                dYp[j, k] = -dx[rows[j]]
                dY_f.append(_to_np(dYp, P))
                dS_f.append(_to_np(-(I + S) * (D * dYp * D) * (I + S) / 2, P))
                dZ_f.append(_to_np(-Z * dYp * Z, P) if want_z else nan)
            out["dS"].append(dS_f), out["dY"].append(dY_f), out["dZ"].append(dZ_f)
    nf, ns = len(freqs_hz), len(slots)
    res = {k: np.array(v, dtype=np.complex128).reshape((nf, ns, P, P) if k[0] == "d" else (nf, P, P)) for k, v in out.items()}
    for v in res.values():
        v.setflags(write=False)
    return res


def fd_net_sens(c, ports, z0, freqs_hz, slots, want_z=True):
    """{dS, dY, dZ}[n_freq][n_slots][P][P] by the ENGINE'S METHOD in numpy double precision: dY from differences of the numpy stamps at
    sens_step's steps (acsens_reference.step_of), plain LAPACK solves, P adjoint vectors, P^2 bilinear forms per slot, the conversion
    derivatives in numpy.  Its error against the yardstick is the e_cpu the tolerance of the sensitivity tests derives from."""
    P = len(ports)
    z0 = np.repeat(z0, P) if np.ndim(z0) == 0 else np.asarray(z0, dtype=np.float64)
    rows = port_rows(c, ports)
    out = {"dS": [], "dY": [], "dZ": []}
    for f in freqs_hz:
        w = 2.0 * np.pi * float(f)
        Y, B = excitations(c, ports, w)
        x = np.linalg.solve(Y, B)
        E = np.zeros_like(B)
        for j, r in enumerate(rows):
            E[r, j] = 1.0
        lam = np.linalg.solve(Y.T, E)
        Yp = -x[rows, :]
        S = s_of_y_np(Yp, z0)
        Z = np.linalg.inv(Yp) if want_z else None
        for key in out:
            out[key].append([])
        for slot in slots:
            central, h = AR.step_of(c, slot)
            Yplus, _ = SR.mna(AR._moved(c, slot, h), w)
            Yminus = SR.mna(AR._moved(c, slot, -h), w)[0] if central else Y
            dYm = (Yplus - Yminus) / (2.0 * h if central else h)
            dYp = lam.T @ dYm @ x
            dS, dZ = convert_sens_np(S, Z, dYp, z0)
            out["dY"][-1].append(dYp), out["dS"][-1].append(dS), out["dZ"][-1].append(dZ)
    return {k: np.array(v, dtype=np.complex128).reshape(len(freqs_hz), len(slots), P, P) for k, v in out.items()}


# ---- error rules ----
def errors(X, ref):
    """max|X - X_ref| / max|X_ref| over the grid and the entries."""
    return float(np.max(np.abs(np.asarray(X) - np.asarray(ref))) / np.max(np.abs(ref)))


def sens_errors(dX, ref):
    """[n_par]: the rule of loopgain_reference.sens_errors per parameter, the entries of the matrix taken with the frequencies: the
    relative error of every (frequency, entry), exact zero where the reference is exactly zero, the absolute bound 1e-8 of the
    parameter's largest |dX/dp| where the reference lies below 1e-12 of it.  dX, ref: [n_freq][n_par][P][P]."""
    dX, ref = np.asarray(dX), np.asarray(ref)
    n_par = ref.shape[1]
    flat = lambda a: np.moveaxis(a, 1, -1).reshape(-1, n_par)   # noqa: E731
    return LG.sens_errors(flat(dX), flat(ref)).max(axis=0)


_CACHE = {}


def shape_case(key):
    """(circuit, ports, z0, reference dict, {kind: e_cpu}, {kind: tolerance}) of a named shape case over smallsignal_cases.FREQS,
    computed once per process.  Keys: ("stage", n), ("star8", n), ("one",).  tolerance: smallsignal_cases.tolerance(e_cpu) =
    max(1e-12, 32 e_cpu); e_cpu > 1e-11 is refused."""
    if key not in _CACHE:
        (c, ports), z0 = {"stage": lambda: (stage(*key[1:]), Z0_STAGE), "star8": lambda: (star8(*key[1:]), Z0_STAR8), "one": lambda: (one_port(), (50.0,))}[key[0]]()
        ref = net_params(c, ports, z0, cases.FREQS)
        e_cpu = {k: errors(ref[k + "_l"], ref[k]) for k in KINDS}
        _CACHE[key] = (c, ports, z0, ref, e_cpu, {k: cases.tolerance(e) for k, e in e_cpu.items()})
    return _CACHE[key]
