"""Backward error of accepted transient steps and of operating points of LINEAR circuits.  TEST INFRASTRUCTURE ONLY; HIP-free, no
fixtures, shares nothing with the engine.

For a linear circuit  f(x, t) = G x - s(t),  q(x) = C x,  one Newton step with a freshly factored matrix is the exact solution of the
step's equations, so the accepted row x_i of a step of order k must satisfy its variable-step BDF equation

    (G + a0 C) x_i + sum_{j=1..k} a_j C x_{i-j} = s(t_i)

to rounding, whatever the predictor or the tolerances were.  `step_defects` measures how far the saved rows are from that, as the
componentwise (Oettli-Prager) backward error

    w_i = max_rows |r| / ( |G||x_i| + sum_{j=0..k} |a_j| |C||x_{i-j}| + |s(t_i)| )

in numpy.longdouble (the coefficients a_j included: `bdf_alpha` here, not the float one of transens_reference.py, which loses digits at
extreme step ratios).  The componentwise form, not a norm-wise one: MNA rows mix 1's (source rows) with 1e-3 S conductances, and a
norm would hide three digits.  `reference_defects` is the yardstick: the same measure for the plain float64 restatement of the
operation (right-hand side from the same history rows, `numpy.linalg.solve` — `scipy.sparse.linalg.spsolve` where the matrices are
sparse).  G and C are dense arrays or scipy.sparse matrices."""
import numpy as np

LD = np.longdouble
C_SCALE = 2.0 ** 40
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is no wider than a double here: the defect needs the 64-bit mantissa (or mpmath)"


def bdf_alpha(tn, hist):
    """Coefficients of the variable-step BDF of order len(hist) at tn over the history times `hist` (newest first), in longdouble:
    dq/dt(tn) = alpha[0] q(tn) + sum_j alpha[j] q(hist[j-1])."""
    tau = [LD(tn)] + [LD(h) for h in hist]
    k = len(hist)
    alpha = [sum((LD(1) / (tau[0] - tau[m]) for m in range(1, k + 1)), LD(0))]
    for j in range(1, k + 1):
        num = den = LD(1)
        for m in range(1, k + 1):
            if m != j:
                num *= tau[0] - tau[m]
        for m in range(0, k + 1):
            if m != j:
                den *= tau[j] - tau[m]
        alpha.append(num / den)
    return alpha


def linear_parts(oracle, c_scale=C_SCALE):
    """(G, C, s) of a linear circuit from `Oracle.eval`: f(x, t) = G x - s(t), q(x) = C x; s(t, mode=1) = -f(0, t) in that source
    mode (1: the waveforms at t; 0: the dc values; 2: the waveforms at 0).  C by the exact 2^40 scaling of `Replay.matrices`
    (c_scale: another power of two, for a circuit whose capacitances times 2^40 are still small beside its conductances).
    Refuses a circuit with a MOSFET or a compiled device, and asserts linearity at two random points."""
    from cedarsim_jl_amd.circuit import DEV_MOS, DEV_VA
    kinds = list(oracle.circuit.dev_kind)
    if DEV_MOS in kinds or DEV_VA in kinds:
        raise ValueError("linear_parts: the circuit has a nonlinear device (MOSFET or compiled Verilog-A)")
    n = oracle.n
    zero = np.zeros(n)
    _, _, G = oracle.eval(zero, 0.0, 0.0, 1)
    _, _, Ja = oracle.eval(zero, 0.0, c_scale, 1)
    C = (Ja - G) / c_scale

    def s(t, mode=1):
        return -oracle.eval(zero, float(t), 0.0, mode)[0]

    rng = np.random.default_rng(11)
    for t in (0.0, 3.7e-9):
        x = rng.uniform(-2.0, 2.0, n)
        f, q, J = oracle.eval(x, t, 0.0, 1)
        st = s(t)
        assert np.array_equal(J, G), "linear_parts: the Jacobian depends on x"
        assert np.all(np.abs(f + st - G @ x) <= 64 * np.finfo(float).eps * (np.abs(G) @ np.abs(x) + np.abs(st))), "linear_parts: f is not G x - s(t)"
        assert np.all(np.abs(q - C @ x) <= 64 * np.finfo(float).eps * (np.abs(C) @ np.abs(x))), "linear_parts: q is not C x"
    return G, C, s


class _Op:
    """A matrix for longdouble products: dense (numpy matmul) or the triplets of a scipy.sparse matrix."""

    def __init__(self, M):
        self.sparse = hasattr(M, "tocoo")
        if self.sparse:
            m = M.tocoo()
            self.n, self.i, self.j, self.v = m.shape[0], m.row, m.col, m.data.astype(LD)
        else:
            self.n, self.M, self.A = M.shape[0], np.asarray(M).astype(LD), np.abs(np.asarray(M)).astype(LD)

    def mul(self, x, absolute=False):
        if not self.sparse:
            return (self.A if absolute else self.M) @ x
        out = np.zeros(self.n, LD)
        np.add.at(out, self.i, (np.abs(self.v) if absolute else self.v) * x[self.j])
        return out

    def support(self):
        """bool [n][n] (dense) or triplet indices (sparse) of the structural non-zeros."""
        return (self.i, self.j) if self.sparse else np.nonzero(self.M)


def observable_rows(X, *mats):
    """Rows of the equations in which every column with an entry in one of `mats` is observed: no NaN in that column of X[nt][n]."""
    seen = ~np.any(np.isnan(np.atleast_2d(X)), axis=0)
    ok = np.ones(len(seen), bool)
    for M in mats:
        i, j = _Op(M).support()
        ok[i[~seen[j]]] = False
    return np.nonzero(ok)[0]


def _omega(r, den, rows):
    r, den = np.abs(r[rows]), den[rows]
    assert np.all(r[den == 0] == 0), "a row whose terms are all zero has a residual"
    live = den > 0
    return float(np.max(r[live] / den[live])) if np.any(live) else 0.0


class _Steps:
    """The equations of every saved step from the history rows X (NaN: not observed, must meet no entry of C)."""

    def __init__(self, t, orders, X, G, C, s):
        self.t, self.orders = np.asarray(t, float), np.asarray(orders, int)
        self.G, self.C, self.s = _Op(G), _Op(C), s
        X = np.asarray(X, float)
        ci, cj = self.C.support()
        assert not np.any(np.isnan(X[:, np.unique(cj)])), "an unknown that carries charge or flux is not observed"
        self.X = np.nan_to_num(X, nan=0.0).astype(LD)
        self.Cx = [self.C.mul(x) for x in self.X]
        self.aCx = [self.C.mul(np.abs(x), True) for x in self.X]

    def alpha(self, i):
        k = int(self.orders[i])
        assert 1 <= k <= min(i, 5), (i, k)
        return bdf_alpha(self.t[i], self.t[i - 1::-1][:k])

    def defect(self, i, x, rows):
        """w of the candidate row x (longdouble, full MNA) as the result of step i."""
        a = self.alpha(i)
        st = self.s(self.t[i]).astype(LD)
        r = self.G.mul(x) + a[0] * self.C.mul(x) - st
        den = self.G.mul(np.abs(x), True) + np.abs(a[0]) * self.C.mul(np.abs(x), True) + np.abs(st)
        for j in range(1, len(a)):
            r += a[j] * self.Cx[i - j]
            den += np.abs(a[j]) * self.aCx[i - j]
        return _omega(r, den, rows)


def step_defects(t, orders, X, G, C, s, rows=None):
    """w_i of every saved step i >= 1 (entry 0 is 0): X[nt][n] the saved rows in MNA coordinates exactly as the engine returned them
    (NaN where an unknown is not observed), orders[i] the order of the step that ended at t[i], `rows` the equations to check
    (default: `observable_rows`)."""
    S = _Steps(t, orders, X, G, C, s)
    rows = observable_rows(X, G, C) if rows is None else rows
    return np.array([0.0] + [S.defect(i, S.X[i], rows) for i in range(1, len(S.t))])


def reference_defects(t, orders, X, G, C, s, rows=None):
    """The same w for the float64 restatement of every step: right-hand side s(t_i) - sum_j a_j C x_{i-j} from the same history rows
    in float64, the full system solved by numpy.linalg.solve (spsolve for sparse matrices)."""
    S = _Steps(t, orders, X, G, C, s)
    rows = observable_rows(X, G, C) if rows is None else rows
    sparse = hasattr(G, "tocoo")
    Xd = np.nan_to_num(np.asarray(X, float), nan=0.0)
    out = [0.0]
    for i in range(1, len(S.t)):
        a = [float(v) for v in S.alpha(i)]
        rhs = np.array(s(S.t[i]), float)
        for j in range(1, len(a)):
            rhs = rhs - a[j] * (C @ Xd[i - j])
        A = G + a[0] * C
        if sparse:
            import scipy.sparse.linalg as spla
            x = spla.spsolve(A.tocsc(), rhs)
        else:
            x = np.linalg.solve(A, rhs)
        out.append(S.defect(i, x.astype(LD), rows))
    return np.array(out)


def dc_defect(x, G, s0, rows=None):
    """w of G x = s0 (an operating point; x may hold NaN where an unknown is not observed)."""
    x = np.asarray(x, float)
    rows = observable_rows(x[None, :], G) if rows is None else rows
    g, xl, sl = _Op(G), np.nan_to_num(x, nan=0.0).astype(LD), np.asarray(s0, float).astype(LD)
    return _omega(g.mul(xl) - sl, g.mul(np.abs(xl), True) + np.abs(sl), rows)


def dc_reference_defect(G, s0, rows=None):
    """w of numpy.linalg.solve's (spsolve's) answer to G x = s0."""
    if hasattr(G, "tocoo"):
        import scipy.sparse.linalg as spla
        x = spla.spsolve(G.tocsc(), np.asarray(s0, float))
    else:
        x = np.linalg.solve(G, np.asarray(s0, float))
    return dc_defect(x, G, s0, np.arange(len(x)) if rows is None else rows)


def newton_replay_errors(replay, t, orders, X, cols, abstol, reltol):
    """A NONLINEAR circuit's saved rows against the converged Newton of every step on the engine's own history: for step i,
    x* solves f(x, t_i) + a0 q(x) + sum_j a_j q(x_{i-j}) = 0 (`Replay.newton` of transens_reference.py from the start x_i, the
    charges q(x_j) from the oracle at the saved rows), and the figure is wrms(x_i - x*) over the columns `cols` in the controller's
    weights 1 / (reltol max(|x_{i-1}|, |x_i|) + abstol).  Unobserved entries (NaN) must carry no charge; they start at 0 and the
    Newton finds them (they enter linearly).  Returns the figure per step (entry 0 is 0)."""
    from transens_reference import bdf_alpha as float_alpha
    t = np.asarray(t, float)
    Xz = np.nan_to_num(np.asarray(X, float), nan=0.0)
    hidden = np.any(np.isnan(np.asarray(X, float)), axis=0)
    _, _, _, C0 = replay.matrices(Xz[0], t[0])
    assert not np.any(C0[:, hidden]), "an unobserved unknown carries charge"
    q = [replay.o.eval(x, tt, 0.0, 1)[1] for x, tt in zip(Xz, t)]
    out = [0.0]
    for i in range(1, len(t)):
        k = int(orders[i])
        assert 1 <= k <= min(i, 5), (i, k)
        a = float_alpha(t[i], t[i - 1::-1][:k])
        hq = sum(a[j] * q[i - j] for j in range(1, k + 1))
        xs = replay.newton(Xz[i], t[i], a[0], hq)
        w = 1.0 / (reltol * np.maximum(np.abs(Xz[i - 1, cols]), np.abs(Xz[i, cols])) + abstol)
        out.append(float(np.sqrt(np.mean(((Xz[i, cols] - xs[cols]) * w) ** 2))))
    return np.array(out)


def excitation(X, cols, n_nodes):
    """The two figures of the excitation condition over the unknowns `cols` (MNA columns) of the rows X[nt][n]:
    the median over steps of max|x_i - x_{i-1}| / max|x|, and the smallest range any unknown covers in the run, as a fraction of the
    largest magnitude among the unknowns of its kind (node voltages: columns below n_nodes; branch currents: the others)."""
    X = np.asarray(X, float)
    cols = np.asarray(cols, int)
    Y = X[:, cols]
    assert not np.any(np.isnan(Y)), "an unknown of the excitation condition is not observed"
    step = np.max(np.abs(np.diff(Y, axis=0)), axis=1) / np.max(np.abs(Y))
    move = np.inf
    for kind in (cols < n_nodes, cols >= n_nodes):
        if np.any(kind):
            move = min(move, float(np.min(np.ptp(Y[:, kind], axis=0)) / np.max(np.abs(Y[:, kind]))))
    return float(np.median(step)), move
