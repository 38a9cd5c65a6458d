"""A small-signal reference that shares nothing with the engine or the oracle: the full, unreduced MNA system
`Y(w) x = b`, `Y = G + jwC`, stamped in numpy from the flat `Circuit` record and solved by LAPACK followed by iterative
refinement with residuals in mpmath at 40 digits.  Linear devices only: R, C, L, V, I, VCVS, VCCS, multipliers included.

Conventions (those of the MNA vector the engine and the oracle return): unknowns are the node voltages 1..n_nodes, then
the branch currents of `Circuit.branch_devices`; a branch current flows from the first terminal through the device to
the second; a current source drives its current from the first terminal through itself to the second.  `source_ac`
holds |ac|: every excitation is real and non-negative."""
import mpmath
import numpy as np

from cedarsim_jl_amd.circuit import (DEV_C, DEV_I, DEV_L, DEV_R, DEV_V, DEV_VCCS, DEV_VCVS, SLOT_DEV_PAR, SLOT_SRC_DC)

MP_DIGITS = 40
K_BOLTZMANN = 1.380649e-23


def _transconductance(Y, a, b, c, d, g):
    """A current g * (V(c) - V(d)) that leaves node a and enters node b (node 0 is ground and has no row)."""
    for row, sr in ((a, 1.0), (b, -1.0)):
        for col, sc in ((c, 1.0), (d, -1.0)):
            if row and col:
                Y[row - 1, col - 1] += sr * sc * g


def _branch(Y, br, a, b, m):
    """Branch current `br` from a to b (times m in the node equations) and the start V(a) - V(b) of its own row."""
    for node, s in ((a, 1.0), (b, -1.0)):
        if node:
            Y[node - 1, br] += s * m
            Y[br, node - 1] += s


def mna(circuit, omega, excitation="ac"):
    """(Y, b) of the circuit at angular frequency `omega`, complex128.  excitation "ac": the sources' |ac|; "dc": their
    DC values (for the operating point of a linear circuit, taken at omega = 0)."""
    nn = circuit.n_nodes
    branches = circuit.branch_devices
    n = nn + len(branches)
    Y = np.zeros((n, n), dtype=np.complex128)
    b = np.zeros(n, dtype=np.complex128)
    jw = 1j * float(omega)
    for i, kind in enumerate(circuit.dev_kind):
        nd, par, m = circuit.dev_node[i], circuit.dev_par[i], circuit.dev_mult[i]
        p, q = nd[0], nd[1]
        br = nn + branches.index(i) if i in branches else -1
        if kind in (DEV_V, DEV_I):
            si = circuit.dev_ipar[i][0]
            value = circuit.source_ac[si] if excitation == "ac" else circuit.sources[si][0]
        if kind == DEV_R:
            _transconductance(Y, p, q, p, q, m / par[0])
        elif kind == DEV_C:
            _transconductance(Y, p, q, p, q, jw * m * par[0])
        elif kind == DEV_L:
            _branch(Y, br, p, q, m)
            Y[br, br] -= jw * par[0]
        elif kind == DEV_V:
            _branch(Y, br, p, q, m)
            b[br] += value
        elif kind == DEV_I:
            if p:
                b[p - 1] -= m * value
            if q:
                b[q - 1] += m * value
        elif kind == DEV_VCVS:
            _branch(Y, br, p, q, m)
            if nd[2]:
                Y[br, nd[2] - 1] -= par[0]
            if nd[3]:
                Y[br, nd[3] - 1] += par[0]
        elif kind == DEV_VCCS:
            _transconductance(Y, p, q, nd[2], nd[3], m * par[0])
        else:
            raise ValueError("the small-signal reference knows linear devices only (device %r)" % circuit.dev_names[i])
    return Y, b


def _mpc(z):
    return mpmath.mpc(float(np.real(z)), float(np.imag(z)))


def solve(Y, b):
    """x with Y x = b: LAPACK, then iterative refinement whose residuals are formed in mpmath at 40 digits (over the
    non-zeros of Y only) until a correction is below 1e-25 of the solution.  Returns (x rounded to complex128, the
    refined solution as a list of mpc, |LAPACK's x - refined x| as a float array)."""
    n = len(b)
    x0 = np.linalg.solve(Y, b)
    if not np.all(np.isfinite(x0)):
        raise ValueError("LAPACK gave a non-finite solution")
    with mpmath.workdps(MP_DIGITS):
        rows = []
        for i in range(n):
            cols = np.nonzero(Y[i])[0]
            rows.append([(int(j), _mpc(Y[i, j])) for j in cols])
        bm = [_mpc(v) for v in b]
        x = [_mpc(v) for v in x0]
        for _ in range(12):
            r = np.array([complex(bm[i] - mpmath.fsum(a * x[j] for j, a in rows[i])) for i in range(n)])
            d = np.linalg.solve(Y, r)
            x = [x[i] + _mpc(d[i]) for i in range(n)]
            scale = max(abs(complex(v)) for v in x)
            if np.max(np.abs(d)) <= 1e-25 * scale:
                break
        else:
            raise ValueError("iterative refinement did not converge: the system is too ill-conditioned for this reference")
        xr = np.array([complex(v) for v in x])
        lapack_err = np.array([float(abs(_mpc(x0[i]) - x[i])) for i in range(n)])
    return xr, x, lapack_err


def scaled_error(x, ref, groups):
    """max over the index groups of max|x - ref| / max|ref| inside the group (node voltages and branch currents have
    different units, independent blocks different levels: each group is scaled by its own largest entry).  A group whose
    reference is all zero must be reproduced exactly."""
    worst = 0.0
    for g in groups:
        g = np.asarray(g, dtype=int)
        if g.size == 0:
            continue
        err, scale = np.max(np.abs(np.asarray(x)[g] - np.asarray(ref)[g])), np.max(np.abs(np.asarray(ref)[g]))
        if scale == 0.0:
            worst = max(worst, 0.0 if err == 0.0 else np.inf)
        else:
            worst = max(worst, err / scale)
    return float(worst)


def unit_groups(circuit):
    """[node rows, branch rows] of the MNA vector."""
    nn = circuit.n_nodes
    return [np.arange(nn), np.arange(nn, circuit.n_mna)]


def noise_psd(circuit, out_index, omega):
    """Output-noise PSD at MNA row `out_index` (a node voltage or a branch current) from the thermal noise of every
    resistor: the adjoint solve Y^T y = e_out, then sum_R m * 4kT/R * |y_a - y_b|^2, T = temp + 273.15."""
    Y, _ = mna(circuit, omega)
    e = np.zeros(Y.shape[0], dtype=np.complex128)
    e[out_index] = 1.0
    _, y, _ = solve(Y.T.copy(), e)
    kt4 = 4.0 * K_BOLTZMANN * (circuit.temp + 273.15)
    with mpmath.workdps(MP_DIGITS):
        total = mpmath.mpf(0)
        zero = mpmath.mpc(0)
        for i, kind in enumerate(circuit.dev_kind):
            if kind != DEV_R:
                continue
            a, b = circuit.dev_node[i][0], circuit.dev_node[i][1]
            d = (y[a - 1] if a else zero) - (y[b - 1] if b else zero)
            total += mpmath.mpf(circuit.dev_mult[i]) * kt4 / mpmath.mpf(circuit.dev_par[i][0]) * (d.real * d.real + d.imag * d.imag)
        return float(total)


def dc_sens(circuit, slot_descriptions):
    """Operating point x of a linear circuit (Y x = b at omega = 0 with the sources' DC values) and its derivatives
    dx/dp = Y^-1 (db/dp - dY/dp x) for every (kind, a, b) of `slot_descriptions` (entries of `Circuit.slots`), with
    analytic derivative stamps: d(1/R)/dR = -1/R^2, the gain of a VCCS / VCVS, the DC value of a source; a capacitance or
    inductance does not enter a DC system.  Returns (x[n_mna], s[n_slots][n_mna]), real."""
    nn = circuit.n_nodes
    branches = circuit.branch_devices
    Y, b = mna(circuit, 0.0, excitation="dc")
    xr, x, _ = solve(Y, b)
    out = []
    for kind, sa, sb in slot_descriptions:
        dY = np.zeros_like(Y)
        db = np.zeros_like(b)
        if kind == SLOT_SRC_DC:
            i = [k for k, dk in enumerate(circuit.dev_kind) if dk in (DEV_V, DEV_I) and circuit.dev_ipar[k][0] == sa][0]
            p, q, m = circuit.dev_node[i][0], circuit.dev_node[i][1], circuit.dev_mult[i]
            if circuit.dev_kind[i] == DEV_V:
                db[nn + branches.index(i)] = 1.0
            else:
                if p:
                    db[p - 1] -= m
                if q:
                    db[q - 1] += m
        elif kind == SLOT_DEV_PAR and sb == 0:
            nd, par, m, dk = circuit.dev_node[sa], circuit.dev_par[sa], circuit.dev_mult[sa], circuit.dev_kind[sa]
            if dk == DEV_R:
                _transconductance(dY, nd[0], nd[1], nd[0], nd[1], -m / par[0] ** 2)
            elif dk == DEV_VCCS:
                _transconductance(dY, nd[0], nd[1], nd[2], nd[3], m)
            elif dk == DEV_VCVS:
                br = nn + branches.index(sa)
                if nd[2]:
                    dY[br, nd[2] - 1] -= 1.0
                if nd[3]:
                    dY[br, nd[3] - 1] += 1.0
            elif dk not in (DEV_C, DEV_L):
                raise ValueError("no derivative stamp for device kind %d" % dk)
        else:
            raise ValueError("no derivative stamp for slot kind %d" % kind)
        with mpmath.workdps(MP_DIGITS):
            rhs = []
            for r in range(len(b)):
                cols = np.nonzero(dY[r])[0]
                rhs.append(complex(_mpc(db[r]) - mpmath.fsum(_mpc(dY[r, j]) * x[int(j)] for j in cols)))
        s, _, _ = solve(Y, np.array(rhs))
        out.append(s.real)
    return xr.real, np.array(out)


# ---- RC ladders: vin - r[0] - n1 - r[1] - n2 ... with c[i] from n(i+1) to ground; node 0 of the ladder is held ----
def tridiagonal_solve(lower, diag, upper, rhs):
    """Thomas algorithm along the last axis, vectorised over the leading axes (complex128).  lower[..., 0] and
    upper[..., -1] are ignored.  No pivoting: for the diagonally dominant matrices of an RC ladder."""
    diag, rhs = np.array(diag, dtype=np.complex128), np.array(rhs, dtype=np.complex128)
    lower, upper = np.asarray(lower), np.asarray(upper)
    n = diag.shape[-1]
    for i in range(1, n):
        w = lower[..., i] / diag[..., i - 1]
        diag[..., i] = diag[..., i] - w * upper[..., i - 1]
        rhs[..., i] = rhs[..., i] - w * rhs[..., i - 1]
    x = np.empty_like(rhs)
    x[..., n - 1] = rhs[..., n - 1] / diag[..., n - 1]
    for i in range(n - 2, -1, -1):
        x[..., i] = (rhs[..., i] - upper[..., i] * x[..., i + 1]) / diag[..., i]
    return x


def _rc_ladder_bands(rs, cs, omegas):
    g = 1.0 / np.asarray(rs, dtype=np.float64)
    cs = np.asarray(cs, dtype=np.float64)
    w = np.asarray(omegas, dtype=np.float64).reshape(-1, 1)
    diag = (g + np.append(g[1:], 0.0))[None, :] + 1j * w * cs[None, :]
    off = np.broadcast_to(-g[None, :], diag.shape)           # off[i] couples n(i) and n(i+1): lower[i] = -g[i], upper[i] = -g[i+1]
    return g, diag, off, np.concatenate([off[:, 1:], off[:, :1]], axis=1)


def rc_ladder_ac(rs, cs, omegas, vin=1.0):
    """(v[n_freq][N] of the nodes n1..nN, i[n_freq] the branch current of the source) for the held input `vin`."""
    g, diag, lower, upper = _rc_ladder_bands(rs, cs, omegas)
    rhs = np.zeros(diag.shape, dtype=np.complex128)
    rhs[:, 0] = g[0] * vin
    v = tridiagonal_solve(lower, diag, upper, rhs)
    return v, -(vin - v[:, 0]) * g[0]


def rc_ladder_noise(rs, cs, omegas, out, temp_c):
    """PSD[n_freq] at ladder node `out` (1..N): the matrix is symmetric and the held input has adjoint value 0."""
    g, diag, lower, upper = _rc_ladder_bands(rs, cs, omegas)
    rhs = np.zeros(diag.shape, dtype=np.complex128)
    rhs[:, out - 1] = 1.0
    y = tridiagonal_solve(lower, diag, upper, rhs)
    y = np.concatenate([np.zeros((y.shape[0], 1), dtype=np.complex128), y], axis=1)
    return np.sum(4.0 * K_BOLTZMANN * (temp_c + 273.15) * g[None, :] * np.abs(y[:, :-1] - y[:, 1:]) ** 2, axis=1)


def rc_ladder_mp(rs, cs, omega, rhs_node=None, vin=1.0):
    """The same recurrence for ONE frequency in mpmath at 40 digits.  rhs_node None: the AC solve, returns (v[N], i);
    rhs_node = k: the adjoint solve for output node k, returns y[N + 1] with y[0] = 0 for the held input."""
    with mpmath.workdps(MP_DIGITS):
        n = len(rs)
        g = [1 / mpmath.mpf(float(r)) for r in rs]
        jw = mpmath.mpc(0, float(omega))
        diag = [g[i] + (g[i + 1] if i + 1 < n else 0) + jw * mpmath.mpf(float(cs[i])) for i in range(n)]
        rhs = [mpmath.mpc(0)] * n
        if rhs_node is None:
            rhs[0] = g[0] * mpmath.mpf(float(vin))
        else:
            rhs[rhs_node - 1] = mpmath.mpc(1)
        for i in range(1, n):
            w = -g[i] / diag[i - 1]
            diag[i] = diag[i] + w * g[i]
            rhs[i] = rhs[i] - w * rhs[i - 1]
        x = [mpmath.mpc(0)] * n
        x[n - 1] = rhs[n - 1] / diag[n - 1]
        for i in range(n - 2, -1, -1):
            x[i] = (rhs[i] + g[i + 1] * x[i + 1]) / diag[i]
        if rhs_node is None:
            return np.array([complex(v) for v in x]), complex(-(mpmath.mpf(float(vin)) - x[0]) * g[0])
        return [mpmath.mpc(0)] + x


def rc_ladder_noise_mp(rs, cs, omega, out, temp_c):
    with mpmath.workdps(MP_DIGITS):
        y = rc_ladder_mp(rs, cs, omega, rhs_node=out)
        total = mpmath.mpf(0)
        for i, r in enumerate(rs):
            d = y[i] - y[i + 1]
            total += 4 * mpmath.mpf(K_BOLTZMANN) * mpmath.mpf(temp_c + 273.15) / mpmath.mpf(float(r)) * (d.real ** 2 + d.imag ** 2)
        return float(total)
