"""An analytic yardstick for noise PSD parameter sensitivities of linear circuits, on top of smallsignal_reference.py and
acsens_reference.py (numpy stamps of the full MNA system, every solve refined at 40 digits).  With Y^T y = e_out and the thermal
noise of every resistor, pwr_e = 4kT m_e / R_e between its terminals a_e, b_e:

    S       = sum_e |dy_e|^2 pwr_e,                     dy_e = y[a_e] - y[b_e]
    Y^T z_k = -(dY/dp_k)^T y
    dS/dp_k = sum_e [ 2 Re(conj(dy_e) dz_{k,e}) pwr_e + |dy_e|^2 dpwr_{k,e} ]

with dY/dp_k the analytic stamp of acsens_reference.derivative_stamp and dpwr analytic: -4kT m/R^2 for the resistance, 4kT/R for the
multiplier, pwr/T for `temp` (whose dY is 0).  The sums run in mpmath.  Beside the value the yardstick returns the conditioning
scale D(k) = sum_e ( |2 Re(conj(dy_e) dz_e)| pwr_e + |dy_e|^2 |dpwr_e| ): what the terms of the sum amount to before they cancel.

`fd_noise_sens` is the SAME METHOD as the engine's in numpy double precision — differences of the numpy stamps and of the source
table at the steps of `sens_step` (ch_sens_host.hpp), LAPACK solves — and its error against the yardstick, in units of D, is the
`e_cpu` the GPU tolerance derives from."""
import mpmath
import numpy as np

import acsens_reference as AR
import smallsignal_reference as SR
from cedarsim_jl_amd.circuit import DEV_R, SLOT_DEV_MULT, SLOT_DEV_PAR, SLOT_TEMP

KT4 = 4.0 * SR.K_BOLTZMANN
T0 = 273.15


def source_table(circuit):
    """[(a, b, pwr)] of every resistor: MNA node numbers (0 = ground) and 4kT m / R."""
    return [(circuit.dev_node[i][0], circuit.dev_node[i][1], KT4 * (circuit.temp + T0) * circuit.dev_mult[i] / circuit.dev_par[i][0])
            for i, k in enumerate(circuit.dev_kind) if k == DEV_R]


def dpwr_analytic(circuit, slot):
    """d(pwr_e)/dp for every entry of source_table, analytic."""
    kind, sa, sb = slot
    out = []
    for i, k in enumerate(circuit.dev_kind):
        if k != DEV_R:
            continue
        m, r, t = circuit.dev_mult[i], circuit.dev_par[i][0], circuit.temp + T0
        if kind == SLOT_TEMP:
            out.append(KT4 * m / r)
        elif kind == SLOT_DEV_PAR and sa == i and sb == 0:
            out.append(-KT4 * t * m / r ** 2)
        elif kind == SLOT_DEV_MULT and sa == i:
            out.append(KT4 * t / r)
        else:
            out.append(0.0)
    return out


def _stamp(circuit, slot, omega):
    if slot[0] == SLOT_TEMP:
        return np.zeros((circuit.n_mna, circuit.n_mna), dtype=np.complex128)
    return AR.derivative_stamp(circuit, slot, omega)[0]


def _delta(v, a, b, zero):
    return (v[a - 1] if a else zero) - (v[b - 1] if b else zero)


def noise_sens(circuit, slots, out_index, omega):
    """(S, dS[n_slots], D[n_slots]) at MNA row `out_index` and angular frequency omega; every solve refined at 40 digits."""
    Y, _ = SR.mna(circuit, omega)
    YT = Y.T.copy()
    e = np.zeros(Y.shape[0], dtype=np.complex128)
    e[out_index] = 1.0
    _, y, _ = SR.solve(YT, e)
    table = source_table(circuit)
    dS, D = [], []
    with mpmath.workdps(SR.MP_DIGITS):
        zero = mpmath.mpc(0)
        dy = [_delta(y, a, b, zero) for a, b, _ in table]
        S = mpmath.fsum((d.real ** 2 + d.imag ** 2) * mpmath.mpf(p) for d, (_, _, p) in zip(dy, table))
    for slot in slots:
        dYT = _stamp(circuit, slot, omega).T
        dpw = dpwr_analytic(circuit, slot)
        if dYT.any():
            with mpmath.workdps(SR.MP_DIGITS):
                rhs = [complex(-mpmath.fsum(SR._mpc(dYT[r, j]) * y[int(j)] for j in np.nonzero(dYT[r])[0])) for r in range(len(e))]
            _, z, _ = SR.solve(YT, np.array(rhs))
        else:
            z = None
        with mpmath.workdps(SR.MP_DIGITS):
            val, scale = mpmath.mpf(0), mpmath.mpf(0)
            for d, (a, b, p), dp in zip(dy, table, dpw):
                cross = mpmath.mpf(0)
                if z is not None:
                    dz = _delta(z, a, b, zero)
                    cross = 2 * (d.real * dz.real + d.imag * dz.imag) * mpmath.mpf(p)
                own = (d.real ** 2 + d.imag ** 2) * mpmath.mpf(dp)
                val += cross + own
                scale += abs(cross) + abs(own)
            dS.append(float(val))
            D.append(float(scale))
    return float(S), np.array(dS), np.array(D)


def step_of(circuit, slot):
    if slot[0] == SLOT_TEMP:
        p = circuit.temp
        return True, AR.REL_STEP * abs(p) if p != 0.0 else AR.REL_STEP
    return AR.step_of(circuit, slot)


def _moved(circuit, slot, dp):
    if slot[0] == SLOT_TEMP:
        return AR._with(circuit, lambda d: setattr(d, "temp", d.temp + dp))
    return AR._moved(circuit, slot, dp)


def fd_noise_sens(circuit, slots, out_index, omega):
    """The engine's method in numpy doubles: (S, dS[n_slots])."""
    Y, _ = SR.mna(circuit, omega)
    e = np.zeros(Y.shape[0], dtype=np.complex128)
    e[out_index] = 1.0
    y = np.linalg.solve(Y.T, e)
    table = source_table(circuit)
    pwr = np.array([p for _, _, p in table])

    def delta(v):
        return np.array([(v[a - 1] if a else 0.0) - (v[b - 1] if b else 0.0) for a, b, _ in table])
    dy = delta(y)
    S = float(np.sum(np.abs(dy) ** 2 * pwr))
    out = []
    for slot in slots:
        central, h = step_of(circuit, slot)
        cp = _moved(circuit, slot, h)
        cm = _moved(circuit, slot, -h) if central else circuit
        den = 2.0 * h if central else h
        dY = (SR.mna(cp, omega)[0] - SR.mna(cm, omega)[0]) / den
        dpw = (np.array([p for _, _, p in source_table(cp)]) - np.array([p for _, _, p in source_table(cm)])) / den
        z = np.linalg.solve(Y.T, -(dY.T @ y))
        dz = delta(z)
        out.append(float(np.sum(2.0 * np.real(np.conj(dy) * dz) * pwr + np.abs(dy) ** 2 * dpw)))
    return S, np.array(out)


def scaled_error(got, want, D):
    """|got - want| / D per parameter; where D = 0 the result must be exactly 0 (inf otherwise)."""
    got, want, D = np.asarray(got, float), np.asarray(want, float), np.asarray(D, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(D > 0.0, np.abs(got - want) / D, np.where(got == 0.0, 0.0, np.inf))
