"""Yardstick of the transient parameter sensitivities (ch_tran_sens).  TEST INFRASTRUCTURE ONLY; shares nothing with the engine.

Given a circuit, the CPU oracle's residual evaluation (`Oracle.eval`), the accepted times of a run and the order of every step, it
replays the variable-coefficient BDF in full MNA coordinates — its own Newton on `Oracle.eval(x, t, alpha0)` to 1e-13 — and runs the
direct-method recursion beside it:

    (G + a0 C) s_k = -[ df/dp_k + a0 dq/dp_k + sum_j a_j w_{j,k} ],      w_{n+1,k} = C s_k + dq/dp_k

G and C come from two `eval` calls (alpha0 = 0 and 2^40, see `matrices`); df/dp and dq/dp from Richardson-extrapolated central differences of
`Oracle.eval` under `Oracle.set_param` at relative steps 1e-3 and 5e-4 (the rule of `yardstick` in tests/test_gpu_dc_sens.py).
`lagrange_rows` is the dense output of a step (the polynomial through its newest points), for rows on a `saveat` grid.
Circuits use continuous sources only, so the left-limit rule at break points never matters."""
import math

import numpy as np

from cedarsim_jl_amd.circuit import (SLOT_DEV_MULT, SLOT_DEV_PAR, SLOT_GMIN, SLOT_MODEL_PAR, SLOT_SRC_DC, SLOT_SRC_PAR, SLOT_TEMP,
                                     SLOT_VA_PAR)

NEWTON_TOL = 1e-13
C_SCALE = 2.0 ** 40


def base_value(c, slot):
    k, a, b = c.slots[slot]
    return {SLOT_DEV_PAR: lambda: c.dev_par[a][b], SLOT_DEV_MULT: lambda: c.dev_mult[a], SLOT_MODEL_PAR: lambda: c.models[a][b],
            SLOT_SRC_DC: lambda: c.sources[a][0], SLOT_SRC_PAR: lambda: c.sources[a][1].par[b], SLOT_TEMP: lambda: c.temp,
            SLOT_GMIN: lambda: c.gmin, SLOT_VA_PAR: lambda: c.va_par[a]}[k]()


def bdf_alpha(tn, hist):
    """Coefficients of the variable-step BDF of order len(hist) at tn over the history times `hist` (newest first):
    dq/dt(tn) = alpha[0] q(tn) + sum_j alpha[j] q(hist[j-1])."""
    k = len(hist)
    tau = [tn] + list(hist)
    alpha = [sum(1.0 / (tau[0] - tau[m]) for m in range(1, k + 1))]
    for j in range(1, k + 1):
        num = den = 1.0
        for m in range(1, k + 1):
            if m != j:
                num *= tau[0] - tau[m]
        for m in range(0, k + 1):
            if m != j:
                den *= tau[j] - tau[m]
        alpha.append(num / den)
    return alpha


def lagrange_rows(t, pts, y, tq):
    """y[nt, ...] at the times tq: the step that ended at row i (t[i-1] < tq <= t[i]) interpolates through its pts[i] newest rows."""
    t, y = np.asarray(t, float), np.asarray(y, float)
    out = np.empty((len(tq),) + y.shape[1:])
    for q, x in enumerate(tq):
        if x <= t[0]:
            out[q] = y[0]
            continue
        i = min(int(np.searchsorted(t, x, side="left")), len(t) - 1)
        m = max(1, min(int(pts[i]), i + 1))
        rows = list(range(i - m + 1, i + 1))
        acc = np.zeros(y.shape[1:])
        for a in rows:
            w = 1.0
            for b in rows:
                if b != a:
                    w *= (x - t[b]) / (t[a] - t[b])
            acc = acc + w * y[a]
        out[q] = acc
    return out


class Replay:
    def __init__(self, oracle, circuit, slots, point=None):
        """slots: slot ids of the circuit; point: {slot: value} applied first (a sweep point)."""
        self.o, self.c, self.slots = oracle, circuit, list(slots)
        self.at = {s: base_value(circuit, s) for s in self.slots}
        for s, v in (point or {}).items():
            self.o.set_param(s, v)
            if s in self.at:
                self.at[s] = v
        self.n = oracle.n

    def matrices(self, x, t, mode=1):
        """f, q, G, C at (x, t): two eval calls, alpha0 = 0 and alpha0 = 2^40.  (With alpha0 = 1 an entry C << G — 1 pF beside 1 mS —
        drowns in the rounding of G + C: measured 3.7e-8 on the sensitivities of a 1 kOhm / 1 pF section.  A power of two scales C
        exactly, and where C is zero the difference is exactly zero.)"""
        f, q, G = self.o.eval(x, t, 0.0, mode)
        _, _, Ja = self.o.eval(x, t, C_SCALE, mode)
        return f, q, G, (Ja - G) / C_SCALE

    def partials(self, x, t, mode=1):
        """df/dp[K][n], dq/dp[K][n] at fixed (x, t): Richardson-extrapolated central differences at relative steps 1e-3 and 5e-4."""
        df, dq = [], []
        for s in self.slots:
            p = self.at[s]
            assert math.isfinite(p) and p != 0.0
            yf, yq = [], []
            for rel in (1e-3, 5e-4):
                h = rel * abs(p)
                self.o.set_param(s, p + h)
                fp, qp, _ = self.o.eval(x, t, 0.0, mode)
                self.o.set_param(s, p - h)
                fm, qm, _ = self.o.eval(x, t, 0.0, mode)
                yf.append((fp - fm) / (2.0 * h))
                yq.append((qp - qm) / (2.0 * h))
            self.o.set_param(s, p)
            df.append((4.0 * yf[1] - yf[0]) / 3.0)
            dq.append((4.0 * yq[1] - yq[0]) / 3.0)
        return np.array(df), np.array(dq)

    def newton(self, x, t, alpha0, hq, mode=1):
        """Solves f(x, t) + alpha0 q(x) + hq = 0 from the start x."""
        x = np.array(x, float)
        last = math.inf
        for _ in range(60):
            F, _, J = self.o.eval(x, t, alpha0, mode)
            dx = np.linalg.solve(J, -(F + hq))
            x = x + dx
            step = float(np.max(np.abs(dx)))
            if step <= NEWTON_TOL * max(1.0, float(np.max(np.abs(x)))):
                return x
            if step >= last and step < 1e-9:      # rounding floor of a stiff system: no further progress to be had
                return x
            last = step
        raise AssertionError("replay: Newton did not converge at t = %g" % t)

    def dc_start(self, mode=0):
        """(x0, s0[K][n]): the operating point by Newton from zero and G s0 = -df/dp there (mode 0: sources at their dc value;
        2: the waveforms at t = 0)."""
        from cedarsim_jl_amd import dc_opts
        rc, x0, _ = self.o.dc(dc_opts(abstol=1e-14, tran_mode=bool(mode)))
        assert rc == 0
        x0 = self.newton(x0, 0.0, 0.0, np.zeros(self.n), mode)
        _, _, G, _ = self.matrices(x0, 0.0, mode)
        df, _ = self.partials(x0, 0.0, mode)
        return x0, np.array([np.linalg.solve(G, -d) for d in df])

    def run(self, t, orders, x0, s0=None):
        """t[nt]: accepted times, t[0] the start; orders[i]: order of the step that ended at t[i] (orders[0] unused); x0[n]: the state at
        t[0]; s0[K][n] or None (zero).  Returns x[nt][n], s[nt][K][n]."""
        t = np.asarray(t, float)
        K, n, nt = len(self.slots), self.n, len(t)
        x, s = np.zeros((nt, n)), np.zeros((nt, K, n))
        qh, wh = np.zeros((nt, n)), np.zeros((nt, K, n))
        x[0] = x0
        if s0 is not None:
            s[0] = s0
        _, q0, _, C0 = self.matrices(x[0], t[0])
        _, dq0 = self.partials(x[0], t[0])
        qh[0] = q0
        wh[0] = s[0] @ C0.T + dq0
        for i in range(1, nt):
            k = int(orders[i])
            assert 1 <= k <= i, (i, k)
            hist = list(range(i - 1, i - 1 - k, -1))
            alpha = bdf_alpha(t[i], t[hist])
            hq = sum(alpha[j + 1] * qh[hist[j]] for j in range(k))
            x[i] = self.newton(x[i - 1], t[i], alpha[0], hq)
            _, q, G, C = self.matrices(x[i], t[i])
            df, dq = self.partials(x[i], t[i])
            A = G + alpha[0] * C
            for p in range(K):
                hw = sum(alpha[j + 1] * wh[hist[j]][p] for j in range(k))
                s[i][p] = np.linalg.solve(A, -(df[p] + alpha[0] * dq[p] + hw))
                wh[i][p] = C @ s[i][p] + dq[p]
            qh[i] = q
        return x, s
