"""Yardstick of the frequency-domain measurements (ch_freq_measure_rows, ch_ac_measure).  TEST INFRASTRUCTURE ONLY; shares nothing with
the engine.

One implementation of the definitions of DESIGN.md 2.7g over an abstract number type, run twice: `measure_mp` in mpmath at 40 digits
and `measure_f64` in plain float64.  The error of the float64 run against the 40-digit run is the `e_cpu` of the tolerance rule
`max(1e-12, 32 e_cpu)`.

A spec is a dict: kind ("when", "find_when", "find_at", "integ", "avg", "rms", "min", "max", "pp"), xscale ("log" | "lin"), s1 / s2
(dicts: a, b (-1: none), scale, sig ("re", "im", "mag", "db", "db10", "phase"), level, edge ("rise" | "fall" | "cross"), count (n >= 1
or -1: last), fd, ref_at (NaN: absolute level)), at, frm, to.  Rows are H[row][freq] complex of ONE sample; dH[row][par][freq].
`measure_*` return (value, status, [d value / d p_k]); value and derivatives are NaN where the status says so (1 not found, 2 empty
window, 3 non-finite signal in the span read, 4 flat interpolant at the event: derivatives NaN).

The phase is in degrees, unwrapped along the grid from row 0: k steps by -1 where the raw increment exceeds 180, by +1 where it is
<= -180.  Between rows a signal is the line in (u, g), u = log10 f or f.  A window end that sits on a row's frequency reads that row."""
import math

import mpmath
import numpy as np

EVENT_KINDS = ("when", "find_when")
WINDOW_KINDS = ("integ", "avg", "rms", "min", "max", "pp")
KINDS = ("when", "find_when", "find_at") + WINDOW_KINDS      # CH_FMEAS_* in order
SIGS = ("re", "im", "mag", "db", "db10", "phase")              # CH_FSIG_* in order
NAN = float("nan")


class _F64:
    @staticmethod
    def num(x):
        return float(x)

    sqrt = staticmethod(math.sqrt)
    log10 = staticmethod(math.log10)
    atan2 = staticmethod(math.atan2)
    pi = math.pi
    ln10 = math.log(10.0)

    @staticmethod
    def pow10(x):
        return 10.0 ** x


class _MP:
    @staticmethod
    def num(x):
        return x if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x))

    sqrt = staticmethod(mpmath.sqrt)
    log10 = staticmethod(mpmath.log10)
    atan2 = staticmethod(mpmath.atan2)

    @staticmethod
    def pow10(x):
        return mpmath.power(10, x)


def side(a, b=-1, scale=1.0, sig="db", level=0.0, edge="cross", count=1, fd=-math.inf, ref_at=NAN):
    return dict(a=int(a), b=int(b), scale=float(scale), sig=sig, level=float(level), edge=edge, count=int(count), fd=float(fd), ref_at=float(ref_at))


def spec(kind, s1, s2=None, xscale="log", at=1.0, frm=-math.inf, to=math.inf):
    return dict(kind=kind, xscale=xscale, s1=s1, s2=s2 or side(0), at=float(at), frm=float(frm), to=float(to))


def _finite(z):
    return bool(mpmath.isfinite(z)) if isinstance(z, (mpmath.mpc, mpmath.mpf)) else bool(np.isfinite(z))


class _Run:
    def __init__(self, A, f, H, dH, xscale):
        self.A, self.xscale = A, xscale
        self.ff = [float(x) for x in f]
        self.f = [A.num(x) for x in f]
        self.nf = len(self.f)
        self.u = [self.uof(x) for x in self.f]
        # rows: complex arrays, or (40-digit run) nested lists of mpmath.mpc
        self.H = H if A is _MP and not isinstance(H, np.ndarray) else np.asarray(H, complex)
        self.dH = None if dH is None else (dH if A is _MP and not isinstance(dH, np.ndarray) else np.asarray(dH, complex))
        self.n_par = 0 if dH is None else len(self.dH[0])
        self._g = {}

    def uof(self, x):
        return self.A.log10(x) if self.xscale == "log" else x

    def fof(self, u):
        return self.A.pow10(u) if self.xscale == "log" else u

    def h(self, rows, sd, i, k=None):
        """(re, im) of the side's H (or dH of parameter k) at row i; parts that are not finite are None."""
        A = self.A

        def parts(z):
            return [A.num(x) if _finite(x) else None for x in (z.real, z.imag)]

        z = parts((rows[sd["a"]] if k is None else rows[sd["a"]][k])[i])
        if sd["b"] >= 0:
            zb = parts((rows[sd["b"]] if k is None else rows[sd["b"]][k])[i])
            z = [None if (p is None or q is None) else p - q for p, q in zip(z, zb)]
        sc = A.num(sd["scale"])
        return [None if p is None else sc * p for p in z]

    def raw(self, sd, i):
        """The signal at row i without its wraps; None where it is not finite (a signal that reads one part ignores the other)."""
        A = self.A
        re, im = self.h(self.H, sd, i)
        sig = sd["sig"]
        if sig == "re":
            return re
        if sig == "im":
            return im
        if sig == "db10":
            return 10 * A.log10(re) if re is not None and re > 0 else None
        if re is None or im is None:
            return None
        if re == 0 and im == 0:
            return re if sig == "mag" else None
        if sig == "mag":
            return A.sqrt(re * re + im * im)
        if sig == "db":
            return 20 * A.log10(A.sqrt(re * re + im * im))
        return A.atan2(im, re) * 180 / (mpmath.pi if A is _MP else math.pi)

    def g(self, sd):
        """The signal at every row, unwrapped (None where it is not finite)."""
        key = (sd["a"], sd["b"], sd["scale"], sd["sig"])
        if key not in self._g:
            raw = [self.raw(sd, i) for i in range(self.nf)]
            if sd["sig"] == "phase":
                k, out = 0, [raw[0]]
                for i in range(1, self.nf):
                    if raw[i] is not None and raw[i - 1] is not None:
                        d = raw[i] - raw[i - 1]
                        k += -1 if d > 180 else (1 if d <= -180 else 0)
                    out.append(None if raw[i] is None else raw[i] + 360 * k)
                raw = out
            self._g[key] = raw
        return self._g[key]

    def dg(self, sd, k, i):
        A = self.A
        nan = A.num(NAN)
        re, im = (nan if p is None else p for p in self.h(self.H, sd, i))
        dre, dim = (nan if p is None else p for p in self.h(self.dH, sd, i, k))
        sig = sd["sig"]
        ln10 = mpmath.log(10) if A is _MP else math.log(10.0)
        pi = mpmath.pi if A is _MP else math.pi
        m2 = re * re + im * im
        if m2 == 0 and sig in ("mag", "db", "phase"):
            return A.num(NAN)   # 0 / 0: the device gives NaN too
        if sig == "re":
            return dre
        if sig == "im":
            return dim
        if sig == "mag":
            return (re * dre + im * dim) / A.sqrt(m2)
        if sig == "db":
            return 20 / ln10 * (re * dre + im * dim) / m2
        if sig == "db10":
            return 10 / ln10 * dre / re
        return 180 / pi * (re * dim - im * dre) / m2

    # -- a place on the axis: (i0, m, w0, w1) --
    def weights(self, i, x):
        u = self.u
        return i - 1, 2, (u[i] - x) / (u[i] - u[i - 1]), (x - u[i - 1]) / (u[i] - u[i - 1])

    def locate(self, fx):
        if not fx > self.ff[0]:
            return 0, 1, 1, 0
        if not fx < self.ff[-1]:
            return self.nf - 1, 1, 1, 0
        i = next(j for j in range(1, self.nf) if self.ff[j] >= fx)
        return self.weights(i, self.uof(self.A.num(fx)))

    def val_at(self, sd, p):
        g = self.g(sd)
        i0, m, w0, w1 = p
        if m == 1:
            return g[i0]
        if g[i0] is None or g[i0 + 1] is None:
            return None
        return w0 * g[i0] + w1 * g[i0 + 1]

    def d_at(self, sd, k, p):
        i0, m, w0, w1 = p
        return self.dg(sd, k, i0) if m == 1 else w0 * self.dg(sd, k, i0) + w1 * self.dg(sd, k, i0 + 1)

    def slope_at(self, sd, p):
        g = self.g(sd)
        i0, m, _, _ = p
        return 0 if m == 1 else (g[i0 + 1] - g[i0]) / (self.u[i0 + 1] - self.u[i0])


def _fail(status, n_par):
    return NAN, status, [NAN] * n_par


def _event(R, sd, L):
    """(interval, non-finite in the span read)."""
    g = R.g(sd)
    found, count = -1, 0
    for i in range(1, R.nf):
        g0, g1 = g[i - 1], g[i]
        if g0 is None or g1 is None or not R.ff[i] >= sd["fd"]:
            continue
        rise, fall = g0 < L <= g1, g0 > L >= g1
        if not ((sd["edge"] in ("rise", "cross") and rise) or (sd["edge"] in ("fall", "cross") and fall)):
            continue
        if not R.ff[i - 1] >= sd["fd"]:
            fs = R.f[i] if g1 == L else R.fof(R.u[i - 1] + (L - g0) / (g1 - g0) * (R.u[i] - R.u[i - 1]))
            if not fs >= sd["fd"]:
                continue
        count += 1
        found = i
        if count == sd["count"]:
            break
    if sd["count"] > 0 and count != sd["count"]:
        found = -1
    span = range(0, found + 1) if (sd["count"] > 0 and found >= 0) else range(R.nf)
    return found, any(g[i] is None for i in span)


def _measure(A, f, H, dH, sp, runs=None):
    """runs: a dict shared by the specs of one sample (one _Run per axis: the signals are computed once)."""
    if runs is None:
        runs = {}
    if sp["xscale"] not in runs:
        runs[sp["xscale"]] = _Run(A, f, H, dH, sp["xscale"])
    R = runs[sp["xscale"]]
    n_par, kind, s1, s2 = R.n_par, sp["kind"], sp["s1"], sp["s2"]
    num = A.num
    if kind in EVENT_KINDS:
        rel = math.isfinite(s1["ref_at"])
        L, pref = num(s1["level"]), None
        if rel:
            pref = R.locate(s1["ref_at"])
            gref = R.val_at(s1, pref)
            if gref is None:
                return _fail(3, n_par)
            L = L + gref
        i, nonfinite = _event(R, s1, L)
        if nonfinite:
            return _fail(3, n_par)
        if i < 0:
            return _fail(1, n_par)
        g = R.g(s1)
        g0, g1 = g[i - 1], g[i]
        if g1 == L:
            ux, fstar = R.u[i], R.f[i]
        else:
            ux = R.u[i - 1] + (L - g0) / (g1 - g0) * (R.u[i] - R.u[i - 1])
            fstar = R.fof(ux)
        p = R.weights(i, ux)
        slope = (g1 - g0) / (R.u[i] - R.u[i - 1])
        value = fstar
        if kind == "find_when":
            value = R.val_at(s2, p)
            if value is None:
                return _fail(3, n_par)
        if slope == 0:
            return float(value), 4, [NAN] * n_par
        ln10 = mpmath.log(10) if A is _MP else math.log(10.0)
        out = []
        for k in range(n_par):
            dL = R.d_at(s1, k, pref) if rel else 0
            du = (dL - R.d_at(s1, k, p)) / slope
            if kind == "when":
                out.append(ln10 * fstar * du if sp["xscale"] == "log" else du)
            else:
                out.append(R.d_at(s2, k, p) + R.slope_at(s2, p) * du)
        return value, 0, out
    if kind == "find_at":
        p = R.locate(sp["at"])
        v = R.val_at(s1, p)
        if v is None:
            return _fail(3, n_par)
        return v, 0, [R.d_at(s1, k, p) for k in range(n_par)]
    # ---- windows: the point set (from, rows strictly inside, to) ----
    frm, to = max(sp["frm"], R.ff[0]), min(sp["to"], R.ff[-1])
    if not to > frm:
        return _fail(2, n_par)
    pts = [(num(frm), R.locate(frm))] + [(R.f[i], (i, 1, 1, 0)) for i in range(R.nf) if frm < R.ff[i] < to] + [(num(to), R.locate(to))]
    # (an end inside an interval touches both its rows)
    vals = [R.val_at(s1, p) for _, p in pts]
    if any(v is None for v in vals):
        return _fail(3, n_par)
    x = [a for a, _ in pts]
    span = num(to) - num(frm)

    def trap(y):
        return sum((y[j] + y[j + 1]) / 2 * (x[j + 1] - x[j]) for j in range(len(x) - 1))

    ds = [[R.d_at(s1, k, p) for _, p in pts] for k in range(n_par)]
    jmn = min(range(len(vals)), key=lambda j: (vals[j], j))
    jmx = min(range(len(vals)), key=lambda j: (-vals[j], j))
    if kind == "integ":
        return trap(vals), 0, [trap(d) for d in ds]
    if kind == "avg":
        return trap(vals) / span, 0, [trap(d) / span for d in ds]
    if kind == "rms":
        r = A.sqrt(trap([v * v for v in vals]) / span)
        return r, 0, [trap([v * q for v, q in zip(vals, d)]) / (r * span) for d in ds]
    if kind == "min":
        return vals[jmn], 0, [d[jmn] for d in ds]
    if kind == "max":
        return vals[jmx], 0, [d[jmx] for d in ds]
    return vals[jmx] - vals[jmn], 0, [d[jmx] - d[jmn] for d in ds]


def measure_mp(f, H, dH, sp, runs=None):
    """40-digit run: (value, status, sens) with mpmath numbers (NaN floats where the status says so)."""
    with mpmath.workdps(40):
        v, st, ds = _measure(_MP, f, H, dH, sp, runs)
        return v, st, list(ds)


def measure_f64(f, H, dH, sp, runs=None):
    v, st, ds = _measure(_F64, f, H, dH, sp, runs)
    return float(v), st, [float(d) for d in ds]


def errors(got, ref, scale):
    """|got - ref| / scale per entry, in float; `ref` mpmath numbers or NaN floats.  A NaN on one side only is infinite."""
    out = []
    for g, r in zip(got, ref):
        gn = isinstance(g, float) and math.isnan(g)
        rn = (isinstance(r, float) and math.isnan(r)) or (isinstance(r, mpmath.mpf) and bool(mpmath.isnan(r)))
        if gn or rn:
            out.append(0.0 if gn and rn else math.inf)
        else:
            with mpmath.workdps(40):
                out.append(float(abs(mpmath.mpf(g) - r) / scale))
    return out


def signal_rows(f, H, dH, sd, xscale="log"):
    """(g[n_freq], dg[n_par][n_freq]) of one side in float64 (NaN where not finite): what the comparison scales by."""
    R = _Run(_F64, f, H, dH, xscale)
    g = [NAN if v is None else v for v in R.g(sd)]
    dg = [[R.dg(sd, k, i) if R.raw(sd, i) is not None else NAN for i in range(R.nf)] for k in range(R.n_par)]
    return np.array(g, float), np.array(dg, float).reshape(R.n_par, R.nf)
