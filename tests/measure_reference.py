"""Yardstick of the waveform measurements (ch_measure_rows, ch_result_measure).  TEST INFRASTRUCTURE ONLY; shares nothing with the engine.

One implementation of the definitions of DESIGN.md 2.7e over an abstract number type, run twice: `measure_mp` in mpmath at 40 digits
(60 halvings of the bracket, then a bracketed secant iteration to 2^-130 of the interval) and `measure_f64` in plain float64
(bisection until the bracket no longer shrinks).  The error of
the float64 run against the 40-digit run is the `e_cpu` of the tolerance rule `max(1e-12, 32 e_cpu)`.

A spec is a dict: kind ("when", "delay", "find_when", "find_at", "integ", "avg", "rms", "min", "max", "pp"), s1 / s2 (dicts: a, b
(-1: none), scale, level, edge ("rise" | "fall" | "cross"), count (n >= 1 or -1: last), td), at, frm, to.  Rows are y[row][time] of
ONE sample; sens[row][par][time].  `measure_*` return (value, status, [d value / d p_k]); value and derivatives are NaN where the
status says so (1 not found, 2 empty window, 3 non-finite row in the span read, 4 flat interpolant at the event: derivatives NaN).

The interpolant on (t[i-1], t[i]] is the polynomial through the m = min(pts[i], i + 1) newest rows when m >= 2 and their times are
distinct, else the line through rows i-1 and i; an interval of zero length has the value y[i].  A window end that sits on a row's
time reads that row (the later one of a repeated time at `frm`, the earlier at `to`: the window lies between them)."""
import math

import mpmath
import numpy as np

EVENT_KINDS = ("when", "delay", "find_when")
WINDOW_KINDS = ("integ", "avg", "rms", "min", "max", "pp")
NAN = float("nan")


class _F64:
    bits = 0

    @staticmethod
    def num(x):
        return float(x)

    sqrt = staticmethod(math.sqrt)


class _MP:
    bits = 140

    @staticmethod
    def num(x):
        return mpmath.mpf(float(x))

    sqrt = staticmethod(mpmath.sqrt)


def side(a, b=-1, scale=1.0, level=0.0, edge="rise", count=1, td=-math.inf):
    return dict(a=int(a), b=int(b), scale=float(scale), level=float(level), edge=edge, count=int(count), td=float(td))


def spec(kind, s1, s2=None, at=0.0, frm=-math.inf, to=math.inf):
    return dict(kind=kind, s1=s1, s2=s2 or side(0), at=float(at), frm=float(frm), to=float(to))


class _Run:
    """Times, dense points and the rows of one sample in the number type A; `fin[row][i]`: the float row value is finite."""

    def __init__(self, A, t, pts, y, sens):
        self.A = A
        self.tf = [float(x) for x in t]
        self.t = [A.num(x) for x in t]
        self.nt = len(self.t)
        self.pts = [0] * self.nt if pts is None else [int(p) for p in pts]
        y = np.asarray(y, float)
        self.fin = np.isfinite(y)
        self.y = [[A.num(v) if f else None for v, f in zip(row, fr)] for row, fr in zip(y, self.fin)]
        self.sens = None if sens is None else [[[A.num(v) for v in par] for par in row] for row in np.asarray(sens, float)]
        self.n_par = 0 if sens is None else len(self.sens[0])

    # -- signals: callables i -> value (None where a row is not finite) --
    def signal(self, sd):
        a, b, sc = sd["a"], sd["b"], self.A.num(sd["scale"])

        def at(i):
            if not self.fin[a][i] or (b >= 0 and not self.fin[b][i]):
                return None
            return sc * (self.y[a][i] - (self.y[b][i] if b >= 0 else 0))
        return at

    def sens_signal(self, sd, k):
        a, b, sc = sd["a"], sd["b"], self.A.num(sd["scale"])
        return lambda i: sc * (self.sens[a][k][i] - (self.sens[b][k][i] if b >= 0 else 0))

    # -- interpolant --
    def window(self, i):
        if not self.t[i] > self.t[i - 1]:
            return [i]
        m = min(self.pts[i], i + 1)
        rows = list(range(i - m + 1, i + 1))
        if m < 2 or any(not self.t[r] > self.t[r - 1] for r in rows[1:]):
            return [i - 1, i]
        return rows

    def weights(self, rows, x, deriv=False):
        t = self.t
        if len(rows) == 1:
            return [self.A.num(0 if deriv else 1)]
        out = []
        for a in rows:
            if not deriv:
                w = self.A.num(1)
                for b in rows:
                    if b != a:
                        w = w * (x - t[b]) / (t[a] - t[b])
            else:
                w = self.A.num(0)
                for c in rows:
                    if c == a:
                        continue
                    p = 1 / (t[a] - t[c])
                    for b in rows:
                        if b != a and b != c:
                            p = p * (x - t[b]) / (t[a] - t[b])
                    w = w + p
            out.append(w)
        return out

    @staticmethod
    def dot(sig, rows, w):
        vals = [sig(r) for r in rows]
        if any(v is None for v in vals):
            return None
        acc = 0
        for v, ww in zip(vals, w):
            acc = acc + ww * v
        return acc

    def event_time(self, sig, i, L):
        t = self.t
        y0, y1 = sig(i - 1), sig(i)
        if y1 == L or not t[i] > t[i - 1]:
            return t[i]
        rows, up = self.window(i), y0 < L
        lo, hi = t[i - 1], t[i]
        if any(sig(r) is None for r in rows):
            return hi

        def g(x):
            return self.dot(sig, rows, self.weights(rows, x)) - L

        for _ in range(60 if self.A.bits else 400):     # 40 digits: 60 halvings pick the root, a bracketed secant iteration polishes it
            mid = lo + (hi - lo) / 2
            if not (lo < mid < hi):
                break
            gm = g(mid)
            if gm == 0:
                return mid
            if (gm < 0) == up:
                lo = mid
            else:
                hi = mid
        if not self.A.bits:
            return hi
        glo, ghi = g(lo), g(hi)
        if glo == 0 or ghi == 0 or (glo < 0) == (ghi < 0):   # (rounding at the bracket's ends: it is 2^-60 of the interval wide already)
            return lo if glo == 0 else hi
        return mpmath.findroot(g, (lo, hi), solver="illinois", tol=(hi - lo) * mpmath.mpf(2) ** -70, maxsteps=60, verify=False)

    def search(self, sig, sd):
        """(interval of the wanted event or None, a non-finite row in the span read)."""
        L, td, n = self.A.num(sd["level"]), sd["td"], sd["count"]
        rise, fall = sd["edge"] in ("rise", "cross"), sd["edge"] in ("fall", "cross")
        count, last = 0, None
        for i in range(1, self.nt):
            y0, y1 = sig(i - 1), sig(i)
            if y0 is None or y1 is None:
                continue
            if not ((rise and y0 < L <= y1) or (fall and y0 > L >= y1)):
                continue
            if self.tf[i] < td or (self.tf[i - 1] < td and not self.event_time(sig, i, L) >= td):   # (the event lies in (t[i-1], t[i]])
                continue
            count, last = count + 1, i
            if count == n:
                break
        found = last if (n == -1 or count == n) else None
        span = range(0, (found + 1) if (found is not None and n != -1) else self.nt)   # the last event is known only at the end of the run
        return found, any(sig(i) is None for i in span)

    def locate(self, x):
        """(rows, weights) of the interpolant at x, as solution._dense_eval places it."""
        if not x > self.t[0]:
            return [0], [self.A.num(1)]
        if not x < self.t[-1]:
            return [self.nt - 1], [self.A.num(1)]
        i = next(j for j in range(self.nt) if self.t[j] >= x)
        rows = self.window(i)
        return rows, self.weights(rows, x)

    def window_end(self, x, is_from):
        """(rows, weights) of a window's end value: the row itself where x sits on a row's time."""
        if is_from:
            i = next(j for j in range(self.nt) if self.t[j] > x)
            if self.t[i - 1] == x:
                return [i - 1], [self.A.num(1)]
        else:
            i = next(j for j in range(self.nt) if self.t[j] >= x)
            if self.t[i] == x:
                return [i], [self.A.num(1)]
        rows = self.window(i)
        return rows, self.weights(rows, x)


def _measure(A, sp, t, pts, y, sens):
    R = _Run(A, t, pts, y, sens)
    nan_s = [NAN] * R.n_par
    kind = sp["kind"]
    if kind in EVENT_KINDS:
        sides = [sp["s1"]] + ([sp["s2"]] if kind == "delay" else [])
        found = [R.search(R.signal(sd), sd) for sd in sides]
        if any(nf for _, nf in found):
            return NAN, 3, nan_s
        if any(i is None for i, _ in found):
            return NAN, 1, nan_s
        ev = []
        for sd, (i, _) in zip(sides, found):
            sig, L = R.signal(sd), A.num(sd["level"])
            te = R.event_time(sig, i, L)
            rows = R.window(i)
            w, dw = R.weights(rows, te), R.weights(rows, te, deriv=True)
            dP = R.dot(sig, rows, dw)
            ev.append((sd, te, rows, w, dw, dP))
        sd1, t1, rows1, w1, dw1, dP1 = ev[0]
        y2 = R.signal(sp["s2"])
        if kind == "find_when" and any(y2(r) is None for r in rows1):
            return NAN, 3, nan_s
        flat = any(len(e[2]) > 1 and e[5] == 0 for e in ev)
        value = t1 if kind == "when" else (ev[1][1] - t1 if kind == "delay" else R.dot(y2, rows1, w1))
        if flat or not R.n_par:
            return value, (4 if flat else 0), nan_s
        out = []
        for k in range(R.n_par):
            dt = [A.num(0) if len(e[2]) == 1 else -R.dot(R.sens_signal(e[0], k), e[2], e[3]) / e[5] for e in ev]
            if kind == "when":
                out.append(dt[0])
            elif kind == "delay":
                out.append(dt[1] - dt[0])
            else:
                out.append(R.dot(R.sens_signal(sp["s2"], k), rows1, w1) + R.dot(y2, rows1, dw1) * dt[0])
        return value, 0, out
    sig = R.signal(sp["s1"])
    if kind == "find_at":
        rows, w = R.locate(A.num(sp["at"]))
        if any(sig(r) is None for r in rows):
            return NAN, 3, nan_s
        return R.dot(sig, rows, w), 0, [R.dot(R.sens_signal(sp["s1"], k), rows, w) for k in range(R.n_par)]
    frm, to = max(sp["frm"], R.tf[0]), min(sp["to"], R.tf[-1])
    if not to > frm:
        return NAN, 2, nan_s
    frm, to = A.num(frm), A.num(to)
    # the point set: (time, rows, weights)
    points = [(frm,) + R.window_end(frm, True)] + [(R.t[j], [j], [A.num(1)]) for j in range(R.nt) if frm < R.t[j] < to] + [(to,) + R.window_end(to, False)]
    if any(sig(r) is None for _, rows, _ in points for r in rows):
        return NAN, 3, nan_s
    xs = [p[0] for p in points]
    ys = [R.dot(sig, rows, w) for _, rows, w in points]

    def trapz(v):
        acc = A.num(0)
        for j in range(1, len(xs)):
            acc = acc + (v[j - 1] + v[j]) * (xs[j] - xs[j - 1]) / 2
        return acc

    imin = min(range(len(ys)), key=lambda j: (ys[j], j))
    imax = min(range(len(ys)), key=lambda j: (-ys[j], j))
    integ, span = trapz(ys), to - frm
    rms = A.sqrt(trapz([v * v for v in ys]) / span)
    value = {"integ": integ, "avg": integ / span, "rms": rms, "min": ys[imin], "max": ys[imax], "pp": ys[imax] - ys[imin]}[kind]
    out = []
    for k in range(R.n_par):
        sk = R.sens_signal(sp["s1"], k)
        ss = [R.dot(sk, rows, w) for _, rows, w in points]
        out.append({"integ": lambda: trapz(ss), "avg": lambda: trapz(ss) / span, "rms": lambda: trapz([a * b for a, b in zip(ys, ss)]) / (rms * span),
                    "min": lambda: ss[imin], "max": lambda: ss[imax], "pp": lambda: ss[imax] - ss[imin]}[kind]())
    return value, 0, out


def measure_mp(sp, t, pts, y, sens=None):
    """The 40-digit yardstick: (value, status, derivatives) as mpmath numbers (NaN floats where the status says so)."""
    with mpmath.workdps(40):
        return _measure(_MP, sp, t, pts, y, sens)


def measure_f64(sp, t, pts, y, sens=None):
    return _measure(_F64, sp, t, pts, y, sens)


def errors(got, ref, scale):
    """|got - ref| / scale per entry, in float; `ref` mpmath numbers or NaN floats.  A NaN on one side only is infinite."""
    out = []
    for g, r in zip(got, ref):
        gn, rn = (isinstance(g, float) and math.isnan(g)), (isinstance(r, float) and math.isnan(r))
        if gn or rn:
            out.append(0.0 if gn and rn else math.inf)
        else:
            with mpmath.workdps(40):
                out.append(float(abs(mpmath.mpf(g) - r) / scale))
    return out
