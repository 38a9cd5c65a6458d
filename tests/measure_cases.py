"""Synthetic rows, measure lists and the comparison rule shared by the GPU tests of the waveform measurements (tests/test_gpu_measure.py,
tests/test_gpu_measure_e2e.py).  TEST INFRASTRUCTURE ONLY.  Nothing here touches the GPU: `runner(t, pts, values, sens, specs)` is
handed in by the caller.

Rows: times t = 1 ns * (0.1 i + 0.03 sin 1.7 i) with one repeated time behind row 40, dense points 1 + i mod 5 with a 0 (no
polynomial) on every seventh row; three state rows and their sensitivity rows are smooth waves whose phase depends on the sample's
VARIANT s mod 3, so that neighbouring samples differ while the 40-digit yardstick is computed three times per row count, once, and
shared (`expected`).

The rule of DESIGN.md 2.7: a figure passes when its scaled error is at most max(1e-12, 32 e_cpu), e_cpu the float64 reference's scaled
error on the same case; a case with e_cpu > 1e-9 is refused as mis-designed.  Scales: event times and delays by the run's span,
values by the signal's largest magnitude (INTEG: times the span), derivatives by the value's scale times max|s| / max|y|."""
import functools
import math

import numpy as np

import measure_reference as mr
from cedarsim_jl_amd.measure import EDGES, KINDS, ChMeasureSpec

N_VARIANTS = 3
N_PAR = 3
LEVEL = 0.5
ROWS_AT = (1, 2, 3, 64, 65, 66, 129)
SAMPLES_AT = (1, 63, 64, 65, 130)
BOUNDARY_ROW = 4     # 129 rows are 128 intervals, 2 per lane: interval 4 closes lane 1's chunk [3, 5)


def times(nt):
    i = np.arange(nt, dtype=float)
    t = 1e-9 * (0.1 * i + 0.03 * np.sin(1.7 * i))
    if nt > 41:
        t[41] = t[40]
    pts = (1 + np.arange(nt) % 5).astype(np.int32)
    pts[np.arange(nt) % 7 == 6] = 0
    return t, pts


def variant_rows(nt, v):
    """(y[3][nt], s[3][N_PAR][nt]) of variant v."""
    t, _ = times(nt)
    tau = t * 1e9
    y = np.array([1.5 * np.sin(0.9 * tau + 0.37 * v) + 0.02 * tau, np.cos(0.45 * tau + 0.2 * v), 0.3 * tau - 0.1 * v + 0.05 * np.sin(3.0 * tau)])
    s = np.array([[np.cos(1.1 * tau + q + r + 0.1 * v) * (1.0 + 0.5 * q) for q in range(N_PAR)] for r in range(3)])
    if nt == 129:
        y[0, BOUNDARY_ROW] = LEVEL   # an event exactly on a lane-chunk boundary: y_i == L on the last row of lane 1's chunk
    return y, s


def batch(nt, S, n_par):
    """(t, pts, values[3][nt][S], sens[3][n_par][nt][S] or None)."""
    t, pts = times(nt)
    per = [variant_rows(nt, v) for v in range(N_VARIANTS)]
    values = np.stack([per[s % N_VARIANTS][0] for s in range(S)], axis=-1)
    sens = np.stack([per[s % N_VARIANTS][1][:, :n_par] for s in range(S)], axis=-1) if n_par else None
    return t, pts, np.ascontiguousarray(values), None if sens is None else np.ascontiguousarray(sens)


def specs_for(nt):
    """Every kind at the run's scale: events in each direction, the n-th and the last, a td inside the run; windows over the whole run,
    with ends inside the first and the last interval (the first and the last lane's chunk), inside one interval, and empty."""
    t, _ = times(nt)
    t0, t1 = float(t[0]), float(t[-1])
    span = t1 - t0
    first = t0 + 0.3 * (float(t[1]) - t0) if nt > 1 else t0
    last = t1 - 0.4 * (t1 - float(t[-2])) if nt > 1 else t1
    S = mr.side
    out = []
    for edge in ("rise", "fall", "cross"):
        for n in (1, 2, -1):
            out.append(mr.spec("when", S(0, level=LEVEL, edge=edge, count=n)))
        out.append(mr.spec("when", S(0, level=LEVEL, edge=edge, count=1, td=t0 + 0.37 * span)))
    out.append(mr.spec("when", S(0, 1, scale=0.5, level=0.1, edge="cross", count=2)))
    out.append(mr.spec("when", S(2, level=0.3 * 1e9 * span * 0.6, edge="rise")))
    out.append(mr.spec("when", S(0, level=7.0)))                                                   # never reached
    out.append(mr.spec("delay", S(0, level=LEVEL, edge="rise"), S(1, level=0.2, edge="fall")))
    out.append(mr.spec("delay", S(0, level=LEVEL, edge="cross", count=-1), S(2, 0, scale=-1.0, level=-0.4, edge="cross", count=1, td=t0 + 0.1 * span)))
    out.append(mr.spec("find_when", S(0, level=LEVEL, edge="rise"), S(1)))
    out.append(mr.spec("find_when", S(1, level=0.2, edge="fall", count=-1), S(0, 2, scale=2.0)))
    for at in (t0 - 1e-9, t0, first, t0 + 0.5 * span, last, t1, t1 + 1e-9):
        out.append(mr.spec("find_at", S(0, 1), at=at))
    for kind in mr.WINDOW_KINDS:
        out.append(mr.spec(kind, S(0)))
        out.append(mr.spec(kind, S(0, 1, scale=0.5), frm=first, to=last))
        out.append(mr.spec(kind, S(1), frm=t0 + 0.52 * span, to=t0 + 0.52 * span + 0.02e-9))
    out.append(mr.spec("avg", S(0), frm=t0 + 0.4 * span, to=t0 + 0.4 * span))                     # empty
    out.append(mr.spec("rms", S(2), frm=t1 + 1e-9, to=t1 + 2e-9))                                  # behind the run
    return out


def to_ctypes(specs):
    arr = (ChMeasureSpec * max(1, len(specs)))()
    for k, sp in enumerate(specs):
        c = arr[k]
        c.kind, c.at, c.frm, c.to = KINDS.index(sp["kind"]), sp["at"], sp["frm"], sp["to"]
        for dst, sd in ((c.s1, sp["s1"]), (c.s2, sp["s2"])):
            dst.row_a, dst.row_b, dst.scale, dst.level, dst.edge, dst.count, dst.td = sd["a"], sd["b"], sd["scale"], sd["level"], EDGES[sd["edge"]], sd["count"], sd["td"]
    return arr


def scales(sp, t, y, s):
    """(scale of the value, scale of a derivative) of one spec on the rows of one sample."""
    span = float(t[-1] - t[0]) or 1.0

    def amp(rows, sd):
        sig = sd["scale"] * (rows[sd["a"]] - (rows[sd["b"]] if sd["b"] >= 0 else 0.0))
        fin = np.abs(sig[np.isfinite(sig)])
        return float(fin.max()) if fin.size and fin.max() > 0 else 1.0

    kind = sp["kind"]
    sd = sp["s2"] if kind == "find_when" else sp["s1"]
    ymax = amp(y, sd)
    smax = max(amp(s[:, k], sd) for k in range(s.shape[1])) if s is not None and s.shape[1] else 1.0
    if kind in ("when", "delay"):
        ymax = amp(y, sp["s1"])
        vs = span
    elif kind == "integ":
        vs = ymax * span
    else:
        vs = ymax
    return vs, vs * smax / ymax


def reference(sp, t, pts, y, s):
    """One (spec, sample): dict(value, status, sens, tol_v, tol_s, e_cpu) from the 40-digit and the float64 reference."""
    vm, stm, dm = mr.measure_mp(sp, t, pts, y, s)
    vf, stf, df = mr.measure_f64(sp, t, pts, y, s)
    assert stm == stf, ("the two references disagree on a status", sp, stm, stf)
    vs, ss = scales(sp, t, y, s)
    ev = mr.errors([vf], [vm], vs)[0]
    es = max(mr.errors(df, dm, ss), default=0.0)
    assert ev <= 1e-9 and es <= 1e-9, ("mis-designed case: the float64 reference itself is off by %.2e (value) / %.2e (derivative)" % (ev, es), sp)
    return dict(value=vm, status=stm, sens=dm, vs=vs, ss=ss, tol_v=max(1e-12, 32 * ev), tol_s=max(1e-12, 32 * es), e_cpu=max(ev, es))


@functools.lru_cache(maxsize=None)
def expected(nt):
    """[variant][spec] -> reference(...), with all N_PAR derivatives; computed once per row count."""
    t, pts = times(nt)
    specs = specs_for(nt)
    return [[reference(sp, t, pts, *variant_rows(nt, v)) for sp in specs] for v in range(N_VARIANTS)]


def compare(what, specs, refs_of_sample, val, status, sens, n_par, verbose=True):
    """val, status [n_meas][S], sens [n_meas][n_par][S] or None against refs_of_sample(s) -> [spec] references.  Statuses and NaN
    positions exactly; figures under the rule.  Prints the worst figure per kind before it asserts."""
    n_meas, S = val.shape
    worst, bad = {}, []
    for s in range(S):
        refs = refs_of_sample(s)
        for k in range(n_meas):
            r, kind = refs[k], specs[k]["kind"]
            if int(status[k, s]) != r["status"]:
                bad.append("%s measure %d (%s) sample %d: status %d, yardstick %d" % (what, k, kind, s, status[k, s], r["status"]))
                continue
            ev = mr.errors([float(val[k, s])], [r["value"]], r["vs"])[0]
            es = 0.0
            if n_par:
                es = max(mr.errors([float(x) for x in sens[k, :n_par, s]], r["sens"][:n_par], r["ss"]))
            w = worst.setdefault(kind, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], ev), max(w[1], es), max(w[2], r["e_cpu"])
            if not (ev <= r["tol_v"] and es <= r["tol_s"]):
                bad.append("%s measure %d (%s) sample %d: value error %.3e (allowed %.3e), derivative error %.3e (allowed %.3e)" % (what, k, kind, s, ev, r["tol_v"], es, r["tol_s"]))
    if verbose:
        for kind, (ev, es, ec) in sorted(worst.items()):
            print("%s %-9s worst scaled error: value %.3e, derivative %.3e (float64 reference: %.3e)" % (what, kind, ev, es, ec))
    assert not bad, "\n".join(bad[:20])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


BIT_EQUAL_KINDS = ("when", "delay", "find_when", "find_at", "min", "max")


def nan_is(x):
    return isinstance(x, float) and math.isnan(x)
