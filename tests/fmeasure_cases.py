"""Synthetic complex rows, measure lists and the comparison rule shared by the GPU tests of the frequency-domain measurements
(tests/test_gpu_fmeasure.py, tests/test_gpu_ac_measure.py).  TEST INFRASTRUCTURE ONLY.  Nothing here touches the GPU.

Grid: f = 10^(1 + 5 (i + 0.2 sin 1.3 i) / (n - 1)) Hz, strictly increasing and not uniform in log f.  Three rows per sample, smooth in
x = i / (n - 1), whose phase offsets depend on the sample's VARIANT s mod 3, so that neighbouring samples differ while the 40-digit
yardstick is computed three times per grid size, once, and shared (`expected`):
  row 0  |H| falls from +40 dB to -40 dB with a ripple (one unity-gain crossing, in the middle); its phase repeats the steps
         -170, +20, +170, -20 degrees: a wrap in every odd interval, in alternating directions — on the 129-row grid (two intervals per
         lane of the split form) that is a wrap on every lane-chunk boundary.
  row 1  |H| = 2 + sin, phase falling by about 100 degrees per row: the wrap count k grows to 35 on 129 rows.
  row 2  a PSD: real, positive, im = 0.
The sensitivity rows are dH = H (a_k + j b_k) with smooth a, b.

The rule of DESIGN.md 2.7: a figure passes when its scaled error is at most max(1e-12, 32 e_cpu), e_cpu the float64 reference's scaled
error on the same case; here every case must have e_cpu <= 1e-12 itself (checked in `reference`).  Scales: an event frequency by the
grid's span in u (its error is taken in u), values by the signal's largest magnitude (INTEG: times the span in Hz), derivatives by the
value's scale times max|dg| / max|g| (an event frequency on a LOG axis: times ln 10 f*)."""
import functools
import math

import mpmath
import numpy as np

import fmeasure_reference as fr
from cedarsim_jl_amd.acmeasure import KINDS, SIGNALS, XSCALES, ChFMeasureSpec
from cedarsim_jl_amd.measure import EDGES

N_VARIANTS = 3
N_PAR = 3
FREQS_AT = (1, 2, 3, 63, 64, 65, 129)
SAMPLES_AT = (1, 2, 63, 64, 65, 130)
BIT_EQUAL_KINDS = ("when", "find_when", "find_at", "min", "max")


def grid(nf):
    i = np.arange(nf, dtype=float)
    return 10.0 ** (1.0 + 5.0 * (i + 0.2 * np.sin(1.3 * i)) / max(1, nf - 1))


def _phase0(nf, v):
    steps = np.array([-170.0, 20.0, 170.0, -20.0])
    return -95.0 + 3.0 * v + np.concatenate(([0.0], np.cumsum(steps[np.arange(nf - 1) % 4])))


def variant_rows(nf, v):
    """(H[3][nf], dH[3][N_PAR][nf]) complex, of variant v."""
    i = np.arange(nf, dtype=float)
    x = i / max(1, nf - 1)
    db0 = 40.0 - 80.0 * x + 1.5 * np.sin(9.0 * x + 0.05 * v)
    ph1 = 30.0 + 7.0 * v - 100.0 * i * (1.0 + 0.01 * np.sin(0.7 * i))
    H = np.array([10.0 ** (db0 / 20.0) * np.exp(1j * np.radians(_phase0(nf, v))),
                  (2.0 + np.sin(0.9 * i + 0.3 * v)) * np.exp(1j * np.radians(ph1)),
                  (1.0 + 3.0 / (1.0 + (5.0 * x) ** 2) + 0.1 * v) + 0j])
    dH = np.array([[H[r] * ((0.3 + 0.2 * q) * np.cos(2.0 * x + q + r) + 1j * (0.0 if r == 2 else 0.25) * np.sin(3.0 * x + q + 0.1 * v)) for q in range(N_PAR)] for r in range(3)])
    return H, dH


def batch(nf, S, n_par):
    """(f, values[3][nf][S], sens[3][n_par][nf][S] or None)."""
    per = [variant_rows(nf, v) for v in range(N_VARIANTS)]
    values = np.stack([per[s % N_VARIANTS][0] for s in range(S)], axis=-1)
    sens = np.stack([per[s % N_VARIANTS][1][:, :n_par] for s in range(S)], axis=-1) if n_par else None
    return grid(nf), np.ascontiguousarray(values), None if sens is None else np.ascontiguousarray(sens)


def specs_for(nf):
    """Every kind and signal on both axes.  On 129 rows the wanted event of the `db` row sits in the first chunk of the split form
    (interval 1 or 2), in a middle one and in the last one (interval 127 or 128); windows cover the whole grid, have their ends inside
    the first and the last interval, sit inside one interval, and are empty."""
    f = grid(nf)
    f0, f1 = float(f[0]), float(f[-1])
    g0 = fr.signal_rows(f, variant_rows(nf, 0)[0], None, fr.side(0, sig="db"))[0]
    first = math.sqrt(f0 * float(f[1])) if nf > 1 else f0
    last = math.sqrt(f1 * float(f[-2])) if nf > 1 else f1
    L_first = 0.5 * (g0[1] + g0[2]) if nf > 2 else 39.0
    L_last = 0.5 * (g0[-2] + g0[-3]) if nf > 2 else -39.0
    mid = float(f[nf // 2]) * 1.01
    S = fr.side
    out = []
    for xs in ("log", "lin"):
        for L in (L_first, 0.0, L_last):
            out.append(fr.spec("when", S(0, sig="db", level=L, edge="fall"), xscale=xs))
        out.append(fr.spec("when", S(0, sig="db", level=-3.0103, edge="fall", ref_at=f0), xscale=xs))
        out.append(fr.spec("when", S(0, sig="db", level=-3.0103, edge="cross", ref_at=first, fd=first), xscale=xs))
        for n in (1, 2, -1):
            out.append(fr.spec("when", S(1, sig="mag", level=2.0, edge="cross", count=n), xscale=xs))
        out.append(fr.spec("when", S(0, sig="phase", level=-180.0, edge="cross", count=3), xscale=xs))
        out.append(fr.spec("when", S(0, sig="phase", level=-180.0, edge="rise", count=-1), xscale=xs))
        out.append(fr.spec("when", S(1, sig="phase", level=-6000.0, edge="fall"), xscale=xs))
        out.append(fr.spec("when", S(1, sig="phase", level=-12000.0, edge="fall", count=-1), xscale=xs))
        out.append(fr.spec("when", S(1, sig="re", level=0.0, edge="rise", count=2, fd=mid), xscale=xs))
        out.append(fr.spec("when", S(1, sig="im", level=0.5, edge="fall", count=2), xscale=xs))
        out.append(fr.spec("when", S(2, sig="db10", level=3.0, edge="fall"), xscale=xs))
        out.append(fr.spec("when", S(0, sig="db", level=70.0), xscale=xs))                                  # never reached
        out.append(fr.spec("find_when", S(0, sig="db", level=0.0, edge="fall"), S(1, sig="phase"), xscale=xs))
        out.append(fr.spec("find_when", S(1, sig="phase", level=-6000.0, edge="fall"), S(0, sig="db"), xscale=xs))
        out.append(fr.spec("find_when", S(0, sig="db", level=L_last, edge="fall"), S(0, 1, scale=0.5, sig="mag"), xscale=xs))
        out.append(fr.spec("find_when", S(1, sig="mag", level=2.0, edge="rise", count=-1), S(0, sig="phase"), xscale=xs))
        for at in (0.5 * f0, f0, first, mid, last, f1, 2.0 * f1):
            out.append(fr.spec("find_at", S(1, sig="phase"), at=at, xscale=xs))
        out.append(fr.spec("find_at", S(0, sig="phase"), at=mid, xscale=xs))
        out.append(fr.spec("find_at", S(2, sig="db10"), at=mid, xscale=xs))
        out.append(fr.spec("find_at", S(0, 1, sig="im", scale=-2.0), at=last, xscale=xs))
        for kind in fr.WINDOW_KINDS:
            out.append(fr.spec(kind, S(1, sig="phase"), xscale=xs))
            out.append(fr.spec(kind, S(0, sig="db"), frm=first, to=last, xscale=xs))
            out.append(fr.spec(kind, S(2, sig="re"), frm=mid, to=mid * 1.001, xscale=xs))
            out.append(fr.spec(kind, S(1, sig="mag"), frm=0.5 * f0, to=mid, xscale=xs))
        out.append(fr.spec("avg", S(0, sig="re"), frm=mid, to=mid, xscale=xs))                              # empty
        out.append(fr.spec("rms", S(2, sig="re"), frm=2.0 * f1, to=3.0 * f1, xscale=xs))                    # beyond the grid
    return out


def to_ctypes(specs):
    arr = (ChFMeasureSpec * max(1, len(specs)))()
    for k, sp in enumerate(specs):
        c = arr[k]
        c.kind, c.xscale, c.at, c.frm, c.to = KINDS.index(sp["kind"]), XSCALES.index(sp["xscale"]), sp["at"], sp["frm"], sp["to"]
        for dst, sd in ((c.s1, sp["s1"]), (c.s2, sp["s2"])):
            dst.row_a, dst.row_b, dst.scale, dst.sig = sd["a"], sd["b"], sd["scale"], SIGNALS.index(sd["sig"])
            dst.level, dst.edge, dst.count, dst.fd, dst.ref_at = sd["level"], EDGES[sd["edge"]], sd["count"], sd["fd"], sd["ref_at"]
    return arr


def scales(sp, f, H, dH):
    """(scale of the value, scale of a derivative without the event's own factor) of one spec on the rows of one sample."""
    def amp(a):
        fin = np.abs(a[np.isfinite(a)])
        return float(fin.max()) if fin.size and fin.max() > 0 else 1.0

    kind = sp["kind"]
    sd = sp["s1"] if kind != "find_when" else sp["s2"]
    g, dg = fr.signal_rows(f, H, dH, sd, sp["xscale"])
    ymax, smax = amp(g), (max(amp(d) for d in dg) if len(dg) else 1.0)
    if kind == "when":
        g, dg = fr.signal_rows(f, H, dH, sp["s1"], sp["xscale"])
        ymax, smax = amp(g), (max(amp(d) for d in dg) if len(dg) else 1.0)
        vs = (math.log10(f[-1] / f[0]) if sp["xscale"] == "log" else float(f[-1] - f[0])) if len(f) > 1 else 1.0
    elif kind == "integ":
        vs = ymax * (float(f[-1] - f[0]) or 1.0)
    else:
        vs = ymax
    return vs, vs * smax / ymax


def figure_errors(sp, got_v, got_d, ref_v, ref_d, vs, ss):
    """Scaled errors (value, worst derivative) of one (spec, sample) against the 40-digit reference.  An event frequency on a LOG axis
    is compared in u = log10 f, its derivatives by ln 10 f* times the scale."""
    log_when = sp["kind"] == "when" and sp["xscale"] == "log"
    ref_nan = isinstance(ref_v, float) and math.isnan(ref_v)
    if log_when and not ref_nan and not math.isnan(got_v) and got_v > 0:
        with mpmath.workdps(40):
            ev = float(abs(mpmath.log10(mpmath.mpf(got_v)) - mpmath.log10(ref_v)) / vs)
    else:
        ev = fr.errors([got_v], [ref_v], vs)[0]
    if log_when and not ref_nan:
        ss = ss * math.log(10.0) * float(ref_v)
    return ev, max(fr.errors(list(got_d), list(ref_d), ss), default=0.0)


def reference(sp, f, H, dH, runs_mp=None, runs_f64=None, limit=1e-12):
    """One (spec, sample): dict(value, status, sens, tol_v, tol_s, e_cpu) from the 40-digit and the float64 reference.  limit: the
    float64 reference's own error above which a case is refused as mis-designed (synthetic rows: 1e-12; rows a circuit hands back
    are what they are: 1e-9, as for the transient measures)."""
    vm, stm, dm = fr.measure_mp(f, H, dH, sp, runs_mp)
    vf, stf, df = fr.measure_f64(f, H, dH, sp, runs_f64)
    assert stm == stf, ("the two references disagree on a status", sp, stm, stf)
    vs, ss = scales(sp, f, H, dH)
    ev, es = figure_errors(sp, vf, df, vm, dm, vs, ss)
    assert ev <= limit and es <= limit, ("mis-designed case: the float64 reference itself is off by %.2e (value) / %.2e (derivative)" % (ev, es), sp)
    return dict(value=vm, status=stm, sens=dm, vs=vs, ss=ss, tol_v=max(1e-12, 32 * ev), tol_s=max(1e-12, 32 * es), e_cpu=max(ev, es))


def references(specs, f, H, dH, limit=1e-12):
    runs_mp, runs_f64 = {}, {}
    return [reference(sp, f, H, dH, runs_mp, runs_f64, limit) for sp in specs]


@functools.lru_cache(maxsize=None)
def expected(nf):
    """[variant][spec] -> reference(...), with all N_PAR derivatives; computed once per grid size."""
    f, specs = grid(nf), specs_for(nf)
    return [references(specs, f, *variant_rows(nf, v)) for v in range(N_VARIANTS)]


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
            ev, es = figure_errors(specs[k], float(val[k, s]), [float(x) for x in sens[k, :n_par, s]] if n_par else [], r["value"], r["sens"][:n_par] if n_par else [],
                                   r["vs"], r["ss"])
            w = worst.setdefault(kind, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], ev), max(w[1], es), max(w[2], r["e_cpu"])
            if not (ev <= r["tol_v"] and es <= r["tol_s"]):
                bad.append("%s measure %d (%s %s) sample %d: value error %.3e (allowed %.3e), derivative error %.3e (allowed %.3e)" % (
                    what, k, kind, specs[k]["s1"]["sig"], s, ev, r["tol_v"], es, r["tol_s"]))
    if verbose:
        for kind, (ev, es, ec) in sorted(worst.items()):
            print("%s %-9s worst scaled error: value %.3e, derivative %.3e (float64 reference: %.3e)" % (what, kind, ev, es, ec))
    assert not bad, "\n".join(bad[:20])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))
