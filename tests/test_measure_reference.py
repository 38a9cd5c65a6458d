"""The yardstick of the waveform measurements (tests/measure_reference.py) pinned on closed forms.  Polynomial waveforms of degree <= 5
sampled at non-uniform times with full dense points: from interval 5 on the interpolant IS the polynomial, so crossing times, end
values of windows and their parameter derivatives are known exactly.  The 40-digit run must hit them to 1e-30, the float64 run to 1e-12."""
import math

import mpmath
import numpy as np
import pytest

import measure_reference as mr

T = np.array([0.0, 0.11, 0.19, 0.33, 0.42, 0.58, 0.66, 0.81, 0.97, 1.08, 1.2, 1.31, 1.5])
PTS = np.minimum(np.arange(len(T)) + 1, 6)
P = 1.7


def rows_and_sens():
    """Row 0: y = p (t - 0.1)^5 (dy/dp = (t - 0.1)^5); row 1: z = 2 - 3 t + t^2 (dz/dp = 0); row 2: u = p t (du/dp = t)."""
    y = np.array([P * (T - 0.1) ** 5, 2 - 3 * T + T * T, P * T])
    s = np.array([[(T - 0.1) ** 5], [0 * T], [T]])
    return y, s


def both(sp):
    y, s = rows_and_sens()
    return mr.measure_mp(sp, T, PTS, y, s), mr.measure_f64(sp, T, PTS, y, s)


def check(sp, value, deriv):
    (vm, sm, dm), (vf, sf, df) = both(sp)
    assert sm == 0 and sf == 0
    assert abs(vm - value) < 1e-30 * max(1, abs(value)) and abs(dm[0] - deriv) < 1e-30 * max(1, abs(deriv)), (vm, dm)
    assert abs(vf - float(value)) < 1e-12 * max(1, abs(value)) and abs(df[0] - float(deriv)) < 1e-11 * max(1, abs(deriv)), (vf, df)


def test_crossing_time_and_its_derivative():
    with mpmath.workdps(40):
        p = mpmath.mpf(P)
        L = float(p * mpmath.mpf("0.9") ** 5)            # a float level: the crossing is where p (t - 0.1)^5 equals THAT number
        ts = mpmath.mpf("0.1") + (mpmath.mpf(L) / p) ** (mpmath.mpf(1) / 5)
        # the rows hold float(P (T - 0.1)^5), not the polynomial itself: the yardstick's answer belongs to the rows.  Their rounding moves
        # the crossing by ~1e-16, so the closed form pins the 40-digit run to 1e-14 here and exactly on exactly representable rows below
        (vm, sm, dm), (vf, sf, df) = both(mr.spec("when", mr.side(0, level=L, edge="rise")))
        assert sm == 0 and abs(vm - ts) < 1e-14 and abs(dm[0] + (ts - mpmath.mpf("0.1")) / (5 * p)) < 1e-13
        assert sf == 0 and abs(vf - float(ts)) < 1e-13


def exact_rows():
    """Integer times and integer-valued polynomials: every row is exact in float64.  y = t^3 - 30 t (p = 1: dy/dp = t^3), z = 7 t."""
    t = np.array([0.0, 1.0, 2.0, 4.0, 5.0, 7.0, 8.0, 11.0, 12.0])
    return t, np.minimum(np.arange(len(t)) + 1, 4), np.array([t ** 3 - 30 * t, 7 * t]), np.array([[t ** 3], [0 * t]])


def test_exact_rows_give_exact_answers():
    t, pts, y, s = exact_rows()
    with mpmath.workdps(40):
        # y = 150 where t^3 - 30 t - 150 = 0: one real root, between 6 and 7 (interval 5, a cubic through rows 2..5)
        root = mpmath.findroot(lambda x: x ** 3 - 30 * x - 150, 6.8)
        dt = -(root ** 3) / (3 * root ** 2 - 30)
        for run, tol in ((mr.measure_mp, 1e-30), (mr.measure_f64, 1e-13)):
            v, st, d = run(mr.spec("when", mr.side(0, level=150.0, edge="rise")), t, pts, y, s)
            assert st == 0 and abs(v - root) < tol * 10 and abs(d[0] - dt) < tol * 10
            # z at that time and its derivative: 7 t*, 7 dt*/dp
            v, st, d = run(mr.spec("find_when", mr.side(0, level=150.0, edge="rise"), mr.side(1)), t, pts, y, s)
            assert st == 0 and abs(v - 7 * root) < tol * 100 and abs(d[0] - 7 * dt) < tol * 100
            # delay from z = 21 (t = 3) to the crossing
            v, st, d = run(mr.spec("delay", mr.side(1, level=21.0), mr.side(0, level=150.0, edge="rise")), t, pts, y, s)
            assert st == 0 and abs(v - (root - 3)) < tol * 10 and abs(d[0] - dt) < tol * 10
            # the cubic itself between rows: y(6) = 36, dy/dp = 216
            v, st, d = run(mr.spec("find_at", mr.side(0), at=6.0), t, pts, y, s)
            assert st == 0 and abs(v - 36) < tol * 100 and abs(d[0] - 216) < tol * 1000
            # window [4.5, 7.5]: points 4.5 (-43.875), 5 (-25), 7 (133), 7.5 (196.875): trapezoid 0.25 (-68.875) + 108 + 0.25 (329.875) = 173.25
            v, st, d = run(mr.spec("integ", mr.side(0), frm=4.5, to=7.5), t, pts, y, s)
            assert st == 0 and abs(v - 173.25) < tol * 1000
            # on dy/dp = t^3: 0.25 (91.125 + 125) + (125 + 343) + 0.25 (343 + 421.875) = 713.25
            assert abs(d[0] - 713.25) < tol * 1000
            v, st, d = run(mr.spec("avg", mr.side(0), frm=4.5, to=7.5), t, pts, y, s)
            assert abs(v - 57.75) < tol * 1000 and abs(d[0] - 237.75) < tol * 1000
            v, st, d = run(mr.spec("min", mr.side(0), frm=4.5, to=7.5), t, pts, y, s)
            assert v == -43.875 and abs(d[0] - 91.125) < tol * 1000
            v, st, d = run(mr.spec("pp", mr.side(0), frm=4.5, to=7.5), t, pts, y, s)
            assert abs(v - 240.75) < tol * 1000 and abs(d[0] - (421.875 - 91.125)) < tol * 1000
            # rms of z = 7 t over [0, 12] by the trapezoid rule on the rows: a line's square is not integrated exactly; worked out from the rows
            zz = [(7 * float(x)) ** 2 for x in t]
            sq = sum((zz[j - 1] + zz[j]) * (float(t[j]) - float(t[j - 1])) / 2 for j in range(1, len(t)))
            v, st, d = run(mr.spec("rms", mr.side(1)), t, pts, y, s)
            assert st == 0 and abs(v - mpmath.sqrt(mpmath.mpf(sq) / 12)) < tol * 100 and d[0] == 0


def test_line_windows_are_exact():
    # u = p t: the trapezoid rule is exact: integral over [0.25, 1.4] = p (1.96 - 0.0625) / 2, average p (1.4 + 0.25) / 2; d/dp without the p
    with mpmath.workdps(40):
        p, a, b = mpmath.mpf(P), mpmath.mpf(0.25), mpmath.mpf(1.4)
        (vm, sm, dm), (vf, sf, df) = both(mr.spec("integ", mr.side(2), frm=0.25, to=1.4))
        # (rows are float(P T): each within half an ulp of the line, hence 1e-15 and not 1e-30)
        assert sm == 0 and abs(vm - p * (b * b - a * a) / 2) < 1e-15 and abs(dm[0] - (b * b - a * a) / 2) < 1e-15
        assert sf == 0 and abs(vf - float(p * (b * b - a * a) / 2)) < 1e-14
        (vm, sm, dm), _ = both(mr.spec("max", mr.side(2, scale=-2.0), frm=0.25, to=1.4))
        assert abs(vm + 2 * p * a) < 1e-15 and abs(dm[0] + 2 * a) < 1e-15   # -2 u is largest at the from point


@pytest.mark.parametrize("sp, status", [
    (mr.spec("when", mr.side(0, level=1e3)), 1),
    (mr.spec("when", mr.side(0, level=0.01, edge="fall")), 1),
    (mr.spec("when", mr.side(0, level=0.01, edge="rise", td=1.45)), 1),
    (mr.spec("avg", mr.side(0), frm=0.5, to=0.5), 2),
    (mr.spec("avg", mr.side(0), frm=2.0, to=3.0), 2),
])
def test_statuses(sp, status):
    for v, st, d in both(sp):
        assert st == status and math.isnan(v) and math.isnan(d[0])


def test_nan_rows_and_the_span_read():
    y, s = rows_and_sens()
    y = y.copy()
    y[0, 9] = np.nan
    L = float(y[0, 6] + y[0, 7]) / 2     # crossed in interval 7, in front of the NaN row
    for run in (mr.measure_mp, mr.measure_f64):
        assert run(mr.spec("when", mr.side(0, level=L, edge="rise", count=1)), T, PTS, y, s)[1] == 0
        assert run(mr.spec("when", mr.side(0, level=L, edge="rise", count=-1)), T, PTS, y, s)[1] == 3     # the last event: the whole run is read
        assert run(mr.spec("when", mr.side(0, level=L, edge="rise", count=2)), T, PTS, y, s)[1] == 3
        assert run(mr.spec("max", mr.side(0), frm=0.0, to=0.9), T, PTS, y, s)[1] == 0
        assert run(mr.spec("max", mr.side(0), frm=0.0, to=1.0), T, PTS, y, s)[1] == 3                      # the end value's polynomial reads row 9
        assert run(mr.spec("find_at", mr.side(0), at=1.25), T, PTS, y, s)[1] == 3 and run(mr.spec("find_at", mr.side(1), at=1.25), T, PTS, y, s)[1] == 0


def test_dense_eval_is_the_interpolant():
    """find_at is solution._dense_eval, and a line between the rows of a saveat grid (no dense points)."""
    from cedarsim_jl_amd.solution import _dense_eval
    y, s = rows_and_sens()
    tq = [0.05, 0.3, 0.58, 0.9, 1.45]
    want = _dense_eval(T, PTS, y[1], np.array(tq))
    for x, w in zip(tq, want):
        assert abs(mr.measure_f64(mr.spec("find_at", mr.side(1), at=x), T, PTS, y)[0] - w) < 1e-14
        assert abs(mr.measure_f64(mr.spec("find_at", mr.side(1), at=x), T, None, y)[0] - np.interp(x, T, y[1])) < 1e-15
