"""The yardstick of the frequency-domain measurements (tests/fmeasure_reference.py) pinned on closed forms: on the exact single pole
H = A / (1 + j f / fc) and on a three-pole response whose phase passes -180 degrees, the discrete bandwidth, unity-gain frequency and
phase-crossover frequency converge to the closed forms at second order as the grid is refined, and every sensitivity formula equals a
40-digit central difference of the yardstick's own discrete measure on the same grid.  No GPU."""
import math

import mpmath
import numpy as np
import pytest

import fmeasure_reference as fr

mp = mpmath.mp


def _grid(u0, decades, ppd):
    return [mpmath.power(10, u0 + mpmath.mpf(i) / ppd) for i in range(decades * ppd + 1)]


def _pole1(f, A, fc):
    return [A / (1 + 1j * x / fc) for x in f]


def _pole3(f, A, f1, f2, f3):
    return [A / ((1 + 1j * x / f1) * (1 + 1j * x / f2) * (1 + 1j * x / f3)) for x in f]


def _measure(f, rows, sp):
    v, st, _ = fr._measure(fr._MP, f, [rows], None, sp)
    assert st == 0
    return v


def _place(u0, ppd_coarse, cell):
    """A frequency a third of the way into cell `cell` of the coarse grid: it then sits two thirds into a cell of the grid twice as
    fine, and the line's error factor t (1 - t) is the same 2/9 on both, so the error ratio shows the h^2 alone."""
    return mpmath.power(10, u0 + (cell + mpmath.mpf(1) / 3) / ppd_coarse)


def _second_order(errs):
    """The observed order log2(e_20 / e_40) lies within half an order of 2: a first-order rule gives 1, a third-order one 3.  (The
    ratio is 4 (1 + O(h)): the line's cubic error term changes sign between t = 1/3 and t = 2/3.)"""
    return 1.5 < mpmath.log(errs[0] / errs[1], 2) < 2.5


def test_the_discrete_measures_converge_at_second_order():
    with mpmath.workdps(40):
        u0, A = 1, mpmath.mpf(100)
        # ---- single pole: unity-gain frequency fc sqrt(A^2 - 1); bandwidth: |H|^2 falls by D dB against f_ref = the first row ----
        fug = _place(u0, 20, 57)
        fc = fug / mpmath.sqrt(A * A - 1)
        ug = fr.spec("when", fr.side(0, sig="db", level=0.0, edge="fall"))
        errs = [abs(_measure(_grid(u0, 4, n), _pole1(_grid(u0, 4, n), A, fc), ug) - fug) / fug for n in (20, 40)]
        assert _second_order(errs), errs
        D = mpmath.mpf("3.0103")
        fbw = _place(u0, 20, 31)
        xr_over_x = mpmath.power(10, u0) / fbw   # f_ref / f_bw; x^2 = 10^(D/10) (1 + xr^2) - 1 with x = f_bw / fc, xr = f_ref / fc
        q = mpmath.power(10, D / 10)
        x2 = (q - 1) / (1 - q * xr_over_x ** 2)
        fc = fbw / mpmath.sqrt(x2)
        bw = fr.spec("when", fr.side(0, sig="db", level=-float(D), edge="fall", ref_at=10.0))
        errs = [abs(_measure(_grid(u0, 4, n), _pole1(_grid(u0, 4, n), A, fc), bw) - fbw) / fbw for n in (20, 40)]
        assert _second_order(errs), errs
        # ---- three poles at (1, 30, 100) s: |H| = 1 and arg H = -180 by a 40-digit root; the poles are scaled to place each ----
        base = (mpmath.mpf(1), mpmath.mpf(30), mpmath.mpf(100))
        x_ug = mpmath.findroot(lambda x: A * A - (1 + x * x) * (1 + (x / 30) ** 2) * (1 + (x / 100) ** 2), 60)
        x_pc = mpmath.findroot(lambda x: mpmath.atan(x) + mpmath.atan(x / 30) + mpmath.atan(x / 100) - mpmath.pi, 60)
        pc = fr.spec("when", fr.side(0, sig="phase", level=-180.0, edge="fall"))
        for x0, sp, cell in ((x_ug, ug, 55), (x_pc, pc, 58)):
            target = _place(u0, 20, cell)
            s = target / x0
            errs = [abs(_measure(_grid(u0, 4, n), _pole3(_grid(u0, 4, n), A, *(s * b for b in base)), sp) - target) / target for n in (20, 40)]
            assert _second_order(errs), (errs, float(x0))


def _responses(f, p):
    """Rows (single pole, three poles) and their derivatives with respect to p = (A, fc): the three poles sit at fc, 30 fc, 100 fc."""
    A, fc = p
    r1 = _pole1(f, A, fc)
    r3 = _pole3(f, A, fc, 30 * fc, 100 * fc)
    d1 = [[h / A for h in r1], [h * (1j * x / fc ** 2) / (1 + 1j * x / fc) for h, x in zip(r1, f)]]
    d3 = [[h / A for h in r3],
          [h * sum((1j * x / (m * fc ** 2)) / (1 + 1j * x / (m * fc)) for m in (1, 30, 100)) for h, x in zip(r3, f)]]
    return [r1, r3], [d1, d3]


S = fr.side
SENS_SPECS = [
    fr.spec("when", S(0, sig="db", level=0.0, edge="fall")),
    fr.spec("when", S(0, sig="db", level=-3.0103, edge="fall", ref_at=10.0)),
    fr.spec("when", S(0, sig="db", level=-3.0103, edge="fall", ref_at=13.7), xscale="lin"),
    fr.spec("when", S(1, sig="phase", level=-180.0, edge="fall")),
    fr.spec("when", S(1, sig="mag", level=1.0, edge="cross", count=-1)),
    fr.spec("when", S(1, sig="re", level=0.0, edge="fall")),
    fr.spec("when", S(1, sig="im", level=-20.0, edge="rise", fd=300.0)),
    fr.spec("find_when", S(1, sig="db", level=0.0, edge="fall"), S(1, sig="phase")),
    fr.spec("find_when", S(1, sig="phase", level=-180.0, edge="fall"), S(1, sig="db")),
    fr.spec("find_when", S(0, sig="db", level=20.0, edge="fall"), S(1, 0, sig="mag", scale=2.0), xscale="lin"),
    fr.spec("find_at", S(1, sig="phase"), at=4321.0),
    fr.spec("find_at", S(0, sig="db"), at=77.0, xscale="lin"),
    fr.spec("find_at", S(0, sig="db10"), at=200.0),
] + [fr.spec(k, S(r, sig=g), frm=a, to=b, xscale=xs) for k in fr.WINDOW_KINDS
     for r, g, a, b, xs in ((1, "phase", 33.0, 7.7e4, "log"), (0, "mag", -math.inf, math.inf, "lin"), (1, "im", 150.0, 160.0, "log"))]


@pytest.mark.parametrize("k", range(len(SENS_SPECS)))
def test_sensitivities_equal_a_40_digit_central_difference(k):
    sp = SENS_SPECS[k]
    with mpmath.workdps(40):
        f = _grid(1, 4, 10)
        p = (mpmath.mpf(100), mpmath.mpf(150))
        rows, drows = _responses(f, p)
        v, st, ds = fr._measure(fr._MP, f, rows, drows, sp)
        assert st == 0
        for j in range(2):
            h = p[j] * mpmath.mpf(10) ** -12
            hi = fr._measure(fr._MP, f, _responses(f, tuple(q + (h if i == j else 0) for i, q in enumerate(p)))[0], None, sp)
            lo = fr._measure(fr._MP, f, _responses(f, tuple(q - (h if i == j else 0) for i, q in enumerate(p)))[0], None, sp)
            assert hi[1] == 0 and lo[1] == 0
            cd = (hi[0] - lo[0]) / (2 * h)
            assert abs(ds[j] - cd) <= mpmath.mpf(10) ** -18 * (abs(cd) + abs(v) / p[j]), (sp, j, ds[j], cd)


def test_the_float64_run_follows_the_40_digit_run():
    f = [float(x) for x in 10.0 ** np.linspace(1, 5, 41)]
    rows, drows = _responses(np.array(f), (100.0, 150.0))
    rows, drows = np.array(rows), np.array(drows)
    for sp in SENS_SPECS:
        v, st, ds = fr.measure_f64(f, rows, drows, sp)
        vm, stm, dsm = fr.measure_mp(f, rows, drows, sp)
        assert st == stm == 0
        assert abs(v - float(vm)) <= 1e-12 * max(1.0, abs(v)), sp
        for a, b in zip(ds, dsm):
            assert abs(a - float(b)) <= 1e-11 * max(1.0, abs(a)), sp


def test_statuses():
    f = [1.0, 2.0, 3.0, 4.0]
    H = np.array([[0, 1, 0, 2], [1, np.nan, 1, 1], [1, 0, 1, 1]], complex)
    for run in (fr.measure_f64, fr.measure_mp):
        assert run(f, H, None, fr.spec("when", S(0, sig="re", level=5.0), xscale="lin"))[1] == 1
        assert run(f, H, None, fr.spec("integ", S(0, sig="re"), frm=2.0, to=2.0, xscale="lin"))[1] == 2
        assert run(f, H, None, fr.spec("find_at", S(1, sig="re"), at=1.5, xscale="lin"))[1] == 3
        assert run(f, H, None, fr.spec("find_at", S(2, sig="db"), at=2.0, xscale="lin"))[1] == 3
        assert run(f, H, None, fr.spec("find_at", S(2, sig="phase"), at=2.0, xscale="lin"))[1] == 3
        v, st, _ = run(f, H, None, fr.spec("when", S(0, sig="re", level=1.0, edge="rise"), xscale="lin"))
        assert st == 0 and float(v) == 2.0   # g_i == L: the row's own frequency
        assert run(f, H, None, fr.spec("when", S(0, sig="re", level=1.0, edge="fall"), xscale="lin"))[1] == 1   # a touch from below
