"""CPU half of the device-math tests: the mpmath reference of tests/device_math_reference.py against closed forms, and the HOST
instantiation of csrc/va_rt.hpp (tests/host_device_math.cpp, built sanitized) against that reference — the admission condition the
GPU test (tests/test_gpu_device_math.py) relies on, the special-value tables, and the exact special cases."""
import numpy as np
import pytest
from mpmath import mp, mpf

import device_math_cases as DC
import device_math_reference as DR
from test_host_analysis_fuzz import build_sanitized


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("device_math_host")
    return DC.run_program(build_sanitized(d, "host_device_math.cpp", "host_device_math"), d, "host")


def test_reference_reproduces_closed_forms():
    tol = mpf(10) ** -45
    x = mpf(1.7)   # the fp64 number the rule is evaluated at
    f, fx, _, fxx, _, _ = DR.derivatives("pow_vc", 1.7, 0.0, 2.5)
    assert abs(f - x ** mpf("2.5")) < tol and abs(fx - mpf("2.5") * x ** mpf("1.5")) < tol
    assert abs(fxx - mpf("3.75") * mp.sqrt(x)) < tol                      # d2/dx2 x^2.5 = 3.75 sqrt(x)
    a, b = mpf("0.75"), mpf("-2.5")                                       # atan2(first, second): mixed partial (first^2 - second^2) / r^4
    _, f1, f2, _, f12, _ = DR.derivatives("atan2", 0.75, -2.5, 0.0)
    r2 = a * a + b * b
    assert abs(f12 - (a * a - b * b) / r2 ** 2) < tol and abs(f1 - b / r2) < tol and abs(f2 + a / r2) < tol
    f, fx, _, fxx, _, _ = DR.derivatives("limexp", 85.0, 0.0, 0.0)       # linear from 80: slope e^80, value 6 e^80, no curvature
    assert abs(fx / mp.exp(80) - 1) < tol and abs(f / mp.exp(80) - 6) < tol and fxx == 0
    _, fx, _, fxx, _, _ = DR.derivatives("limexp", 79.9, 0.0, 0.0)
    assert abs(fx / mp.exp(mpf(79.9)) - 1) < tol and abs(fxx / mp.exp(mpf(79.9)) - 1) < tol
    _, fx, fy, fxx, fxy, fyy = DR.derivatives("mul", 3.0, -2.0, 0.0)     # structural zeros are exact zeros
    assert (fx, fy, fxx, fxy, fyy) == (-2, 3, 0, 1, 0)
    _, fx, fy, _, _, _ = DR.derivatives("min", 1.5, 1.5, 0.0)            # a tie: the second operand
    assert (fx, fy) == (0, 1)
    _, fx, _, _, _, _ = DR.derivatives("abs", -0.0, 0.0, 0.0)            # +-0 keeps x
    assert fx == 1
    assert DR.ulp_error(1.0 + 2.0 ** -52, mpf(1)) == 1.0 and DR.ulp_error(5e-324, mpf(0) + mpf(2) ** -1074 * 2) == 1.0


def test_case_sets_are_as_specified():
    for g in DC.GROUPS:
        assert len(g.data) <= 128 or g.name == "s_flog", (g.name, len(g.data))
        assert g.hi - g.lo == len(g.data) and np.array_equal(DC.RECORDS[g.lo:g.hi, 2:2 + g.data.shape[1]], g.data, equal_nan=True)
    x = DC.BY_NAME["s_rcp"].data[:, 0]
    assert np.all(np.isfinite(x)) and np.all(x != 0) and (x < 0).any() and (np.abs(x) > 2.0 ** 1022).any() and (np.abs(x) < 2.0 ** -1022).any()
    for e in DC.EXPONENTS:
        for m in DC.MANTISSAS:
            assert np.ldexp(m, e) in x
    assert np.array_equal(DC.BY_NAME["s_frcp"].data, DC.BY_NAME["s_rcp"].data) and np.array_equal(DC.BY_NAME["s_vdiv"].data[:, 1], x)
    a, b = DC.BY_NAME["s_pow_special"].data.T
    assert len(a) == len(DC.POW_SPECIAL_A) * len(DC.POW_SPECIAL_B) and (b == 1e15).any() and (b == 1e16).any()
    a, b = DC.BY_NAME["s_pow_general"].data.T
    assert len(a) >= 64 and np.all(np.abs(b * np.log(a)) < 700) and a.min() < 1e-20 and a.max() > 1e20
    a, b = DC.BY_NAME["s_pow_negative"].data.T
    assert np.all(a < 0) and np.all(b == np.floor(b)) and (b % 2 == 1).any() and (b % 2 == 0).any()
    a, b = DC.BY_NAME["s_pow_negative_fraction"].data.T
    assert np.all(a < 0) and np.all(b != np.floor(b))
    assert len(DC.BY_NAME["s_flog"].data) == 42008 + 4
    for name in ("vd1_atan2", "vd2_atan2", "vd1_hypot", "vd2_hypot"):   # all four quadrants
        x, y = DC.BY_NAME[name].data[:, :2].T
        assert {(bool(p), bool(q)) for p, q in zip(x > 0, y > 0)} == {(True, True), (True, False), (False, True), (False, False)}
    # every pair of per-partial states is in some instantiation of every binary DN operator, every state in every unary one
    for n in (3, 1):
        assert {p for j in range(DC.NB[n]) for p in DC.bin_states(n, j)} == {(a, b) for a in range(5) for b in range(5)}
        assert {s for j in range(DC.NU[n]) for s in DC.un_states(n, j)} == set(range(5))
        assert any(g.dense for g in DC.GROUPS if g.judge == "dn" and g.n == n and g.form == 0)


def test_host_is_admitted_on_nine_tenths_of_every_rule(host):
    """The admission condition and its cap: the library-path instantiation within 6 ulp of the reference on >= 90 % of the points of
    every output of every rule, first order and nested; structural zeros are +-0.0 everywhere.  Prints the worst host error per rule."""
    short = []
    for g in DC.GROUPS:
        if g.judge != "vd":
            continue
        e = DR.errors(host, g)
        z = DR.structural(g)
        assert np.all(e[z] == 0.0), (g.name, "a structural zero is not +-0.0")
        share = (e <= DR.ADMIT_ULP).mean(axis=0)
        fin = np.where(np.isfinite(e), e, 0.0)
        print("%-16s admitted %5.1f %% (worst output)   worst admitted error %.2f ulp   worst error %.3g ulp" % (
            g.name, 100 * share.min(), np.where(e <= DR.ADMIT_ULP, e, 0.0).max(), fin.max()))
        if share.min() < DR.ADMIT_SHARE:
            short.append((g.name, int(np.argmin(share)), float(share.min())))
    assert not short, short


def test_host_special_values_and_exact_cases(host):
    """The tables of device_math_cases.py (NaNMath domains, ties, zero bases, to_int / clamp_index / truth) and the cases that are exact
    (b == 0, a.v == 0 with b = 1 and 2, limexp at exactly 80), on the host instantiation; 6 ulp where a value is not exact."""
    bad = DR.special_failures(host, DR.ADMIT_ULP)
    assert not bad, bad
    bad = DR.ieee_failures(host)
    assert not bad, bad
