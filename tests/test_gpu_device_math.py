"""The device arithmetic under every device evaluation, held to a 60-digit reference (run with `-m gpu` on an MI355X):
  * csrc/va_rt.hpp under __HIP_DEVICE_COMPILE__: rcp / sqrt_pos / ln_pos / v_pow built on v_rcp_f64, v_rsq_f64 and frexp, and every VD
    chain rule on top of them, first order (VD<2, double>) and nested (VD<2, VD<2, double>>, what ddx() runs on);
  * csrc/ch_bsim4.hpp: frcp, fsqrt, flog from both constant sources, and the DN<N, S> algebra in every combination of per-partial
    states, sparse against dense and dense against the reference.
tests/gpu_device_math.hip is built once (the library's own flags, csrc/Makefile) and run once on the records of
tests/device_math_cases.py; tests/device_math_reference.py has the reference and the admission rule.  The host instantiation
(tests/host_device_math.cpp) is run next to it: it decides which (point, output) pairs are judged.

frcp has no guard: frcp(+-0), frcp(+-inf) and frcp of an argument whose reciprocal overflows are NaN by construction
(e = fma(-x, r, 1) is NaN or infinite there).  That is its contract; check_primitives prints what it gives there and judges it
where the exact reciprocal is a finite number.  test_gpu_bsim4_cards.py (far-bias rows) shows that no model path reaches such an
argument."""
import os
import subprocess

import numpy as np
import pytest
from mpmath import mpf

import device_math_cases as DC
import device_math_reference as DR

pytestmark = pytest.mark.gpu

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
VD_BOUND = 2 * DR.ADMIT_ULP    # twice the admission bound: every device primitive is specified at 2 ulp where the library's is at most 1, and
                               # cancellation amplifies both alike


def build_gpu(tmp_dir, include=DC.CSRC):
    exe = os.path.join(str(tmp_dir), "gpu_device_math")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", include, os.path.join(DC.ROOT, "tests", "gpu_device_math.hip"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    d = tmp_path_factory.mktemp("device_math_gpu")
    return DC.run_program(build_gpu(d), d, "gpu")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("device_math_host")
    return DC.run_program(DC.build_host(d), d, "host")


# ---- 1 ----
def check_primitives(dev):
    bad = []
    for name in ("s_rcp", "s_frcp", "s_vdiv", "s_sqrt", "s_fsqrt"):
        g = DC.BY_NAME[name]
        fn = DC.SCALARS[g.rule]
        want_ieee = DR.ieee(g)
        worst, worst_sub = 0.0, 0.0
        for i, row in enumerate(g.data):
            got = dev[g.lo + i, 0]
            exact = DR.scalar_exact(fn, *row)
            if abs(exact) > DR.MAX_FINITE:              # the reciprocal overflows: IEEE's answer where there is a guard
                if fn == "frcp":
                    print("frcp(%r) = %r: no guard, not judged (1/x overflows)" % (row[0], got))
                elif not DR.same(got, want_ieee[i]):
                    bad.append((name, row.tolist(), got, want_ieee[i]))
                continue
            e = DR.ulp_error(got, exact)
            if abs(exact) >= DR.MIN_NORMAL:
                worst = max(worst, e)
                if not e <= 2.0:
                    bad.append((name, row.tolist(), got, float(exact), "%.2f ulp" % e))
            else:                                       # a subnormal result: one unit of the subnormal spacing
                worst_sub = max(worst_sub, e)
                if not e <= 1.0:
                    bad.append((name, row.tolist(), got, float(exact), "%.2f subnormal spacings" % e))
        print("%-8s worst error %.3f ulp (normal results), %.3f spacings (subnormal results), %d points" % (name, worst, worst_sub, len(g.data)))
    bad += [b for b in DR.ieee_failures(dev) if b[0] in ("s_rcp_special", "s_vdiv_special", "s_sqrt_special")]
    return bad


def test_primitives_within_2_ulp_and_ieee_special_values(dev):
    bad = check_primitives(dev)
    assert not bad, bad


# ---- 2 ----
def check_flog(dev):
    g = DC.BY_NAME["s_flog"]
    lit, lds = dev[g.lo:g.hi, 0], dev[g.lo:g.hi, 1]
    nan = np.isnan(lit)
    differ = np.where(nan, ~np.isnan(lds), lit.view(np.int64) != lds.view(np.int64))
    x = g.data[:, 0]
    ok = np.isfinite(x) & (x > 0)
    with np.errstate(all="ignore"):
        assert np.array_equal(lit[~ok], np.log(x[~ok]), equal_nan=True), lit[~ok]     # 0 -> -inf, negative / NaN -> NaN, inf -> inf
    return [(float(x[i]), float(lit[i]), float(lds[i])) for i in np.nonzero(differ)[0][:10]]


def test_flog_from_lds_equals_flog_from_literals_bit_for_bit(dev):
    bad = check_flog(dev)
    assert not bad, bad


# ---- 3 ----
def check_pow(dev):
    """Relative error of the device v_pow at most u (5 |b ln a| + 4), u = 2^-53:
         ln a within 2 ulp (the bound test_gpu_va.test_device_exp_and_ln_accuracy holds it to): at most 4u relative, so b ln a is off by
           4u |b ln a|; the product b * ln a adds half an ulp, at most u |b ln a|: the argument of exp is off by at most 5u |b ln a|
           absolute, which is the relative error it leaves in the result;
         exp within 2 ulp: at most 4u relative.
       (one ulp is at most 2u relative.)  The sign rule, the NaN rule and the special grid are exact: NaN matches NaN, everything else
       must be equal (IEEE pow + the NaNMath rule)."""
    bad = []
    for name in ("s_pow_general", "s_pow_integer", "s_pow_negative"):
        g = DC.BY_NAME[name]
        worst = 0.0
        for i, (a, b) in enumerate(g.data):
            got = dev[g.lo + i, 0]
            exact = DR.scalar_exact("pow", a, b)
            bound = DR.U * (5.0 * abs(b * np.log(abs(a))) + 4.0)
            rel = float(abs(mpf(float(got)) - exact) / abs(exact)) if np.isfinite(got) else np.inf
            worst = max(worst, rel / bound)
            if not rel <= bound:
                bad.append((name, a, b, got, float(exact), rel, bound))
        print("%-16s worst relative error / bound %.3f" % (name, worst))
    bad += [b for b in DR.ieee_failures(dev) if b[0].startswith("s_pow")]
    return bad


def test_scalar_pow_error_bound_sign_rule_and_special_grid(dev):
    bad = check_pow(dev)
    assert not bad, bad


# ---- 4, 5 ----
def check_vd(dev, host, kind):
    bad = []
    for g in DC.GROUPS:
        if g.judge != "vd" or g.kind != kind:
            continue
        adm = DR.admitted(host, g) | DR.structural(g)
        e = DR.errors(dev, g)
        # rules that go through the device v_pow carry its 5 |b ln a| (check_pow), in ulp: one ulp is at least u relative
        bound = VD_BOUND + (5.0 * g.bl[:, None] if g.rule_name in DC.POW_RULES else 0.0) + np.zeros_like(e)
        if kind == DC.K_VD2:
            # ddx2 = (p - q) / 2 is a difference of two partials, each of which has the bound above in ITS ulp; the subtraction adds
            # half an ulp of the result and the halving is exact.  In ulp of the result that is bound * (ulp p + ulp q) / (2 ulp r) + 0.5:
            # the plain bound where nothing cancels, more where p and q are close (counted, not measured: the issue's rule for a finding)
            ref = DR.reference()[g.name]
            sp = lambda v: np.spacing(abs(float(v)))   # noqa: E731
            for j, (p, q) in ((12, (3, 4)), (13, (5, 6)), (14, (7, 8))):
                for i, row in enumerate(ref):
                    if row[j] != 0:
                        bound[i, j] = bound[i, j] * (sp(row[p]) + sp(row[q])) / (2.0 * sp(row[j])) + 0.5
        over = adm & ~(e <= bound)
        fin = np.where(adm & np.isfinite(e), e, 0.0)
        print("%-16s worst device error at admitted points %.2f ulp (value %.2f, partials %.2f)   admitted %d of %d" % (
            g.name, fin.max(), fin[:, 0].max(), fin[:, 1:].max(), int(adm.sum()), adm.size))
        for i, j in zip(*np.nonzero(over)):
            bad.append((g.name, g.data[i, :3].tolist(), int(j), float(dev[g.lo + i, j]), float(DR.reference()[g.name][i][j]), float(e[i, j])))
    return bad


def test_vd_rules_first_order(dev, host):
    bad = check_vd(dev, host, DC.K_VD1)
    assert not bad, bad[:20]


def test_vd_rules_nested_second_and_mixed_partials_and_ddx(dev, host):
    bad = check_vd(dev, host, DC.K_VD2)
    assert not bad, bad[:20]


# ---- 6 ----
def test_vd_special_cases_and_integer_helpers_are_exact(dev):
    bad = DR.special_failures(dev, VD_BOUND)
    assert not bad, bad


# ---- 7 ----
def check_dn_sparse_against_dense(dev):
    """For every operator and every combination of per-partial states of its operands, the sparse result (widened) == the same
    operator on the operands widened first.  `==` lets the sign of a zero pass: the one difference ch_bsim4.hpp allows."""
    bad = []
    for g in DC.GROUPS:
        if g.judge != "dn":
            continue
        sparse, dense = dev[g.lo:g.hi, 0:4], dev[g.lo:g.hi, 4:8]
        states = DC.bin_states(g.n, g.inst) if g.form == 0 else DC.un_states(g.n, g.inst)
        if not (np.all(np.isfinite(sparse)) and np.all(sparse == dense)):
            i = int(np.nonzero(~(np.isfinite(sparse) & (sparse == dense)).all(axis=1))[0][0])
            bad.append((g.name, [tuple(DC.STATE_NAMES[s] for s in p) if g.form == 0 else DC.STATE_NAMES[p] for p in states],
                        g.data[i].tolist(), sparse[i].tolist(), dense[i].tolist()))
    return bad


def test_dn_sparse_equals_dense_in_every_state_combination(dev):
    bad = check_dn_sparse_against_dense(dev)
    assert not bad, bad[:10]


# ---- 8 ----
# ulp per rule, counted: 2 per device primitive (frcp, fsqrt, fexp, flog), half per +, x or fma; one ulp is at most 2^-52 relative.
# Each partial is judged against the sum of the magnitudes of its rule's terms, the value against its own magnitude.
#   rule      value                          partial
DN_COUNT = {
    "mul":     (0.5,                          1.0),   # a*b | a*b' (0.5), fma(a', b, .) (0.5): of |a' b| + |a b'|
    "div":     (2.5,                          5.5),   # r = frcp(b) (2), q = a*r (0.5) | q (2.5), fma(-q, b', a') (0.5), * r (2 + 0.5): of (|a'| + |a/b| |b'|)/|b|
    "recip":   (2.0,                          5.0),   # r (2) | m = -r*r (2 + 2 + 0.5), a'*m (0.5)
    "sqrt":    (2.0,                          4.5),   # s = fsqrt(a) (2) | frcp(s) (2 + the 2 of s), 0.5* (exact), a'* (0.5)
    "exp_lit": (2.0,                          2.5),   # e = fexp(a) (2) | a'*e (0.5)
    "exp_lds": (2.0,                          2.5),
    "log_lit": (2.0,                          2.5),   # flog(a) (2, of |ln a|) | frcp(a) (2), a'* (0.5)
    "log_lds": (2.0,                          2.5),
    "chain":   (0.0,                          0.5),   # f as given | a'*f' (0.5)
    "div_c":   (2.5,                          2.5),   # a * frcp(c): (2 + 0.5) both
    "c_div":   (2.5,                          5.5),   # recip(a) * c: recip + 0.5
}


def dn_terms(op, a, ap, b, bp, c, c2):
    """sum of the magnitudes of the terms of the partial of rule `op`"""
    if op == "mul": return abs(ap * b) + abs(a * bp)
    if op == "div": return (abs(ap) + abs(a / b) * abs(bp)) / abs(b)
    if op == "recip": return abs(ap) / (a * a)
    if op == "sqrt": return abs(ap) / (2.0 * np.sqrt(a))
    if op in ("exp_lit", "exp_lds"): return abs(ap) * np.exp(a)
    if op in ("log_lit", "log_lds"): return abs(ap / a)
    if op == "chain": return abs(c2 * ap)
    if op == "div_c": return abs(ap / c)
    if op == "c_div": return abs(c * ap) / (a * a)
    raise KeyError(op)


def check_dn_dense_against_reference(dev):
    bad = []
    worst = {}
    for g in DC.GROUPS:
        if g.judge != "dn" or not g.dense or g.op not in DN_COUNT:
            continue
        cv, cp = DN_COUNT[g.op]
        for i, d in enumerate(g.data):
            a, b, c, c2 = d[0], d[4], d[8], d[9]
            dense = dev[g.lo + i, 4:8]
            for k in range(g.n):
                ap, bp = d[1 + k], d[5 + k]
                val, par = DR.dn_reference(g.op, a, ap, b, bp, c, c2)
                ev = float(abs(mpf(float(dense[0])) - val) / abs(val)) / 2.0 ** -52
                ep = float(abs(mpf(float(dense[1 + k])) - par)) / (dn_terms(g.op, a, ap, b, bp, c, c2) * 2.0 ** -52)
                w = worst.setdefault((g.n, g.op), [0.0, 0.0])
                w[0], w[1] = max(w[0], ev), max(w[1], ep)
                if not (ev <= cv and ep <= cp):
                    bad.append((g.name, d.tolist(), k, dense.tolist(), float(val), float(par), ev, ep))
    for (n, op), (ev, ep) in sorted(worst.items()):
        print("DN<%d> %-8s worst value error %.2f of %.1f ulp   worst partial error %.2f of %.1f ulp of the rule's terms" % (n, op, ev, DN_COUNT[op][0], ep, DN_COUNT[op][1]))
    assert len(worst) == 2 * len(DN_COUNT)
    return bad


def test_dn_dense_rules_against_the_reference(dev):
    bad = check_dn_dense_against_reference(dev)
    assert not bad, bad[:10]
