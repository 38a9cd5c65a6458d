"""The reference of the device-math tests: every rule of csrc/va_rt.hpp and every dense DN rule of csrc/ch_bsim4.hpp from its
MATHEMATICAL definition in 60-digit mpmath, partial derivatives by mp.diff of that definition — nothing here restates a formula of
the headers.  HIP-free; a plain helper module (no fixtures, no test collection); computed once per importing module (`reference()`).

Piecewise functions are differentiated on the branch the semantics select at the point.  The selection rules, each with the line
of va_rt.hpp it restates:
  v_min / v_max   on a tie the SECOND operand (:180-181, :207-208: `a < b ? a : b`, `a > b ? a : b`);
  v_abs           +-0 keeps x, so the slope there is +1 (:203: `val(x) < 0 ? -x : x`);
  v_limexp        the exponential below 80, linear FROM exactly 80 with the value and slope of e^80 (:164, :206);
  to_int          half away from zero (:235) — a table in device_math_cases.py;
  NaNMath (:138-159, :175-178, src/va_env.jl:35-47): ln, sqrt, log10 outside the domain give NaN and ln 0 = -inf; pow of a negative
  base with a non-integer exponent gives NaN; asin, acos, acosh, atanh outside their domain give NaN — tables in device_math_cases.py.

ADMISSION.  Some rules cancel by construction (1 - tanh^2, the second partials of hypot, atan2 and pow): they lose digits in any
fp64 evaluation, host or device, as they do in ForwardDiff.  A (point, output) pair is judged on the device only where the HOST
instantiation of va_rt.hpp is within ADMIT_ULP of the reference, and at least ADMIT_SHARE of every rule's points must be admitted
for every output (test_device_math_reference.py asserts both).  Where the reference is zero by structure (the second derivative of a
product, the partial of a variable the rule does not see) the output must be +-0.0 and is always judged."""
import numpy as np
from mpmath import mp, mpf

import device_math_cases as DC

mp.dps = 60
ADMIT_ULP, ADMIT_SHARE = 6.0, 0.90
U = 2.0 ** -53
STRUCTURAL_ZERO = mpf(10) ** -35      # a derivative below this (relative to 1 and to |f|) is a structural zero: mp.diff's own noise is 1e-55


def _min(x, y, c, x0, y0): return x if x0 < y0 else y
def _max(x, y, c, x0, y0): return x if x0 > y0 else y


RULE_F = {
    "exp": lambda x, y, c, x0, y0: mp.exp(x), "ln": lambda x, y, c, x0, y0: mp.log(x), "log10": lambda x, y, c, x0, y0: mp.log10(x),
    "sqrt": lambda x, y, c, x0, y0: mp.sqrt(x), "sin": lambda x, y, c, x0, y0: mp.sin(x), "cos": lambda x, y, c, x0, y0: mp.cos(x),
    "tan": lambda x, y, c, x0, y0: mp.tan(x), "sinh": lambda x, y, c, x0, y0: mp.sinh(x), "cosh": lambda x, y, c, x0, y0: mp.cosh(x),
    "tanh": lambda x, y, c, x0, y0: mp.tanh(x), "atan": lambda x, y, c, x0, y0: mp.atan(x), "asin": lambda x, y, c, x0, y0: mp.asin(x),
    "acos": lambda x, y, c, x0, y0: mp.acos(x), "asinh": lambda x, y, c, x0, y0: mp.asinh(x), "acosh": lambda x, y, c, x0, y0: mp.acosh(x),
    "atanh": lambda x, y, c, x0, y0: mp.atanh(x),
    "abs": lambda x, y, c, x0, y0: -x if x0 < 0 else x,
    "floor": lambda x, y, c, x0, y0: mp.floor(x0) + 0 * x, "ceil": lambda x, y, c, x0, y0: mp.ceil(x0) + 0 * x,
    "limexp": lambda x, y, c, x0, y0: mp.exp(x) if x0 < 80 else mp.exp(80) * (1 + (x - 80)),
    "rcp": lambda x, y, c, x0, y0: 1 / x, "neg": lambda x, y, c, x0, y0: -x, "seed": lambda x, y, c, x0, y0: x,
    "add": lambda x, y, c, x0, y0: x + y, "sub": lambda x, y, c, x0, y0: x - y, "mul": lambda x, y, c, x0, y0: x * y,
    "div": lambda x, y, c, x0, y0: x / y, "vdiv": lambda x, y, c, x0, y0: x / y, "min": _min, "max": _max,
    "hypot": lambda x, y, c, x0, y0: mp.sqrt(x * x + y * y), "atan2": lambda x, y, c, x0, y0: mp.atan2(x, y),
    "pow_vv": lambda x, y, c, x0, y0: x ** y, "add_assign": lambda x, y, c, x0, y0: x + y, "sub_assign": lambda x, y, c, x0, y0: x - y,
    "pow_vc": lambda x, y, c, x0, y0: x ** c, "pow_vi": lambda x, y, c, x0, y0: x ** c, "pow_cv": lambda x, y, c, x0, y0: c ** x,
    "vdiv_vc": lambda x, y, c, x0, y0: x / c, "vdiv_cv": lambda x, y, c, x0, y0: c / x,
}
for _op, _f, _r in (("add", lambda a, b: a + b, lambda a, b: b + a), ("sub", lambda a, b: a - b, lambda a, b: b - a),
                    ("mul", lambda a, b: a * b, lambda a, b: b * a), ("div", lambda a, b: a / b, lambda a, b: b / a)):
    for _s in ("vc", "vi"):
        RULE_F["%s_%s" % (_op, _s)] = (lambda f: lambda x, y, c, x0, y0: f(x, c))(_f)
    for _s in ("cv", "iv"):
        RULE_F["%s_%s" % (_op, _s)] = (lambda f: lambda x, y, c, x0, y0: f(x, c))(_r)
assert set(RULE_F) == set(DC.RULES)


def _clean(v, f):
    v = mp.re(v)
    return mpf(0) if abs(v) < STRUCTURAL_ZERO * max(1, abs(f)) else v


def derivatives(name, x0, y0, c0):
    """f, fx, fy, fxx, fxy, fyy of rule `name` at (x0, y0) as mpf; exact zeros where the rule does not see y"""
    F = RULE_F[name]
    x0, y0, c0 = mpf(float(x0)), mpf(float(y0)), mpf(float(c0))
    f2 = lambda x, y: F(x, y, c0, x0, y0)   # noqa: E731
    f = mp.re(f2(x0, y0))
    if name in DC.UNARY or name.endswith(("_vc", "_cv", "_vi", "_iv")):
        f1 = lambda x: F(x, y0, c0, x0, y0)   # noqa: E731
        return f, _clean(mp.diff(f1, x0), f), mpf(0), _clean(mp.diff(f1, x0, 2), f), mpf(0), mpf(0)
    d = lambda i, j: _clean(mp.diff(f2, (x0, y0), (i, j)), f)   # noqa: E731
    return f, d(1, 0), d(0, 1), d(2, 0), d(1, 1), d(0, 2)


def vd_outputs(kind, f, fx, fy, fxx, fxy, fyy):
    """what tests/device_math_rules.hpp run_vd1 / run_vd2 write, from the derivatives: the nested type carries x as outer variable 0 and
    inner variable 0, y as 1 and 1; ddx1(r, 0) and ddx2(r, 0, 1) = (d/dx - d/dy)/2 follow, value and outer partials"""
    if kind == DC.K_VD1:
        return [f, fx, fy]
    h = mpf(1) / 2
    return [f, fx, fy, fx, fy, fxx, fxy, fxy, fyy, fx, fxx, fxy, h * (fx - fy), h * (fxx - fxy), h * (fxy - fyy), mpf(0)]


def ulp_error(got, ref):
    """|got - ref| in units of the spacing of fp64 at ref (the normal-number ulp; below the normal range the subnormal spacing)"""
    got = float(got)
    if not np.isfinite(got):
        return np.inf
    r = float(ref)
    sp = np.spacing(abs(r)) if np.isfinite(r) else np.spacing(DC.MAXF)
    return float(abs(mpf(got) - ref) / mpf(float(sp)))


_cache = {}


def reference():
    """group name -> list (points) of lists (outputs) of mpf, for the groups judged 'vd', 'exact', 'limexp80' and 'seed1'; once"""
    if _cache:
        return _cache
    der = {}
    for g in DC.GROUPS:
        if g.judge in ("vd", "exact", "limexp80"):
            rows = []
            for x, y, c in g.data[:, :3]:
                key = (g.rule_name if g.judge != "limexp80" else "limexp", float(x), float(y), float(c), bool(np.signbit(x)), bool(np.signbit(y)))
                if key not in der:
                    der[key] = derivatives(key[0], x, y, c)
                rows.append(vd_outputs(g.kind, *der[key]))
            _cache[g.name] = rows
        elif g.judge == "seed1":
            rows = []
            for x, is_dir, dk in g.data[:, :3]:
                x, s = mpf(float(x)), mpf(1 if is_dir else 0)
                f, f1, f2 = mp.sin(x), mp.diff(mp.sin, x), mp.diff(mp.sin, x, 2)
                inner = [f1 if dk == k else mpf(0) for k in (0, 1)]
                rows.append([f, s * f1, f] + inner + [s * f1] + [s * f2 if dk == k else mpf(0) for k in (0, 1)])
            _cache[g.name] = rows
    return _cache


def errors(out, g):
    """(points, outputs) ulp errors of results `out` on group g; inf where a structural zero of the reference is not +-0.0"""
    ref = reference()[g.name]
    e = np.zeros((len(ref), len(ref[0])))
    for i, row in enumerate(ref):
        for j, r in enumerate(row):
            got = out[g.lo + i, j]
            e[i, j] = (0.0 if got == 0.0 else np.inf) if r == 0 else ulp_error(got, r)
    return e


def structural(g):
    """(points, outputs) True where the reference is zero by structure"""
    return np.array([[r == 0 for r in row] for row in reference()[g.name]])


def admitted(host_out, g):
    """(points, outputs) True where the host instantiation is within ADMIT_ULP of the reference"""
    return errors(host_out, g) <= ADMIT_ULP


# ---- scalars ----
def scalar_exact(name, a, b=0.0):
    a, b = mpf(float(a)), mpf(float(b))
    return {"rcp": lambda: 1 / a, "frcp": lambda: 1 / a, "vdiv": lambda: a / b, "sqrt": lambda: mp.sqrt(a), "fsqrt": lambda: mp.sqrt(a),
            "pow": lambda: mp.re(mp.power(a, b))}[name]()


MIN_NORMAL = mpf(2) ** -1022
MAX_FINITE = mpf(DC.MAXF)


# ---- the dense DN rules: value and one partial of a rule applied to a(t) = a + a' t, b(t) = b + b' t ----
DN_F = {"mul": lambda a, b, c, c2: a * b, "div": lambda a, b, c, c2: a / b, "recip": lambda a, b, c, c2: 1 / a, "sqrt": lambda a, b, c, c2: mp.sqrt(a),
        "exp_lit": lambda a, b, c, c2: mp.exp(a), "exp_lds": lambda a, b, c, c2: mp.exp(a), "log_lit": lambda a, b, c, c2: mp.log(a),
        "log_lds": lambda a, b, c, c2: mp.log(a), "div_c": lambda a, b, c, c2: a / c, "c_div": lambda a, b, c, c2: c / a}


def dn_reference(op, a, ap, b, bp, c, c2):
    """(value, partial) of a dense rule; chain(a, f, f') is BY DEFINITION the value f with the partial f' a'"""
    a, ap, b, bp, c, c2 = (mpf(float(v)) for v in (a, ap, b, bp, c, c2))
    if op == "chain":
        return c, c2 * ap
    F = DN_F[op]
    return F(a, b, c, c2), mp.diff(lambda t: F(a + ap * t, b + bp * t, c, c2), mpf(0))


# ---- judges shared by the CPU test (host instantiation) and the GPU test (device) ----
def same(got, want):
    """NaN matches NaN; everything else must be equal"""
    return bool((np.isnan(got) and np.isnan(want)) or got == want)


def special_failures(out, bound_ulp):
    """The groups judged 'table', 'exact', 'limexp80' and 'seed1' on results `out`: a list of what is wrong, empty if nothing is"""
    bad = []
    for g in DC.GROUPS:
        if g.judge == "table":
            for i, row in enumerate(g.expect):
                for j, want in enumerate(row):
                    if want is not None and not same(out[g.lo + i, j], want):
                        bad.append((g.name, g.data[i].tolist(), j, out[g.lo + i, j], want))
                sb = getattr(g, "signbit", None)
                if sb is not None and bool(np.signbit(out[g.lo + i, 0])) != sb:
                    bad.append((g.name, g.data[i].tolist(), "sign of zero", out[g.lo + i, 0], sb))
        elif g.judge == "exact":
            for i, row in enumerate(reference()[g.name]):
                for j, want in enumerate(row):
                    if not out[g.lo + i, j] == float(want):
                        bad.append((g.name, g.data[i].tolist(), j, out[g.lo + i, j], float(want)))
                if g.rule_name in ("min", "max", "abs") and out[g.lo + i, 0] == 0.0:   # the operand the rule keeps, with its sign
                    keep = g.data[i, 0] if g.rule_name == "abs" else g.data[i, 1]
                    if np.signbit(out[g.lo + i, 0]) != np.signbit(keep):
                        bad.append((g.name, g.data[i].tolist(), "sign of zero", out[g.lo + i, 0], keep))
        elif g.judge in ("limexp80", "seed1"):
            e = errors(out, g)
            if not e.max() <= bound_ulp:
                bad.append((g.name, "ulp", e.max()))
            if g.judge == "limexp80":
                o = out[g.lo]   # x = 80 exactly: slope == value, no curvature
                if o[1] != o[0] or (g.kind == DC.K_VD2 and (o[3] != o[0] or o[5] != 0.0 or o[9] != o[0])):
                    bad.append((g.name, "slope != value at 80", o[:6].tolist()))
    return bad


def ieee(g):
    """what IEEE arithmetic (numpy) gives on a scalar group, with the NaNMath rules of va_rt.hpp"""
    a = g.data[:, 0]
    b = g.data[:, 1] if g.data.shape[1] > 1 else None
    with np.errstate(all="ignore"):
        if g.rule in (DC.S["rcp"], DC.S["frcp"]): return 1.0 / a
        if g.rule == DC.S["vdiv"]: return a / b
        if g.rule in (DC.S["sqrt"], DC.S["fsqrt"]): return np.where(a >= 0, np.sqrt(np.abs(a)), np.nan)
        if g.rule == DC.S["pow"]: return DC.nanmath_pow(a, b)
    raise KeyError(g.name)


IEEE_GROUPS = ("s_rcp_special", "s_vdiv_special", "s_sqrt_special", "s_pow_special", "s_pow_negative_fraction")


def ieee_failures(out):
    bad = []
    for name in IEEE_GROUPS:
        g = DC.BY_NAME[name]
        bad += [(name, g.data[i].tolist(), float(p), float(q)) for i, (p, q) in enumerate(zip(out[g.lo:g.hi, 0], ieee(g))) if not same(p, q)]
    return bad
