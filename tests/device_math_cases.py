"""The records that tests/host_device_math.cpp (host instantiation of csrc/va_rt.hpp) and tests/gpu_device_math.hip (device paths
of va_rt.hpp and ch_bsim4.hpp) evaluate: seeded and fixed, shared by test_host_device_math.py, test_device_math_reference.py and
test_gpu_device_math.py.  A plain helper module, HIP-free: no fixtures, no test collection.

One record is NIN doubles [kind, rule, operands ...]; one result is NOUT doubles (tests/device_math_rules.hpp has the layout).
A GROUP is a run of records of one rule with what judges it:
  'vd'               value and partials against the mpmath reference at admitted points (device_math_reference.py admits);
  'exact'            every output equal to the reference value (ties, +-0, zero bases with b = 1 and 2, b == 0, floor / ceil);
  'table'            outputs written out by hand where the definition is a table and not a formula (None: not specified):
                     the NaNMath domains, the scalar tie rules, x^0.5 at 0, zero bases with VD exponents, the integer helpers;
  'limexp80'         the slope equals the value at exactly 80, the exponential one fp64 number below;
  'seed1'            sin of a one-directional seed;
  'recip' / 'sqrt'   the scalar primitives against 1/x, a/b and sqrt x; 'ieee' their special values; 'flog' both constant sources;
  'pow_bound' / 'pow_exact'   the scalar v_pow by its error bound / exactly against IEEE pow with the NaNMath rule;
  'dn'               one DN operator in one instantiation of per-partial states: sparse and dense result side by side.
The ranges of the 'vd' groups keep the host instantiation within 6 ulp of the reference on at least 90 % of the points of every
output; where a rule cancels by construction the comment next to its range says what was left out."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cedarsim.jl_amd", "csrc")
NIN, NOUT = 12, 16
K_SCALAR, K_VD1, K_VD2, K_INT, K_DN, K_SEED1 = range(6)
NPTS = 48          # points per 'vd' rule (the cap is 128)

# tests/device_math_rules.hpp enum Rule, in order
RULES = ("exp ln log10 sqrt sin cos tan sinh cosh tanh atan asin acos asinh acosh atanh abs floor ceil limexp rcp neg "
         "add sub mul div vdiv min max hypot atan2 pow_vv add_assign sub_assign "
         "add_vc add_cv add_vi add_iv sub_vc sub_cv sub_vi sub_iv mul_vc mul_cv mul_vi mul_iv div_vc div_cv div_vi div_iv "
         "vdiv_vc vdiv_cv pow_vc pow_vi pow_cv seed").split()
R = {n: i for i, n in enumerate(RULES)}
SCALARS = "rcp frcp vdiv sqrt fsqrt flog pow limexp hypot atan2 min max abs ln log10 asin acos acosh atanh".split()
S = {n: i for i, n in enumerate(SCALARS)}
I_TO_INT, I_CLAMP, I_TRUTH, I_ABS_INT, I_MINMAX_INT = range(5)
UNARY = set("exp ln log10 sqrt sin cos tan sinh cosh tanh atan asin acos asinh acosh atanh abs floor ceil limexp rcp neg seed".split())
POW_RULES = ("pow_vv", "pow_vc", "pow_vi", "pow_cv")   # carry the 5 |b ln a| term of the scalar v_pow


class Group:
    def __init__(self, name, kind, rule, data, judge, **kw):
        self.name, self.kind, self.rule, self.judge = name, kind, rule, judge
        self.data = np.atleast_2d(np.asarray(data, dtype=np.float64))
        self.lo = self.hi = 0
        self.__dict__.update(kw)

    def records(self):
        r = np.zeros((len(self.data), NIN))
        r[:, 0], r[:, 1] = self.kind, self.rule
        r[:, 2:2 + self.data.shape[1]] = self.data
        return r


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _sign(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _away(rng, lo, hi, n, holes, w):
    """uniform in [lo, hi] but no closer than w to any of holes"""
    out = []
    while len(out) < n:
        v = rng.uniform(lo, hi)
        if all(abs(v - h) >= w for h in holes):
            out.append(v)
    return np.array(out)


def vd_points(name, rng, n=NPTS):
    """(x, y, c) of rule `name`: the ranges of the measurements in DESIGN 4 (host instantiation against mpmath)."""
    z = np.zeros(n)
    u = lambda a, b: rng.uniform(a, b, n)   # noqa: E731
    if name == "exp": return u(-30, 30), z, z
    if name in ("sin", "cos"): return u(-6, 6), z, z
    if name in ("ln", "log10"): return _logu(rng, 1e-3, 50, n), z, z
    if name == "sqrt": return _logu(rng, 1e-6, 100, n), z, z
    if name == "tan": return u(-1.4, 1.4), z, z
    if name == "atan": return u(-20, 20), z, z
    if name in ("sinh", "cosh"): return u(-10, 10), z, z
    if name == "tanh": return u(-1, 1), z, z          # 1 - tanh^2 cancels beyond: 84 ulp at +-3 on the host
    if name in ("asin", "acos", "atanh"): return u(-0.9, 0.9), z, z
    if name == "asinh": return u(-20, 20), z, z
    if name == "acosh": return u(1.1, 20), z, z
    if name in ("abs", "neg", "floor", "ceil", "seed"): return u(-9, 9), z, z
    if name == "limexp": return np.concatenate((u(-30, 79.9)[:n - 3], [79.9, 80.0, 85.0])), z, z
    if name == "rcp": return _logu(rng, 1e-3, 1e3, n) * _sign(rng, n), z, z
    if name in ("add", "sub", "mul", "min", "max", "add_assign", "sub_assign"): return u(-9, 9), u(-9, 9), z
    if name in ("div", "vdiv"): return _logu(rng, 0.1, 9, n) * _sign(rng, n), _logu(rng, 0.1, 9, n) * _sign(rng, n), z
    if name in ("hypot", "atan2"):
        # all four quadrants, 0.5 <= |x/y| <= 2 but a factor 1.25 away from 1.  hypot's second partials y^2/r^3, -xy/r^3 come out of a
        # sum of four terms that cancels as the ratio leaves that band; atan2's mixed partial (first^2 - second^2)/r^4 vanishes on the
        # diagonals; and ddx2 = (d/dx - d/dy)/2 of either has its own zeros at |x| = |y| (hypot) and |x/y| = sqrt(2) -+ 1 (atan2)
        y = _logu(rng, 0.5, 9, n) * np.tile([1.0, 1.0, -1.0, -1.0], n)[:n]
        ratio = np.where(rng.random(n) < 0.5, _logu(rng, 0.5, 0.8, n), _logu(rng, 1.25, 2.0, n))
        sx = np.tile([1.0, -1.0, 1.0, -1.0], n)[:n]
        if name == "hypot":
            # with x and y of opposite sign ddx2 is (y^2 - |xy|)/r^3 and (|xy| - x^2)/r^3: two to five times the error of second partials
            # that are 4 ulp off on their own, anywhere in the band (measured: the host is within 6 ulp at half of such points).  Those
            # two quadrants get one point in six, so that they are there and the 90 % still hold
            sx = np.where(np.arange(n) % 6 == 5, -np.sign(y), np.sign(y))
        return np.abs(y) * ratio * sx, y, z
    if name == "pow_vv":  # the y-partials carry ln x and 1/x together: y stays 0.2 away from 0 and 1, x 0.1 away from 1
        return np.where(rng.random(n) < 0.5, u(0.5, 0.9), u(1.1, 2.0)), _away(rng, -2, 2, n, (0.0, 1.0), 0.2), z
    if name == "pow_vc": return _logu(rng, 0.1, 10, n), z, rng.choice([2.5, -3.0, 0.5, 2.0, 1.7, -1.3], n)
    if name == "pow_vi": return _logu(rng, 0.1, 10, n) * _sign(rng, n), z, rng.choice([-6, -3, -2, -1, 2, 3, 4, 5, 6], n).astype(float)
    if name == "pow_cv": return _away(rng, -2, 2, n, (0.0,), 0.2), z, np.where(rng.random(n) < 0.5, u(0.5, 0.9), u(1.1, 2.0))
    if name.endswith(("_vi", "_iv")): return _logu(rng, 0.1, 9, n) * _sign(rng, n), z, rng.choice([-7, -3, -2, -1, 1, 2, 3, 5], n).astype(float)
    if name.endswith(("_vc", "_cv")): return _logu(rng, 0.1, 9, n) * _sign(rng, n), z, _logu(rng, 0.1, 9, n) * _sign(rng, n)
    raise KeyError(name)


def pow_term(name, x, y, c):
    """|b ln a| of the pow a rule goes through"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if name == "pow_vv": return np.abs(y * np.log(np.abs(x)))
        if name in ("pow_vc", "pow_vi"): return np.abs(c * np.log(np.abs(x)))
        if name == "pow_cv": return np.abs(x * np.log(np.abs(c)))
    return np.zeros_like(x)


# ------------------------------------------------------------------------------------------------------------------------------
# scalars
def _magnitudes(rng, n):
    return np.exp2(rng.uniform(-1020, 1020, n))


MANTISSAS = (1.0, 1.0 + 2.0 ** -52, 1.5, 2.0 - 2.0 ** -52)
EXPONENTS = (-1021, -512, -1, 0, 1, 511, 1020)
MAXF, MINSUB, MAXSUB = 1.7976931348623157e308, 5e-324, 2.225073858507201e-308


def reciprocal_arguments(rng):
    """finite non-zero arguments of va::rcp, chip::frcp and (as divisor) va::v_div"""
    grid = np.array([np.ldexp(m, e) for e in EXPONENTS for m in MANTISSAS])
    big = np.array([np.ldexp(1.0 + 2.0 ** -52, 1022), np.ldexp(1.5, 1022), np.ldexp(1.0, 1023), np.ldexp(1.75, 1023), MAXF])   # 1/x is subnormal
    sub = np.array([MINSUB, np.ldexp(1.0, -1030), np.ldexp(1.5, -1024), np.ldexp(1.0, -1023), np.ldexp(1.5, -1023), MAXSUB])  # 1/x overflows for the first two
    x = np.concatenate((_magnitudes(rng, 48) * _sign(rng, 48), grid, -grid[::3], big, -big[:2], sub, -sub[3:5]))
    assert len(x) <= 128
    return x


def sqrt_arguments(rng):
    return np.concatenate((_magnitudes(rng, 64), [MINSUB, MAXSUB, MAXF, np.ldexp(1.0, -1022), 4.0, 9.0, 0.25, 1e10, 2.0 ** 100, 2.0 ** -100,
                                                  49.0, 1.0, 3.0 ** 30, (2.0 ** 26 + 1) ** 2]))


def flog_arguments():
    """The arguments test_gpu_va.test_device_exp_and_ln_accuracy gives ch_debug_math for which = 2: the same generator, the same
    draws in the same order."""
    rng = np.random.default_rng(11)
    rng.uniform(-745.0, 709.7, 20000), rng.uniform(-2.0, 2.0, 20000), rng.uniform(-1e-8, 1e-8, 2000)
    for which in (1, 2):
        xl = np.concatenate((np.exp(rng.uniform(-700.0, 700.0, 20000)), rng.uniform(0.5, 2.0, 20000), 1.0 + rng.uniform(-1e-6, 1e-6, 2000),
                             np.array([1.0, 2.0, 0.5, np.sqrt(0.5), np.sqrt(2.0), 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308])))
    return np.concatenate((xl, [0.0, -1.0, np.inf, np.nan]))


POW_SPECIAL_A = (0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0)
POW_SPECIAL_B = (0.0, -0.0, np.inf, -np.inf, np.nan, 0.5, -0.5, 3.0, -3.0, 2.0, 1e15, 1e16, 999999999999999.0)   # |b| < 1e15 is the device's own path


def nanmath_pow(a, b):
    """IEEE pow with the NaNMath rule of va_rt.hpp:175/178 (src/va_env.jl:35-47): a negative base with a non-integer exponent is NaN"""
    with np.errstate(all="ignore"):
        return np.where((a < 0.0) & (b != np.floor(b)), np.nan, np.power(a, b))


def pow_cases(rng):
    """name -> (a, b); 'general' is judged by the error bound, everything else exactly"""
    a = _logu(rng, 1e-30, 1e30, 400)
    b = rng.uniform(-8, 8, 400)
    keep = np.abs(b * np.log(a)) < 700
    a, b = a[keep][:96], b[keep][:96]
    ib = rng.integers(-6, 7, 32).astype(float)
    neg = -_logu(rng, 1e-3, 1e3, 32)
    nb = rng.integers(-7, 8, 32).astype(float)        # odd and even
    frac = _away(rng, -5, 5, 16, tuple(range(-5, 6)), 0.05)
    ga, gb = np.meshgrid(POW_SPECIAL_A, POW_SPECIAL_B, indexing="ij")
    return {"general": (a, b), "integer": (_logu(rng, 1e-3, 1e3, 32), ib), "negative": (neg, nb), "negative_fraction": (neg[:16], frac),
            "special": (ga.ravel(), gb.ravel())}


# ------------------------------------------------------------------------------------------------------------------------------
# DN
B_OPS = "add sub mul div".split()
U_OPS = "neg add_c c_add sub_c c_sub mul_c c_mul div_c c_div recip chain sqrt exp_lit exp_lds log_lit log_lds widen".split()
STATE_NAMES = ("ZP", "ZN", "ZR", "PR", "PX")
NB = {3: 10, 1: 25}
NU = {3: 6, 1: 5}


def dn_code(n, form, inst, op):
    return n * 10000 + form * 1000 + inst * 20 + op


def bin_states(n, j):
    """per partial: (state of a, state of b) in instantiation j (gpu_device_math.hip bin_state)"""
    cs = [j if n == 1 else (18 if j == 9 else (3 * j + i) % 25) for i in range(n)]
    return [(c // 5, c % 5) for c in cs]


def un_states(n, j):
    return [j if n == 1 else (3 if j == 5 else (j + i) % 5) for i in range(n)]


def dn_dense(n, form, j):
    return all(s >= 3 for p in bin_states(n, j) for s in p) if form == 0 else all(s >= 3 for s in un_states(n, j))


def dn_groups(rng):
    out = []
    for n in (3, 1):
        for form, ops, cnt in ((0, B_OPS, NB[n]), (1, U_OPS, NU[n])):
            for j in range(cnt):
                for k, op in enumerate(ops):
                    m = 16 if dn_dense(n, form, j) else 4
                    d = _logu(rng, 0.1, 10, (m, 10)) * np.where(rng.random((m, 10)) < 0.5, -1.0, 1.0)
                    if op in ("sqrt", "log_lit", "log_lds"):    # positive; ln stays away from its zero at 1 (the 2 ulp of flog are of |ln x|)
                        d[:, 0] = np.where(rng.random(m) < 0.5, _logu(rng, 1e-3, 0.5, m), _logu(rng, 2.0, 1e3, m))
                    if op in ("exp_lit", "exp_lds"):
                        d[:, 0] = rng.uniform(-30, 30, m)
                    out.append(Group("dn%d_%s_%s" % (n, op, j), K_DN, dn_code(n, form, j, k), d, "dn", n=n, form=form, inst=j, op=op,
                                     dense=dn_dense(n, form, j)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
def build_groups():
    rng = np.random.default_rng(20240611)
    g = []
    # scalars
    xr = reciprocal_arguments(rng)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    g.append(Group("s_rcp", K_SCALAR, S["rcp"], np.c_[xr], "recip"))
    g.append(Group("s_frcp", K_SCALAR, S["frcp"], np.c_[xr], "recip"))
    # a * rcp(b): a reciprocal that is subnormal has lost its low bits before a multiplies it, so beyond 2^1021 (and for subnormal b,
    # whose reciprocal overflows for every a >= 1) the numerator is 1 and v_div is held to what rcp is held to
    num = np.where((np.abs(xr) > 2.0 ** 1021) | (np.abs(xr) < 2.0 ** -1021), 1.0, _logu(rng, 2.0 ** -40, 2.0 ** 40, len(xr)) * _sign(rng, len(xr)))
    num = np.where(np.abs(np.log2(np.abs(xr)) - np.log2(np.abs(num))) > 1000, 1.0, num)
    g.append(Group("s_vdiv", K_SCALAR, S["vdiv"], np.c_[num, xr], "recip"))
    g.append(Group("s_rcp_special", K_SCALAR, S["rcp"], np.c_[sp], "ieee"))
    g.append(Group("s_vdiv_special", K_SCALAR, S["vdiv"], np.array([(a, b) for a in (1.5, -2.0, 0.0, np.inf, np.nan) for b in sp]), "ieee"))
    xs = sqrt_arguments(rng)
    g.append(Group("s_sqrt", K_SCALAR, S["sqrt"], np.c_[xs], "sqrt"))
    g.append(Group("s_fsqrt", K_SCALAR, S["fsqrt"], np.c_[xs], "sqrt"))
    g.append(Group("s_sqrt_special", K_SCALAR, S["sqrt"], np.c_[np.array([0.0, -0.0, np.inf, -1.0, -np.inf, np.nan, -MINSUB])], "ieee"))
    g.append(Group("s_flog", K_SCALAR, S["flog"], np.c_[flog_arguments()], "flog"))
    for nm, (a, b) in pow_cases(rng).items():
        g.append(Group("s_pow_" + nm, K_SCALAR, S["pow"], np.c_[a, b], "pow_bound" if nm in ("general", "integer", "negative") else "pow_exact"))
    # the NaNMath domain rules and the tie rules of the scalar functions (the VD forms select on them)
    nm_tab = [("ln", -1.0, np.nan), ("ln", 0.0, -np.inf), ("ln", -0.0, -np.inf), ("ln", np.nan, np.nan), ("ln", np.inf, np.inf),
              ("log10", -1.0, np.nan), ("log10", 0.0, -np.inf), ("log10", 100.0, 2.0),
              ("asin", 1.0000000000000002, np.nan), ("asin", -1.5, np.nan), ("acos", 1.0000000000000002, np.nan), ("acos", -2.0, np.nan),
              ("acosh", 0.9999999999999999, np.nan), ("acosh", 1.0, 0.0), ("atanh", 1.0, np.nan), ("atanh", -1.0, np.nan), ("atanh", 1.5, np.nan),
              ("abs", -0.0, 0.0), ("abs", -2.5, 2.5)]
    for k, (fn, x, want) in enumerate(nm_tab):
        g.append(Group("s_dom_%s_%d" % (fn, k), K_SCALAR, S[fn], [[x, 0.0]], "table", expect=[[want]]))
    tie_tab = [("min", 1.5, 1.5, 1.5, None), ("min", 0.0, -0.0, 0.0, True), ("min", -0.0, 0.0, 0.0, False), ("max", 0.0, -0.0, 0.0, True),
               ("max", -0.0, 0.0, 0.0, False), ("min", 1.0, 2.0, 1.0, None), ("max", 1.0, 2.0, 2.0, None),
               ("hypot", 3.0, 4.0, 5.0, None), ("hypot", 0.0, 0.0, 0.0, None)]
    for k, (fn, x, y, want, neg) in enumerate(tie_tab):   # v_min / v_max return the SECOND operand on a tie (va_rt.hpp:180-181): its sign of zero
        g.append(Group("s_tie_%s_%d" % (fn, k), K_SCALAR, S[fn], [[x, y]], "table", expect=[[want]], signbit=neg))
    # VD rules, first order and nested
    for name in RULES:
        x, y, c = vd_points(name, rng)
        for kind in (K_VD1, K_VD2):
            g.append(Group("vd%d_%s" % (kind, name), kind, R[name], np.c_[x, y, c], "vd", rule_name=name, bl=pow_term(name, x, y, c)))
    # special cases, exact against the reference with the branch the semantics select
    ex = {"min": [(1.5, 1.5), (0.0, -0.0), (-0.0, 0.0), (2.0, 2.0)], "max": [(1.5, 1.5), (0.0, -0.0), (-0.0, 0.0), (-3.0, -3.0)],
          "abs": [(0.0, 0.0), (-0.0, 0.0), (-2.0, 0.0), (2.0, 0.0)],
          "pow_vc": [(0.0, 0.0, 1.0), (0.0, 0.0, 2.0), (3.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-2.0, 0.0, 0.0)],
          "pow_vi": [(0.0, 0.0, 1.0), (0.0, 0.0, 2.0), (3.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-2.0, 0.0, 0.0)],
          "floor": [(2.5, 0.0), (-2.5, 0.0), (3.0, 0.0)], "ceil": [(2.5, 0.0), (-2.5, 0.0), (3.0, 0.0)],
          "add": [(1.5, 2.25)], "sub": [(1.5, 2.25)], "mul": [(1.5, 2.25)], "neg": [(1.5, 0.0)], "seed": [(1.5, 0.0)]}
    for name, pts in ex.items():
        d = np.zeros((len(pts), 3))
        for k, p in enumerate(pts):
            d[k, :len(p)] = p
        for kind in (K_VD1, K_VD2):
            g.append(Group("vd%d_exact_%s" % (kind, name), kind, R[name], d, "exact", rule_name=name))
    # tables: what the definition gives where no derivative exists.  x^0.5 at 0: value 0, slope +inf (0.5 * 0^-0.5); the partial of the
    # variable the rule does not depend on is inf * 0 there, as in ForwardDiff, and is not specified.  A zero base with a VD exponent:
    # the constant 0 for a positive exponent, the constant NaN otherwise (va_rt.hpp:226-227), both with zero partials.
    N_, Z, NAN, INF = None, 0.0, np.nan, np.inf
    g.append(Group("vd1_table_pow_half", K_VD1, R["pow_vc"], [[0.0, 0.0, 0.5]], "table", expect=[[Z, INF, N_]]))
    g.append(Group("vd2_table_pow_half", K_VD2, R["pow_vc"], [[0.0, 0.0, 0.5]], "table", expect=[[Z, INF, N_, INF, N_] + [N_] * 11]))
    zero16, nan16 = [Z] * 16, [NAN] + [Z] * 15
    for nm, rule, pt, e1, e2 in (("zero_pos", "pow_vv", (0.0, 1.5, 0.0), [Z, Z, Z], zero16), ("zero_zero", "pow_vv", (0.0, 0.0, 0.0), [NAN, Z, Z], nan16),
                                 ("zero_neg", "pow_vv", (0.0, -1.0, 0.0), [NAN, Z, Z], nan16), ("neg_base", "pow_vv", (-2.0, 2.0, 0.0), [NAN, Z, Z], nan16),
                                 ("c_zero_pos", "pow_cv", (2.0, 0.0, 0.0), [Z, Z, Z], zero16), ("c_zero_neg", "pow_cv", (-2.0, 0.0, 0.0), [NAN, Z, Z], nan16)):
        g.append(Group("vd1_table_" + nm, K_VD1, R[rule], [pt], "table", expect=[e1]))
        g.append(Group("vd2_table_" + nm, K_VD2, R[rule], [pt], "table", expect=[e2]))
    # limexp is linear from EXACTLY 80 (va_rt.hpp:206): there the slope is the value, (80 - 79) e^80, and the curvature is zero
    g.append(Group("vd1_limexp_80", K_VD1, R["limexp"], [[80.0, 0.0, 0.0], [np.nextafter(80.0, 0.0), 0.0, 0.0]], "limexp80"))
    g.append(Group("vd2_limexp_80", K_VD2, R["limexp"], [[80.0, 0.0, 0.0], [np.nextafter(80.0, 0.0), 0.0, 0.0]], "limexp80"))
    # integer helpers.  to_int rounds half away from zero (va_rt.hpp:235): [to_int(double), to_int(VD), to_int(nested VD), to_int(int)]
    ti = [(0.5, 1), (-0.5, -1), (1.5, 2), (-1.5, -2), (2.5, 3), (-2.5, -3), (2.0 ** 31 - 1 - 0.5, 2 ** 31 - 1), (-(2.0 ** 31 - 1) - 0.5, -2 ** 31),
          (0.0, 0), (-0.0, 0), (0.4, 0), (-0.4, 0), (0.6, 1), (-0.6, -1), (7.0, 7), (-7.0, -7), (1e6 + 0.5, 1000001)]
    g.append(Group("int_to_int", K_INT, I_TO_INT, [[x, -5.0] for x, _ in ti], "table", expect=[[float(w), float(w), float(w), -5.0] for _, w in ti]))
    ci = [(i, lo, hi) for lo, hi in ((0, 4), (-3, 2), (5, 5)) for i in (lo - 7, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, hi + 9)]
    g.append(Group("int_clamp", K_INT, I_CLAMP, np.array(ci, dtype=float), "table", expect=[[float(min(max(i, lo), hi) - lo)] for i, lo, hi in ci]))
    tr = [(0.0, 0, 0.0), (-0.0, 0, 0.0), (1e-300, 1, 1.0), (-2.0, -1, 1.0), (MINSUB, 7, 1.0), (np.inf, 0, 0.0)]
    g.append(Group("int_truth", K_INT, I_TRUTH, np.array(tr), "table",
                   expect=[[float(x != 0.0), float(i != 0), float(b != 0.0), float(x != 0.0), float(x != 0.0)] for x, i, b in tr]))
    g.append(Group("int_abs", K_INT, I_ABS_INT, [[-3.0], [3.0], [0.0]], "table", expect=[[3.0], [3.0], [0.0]]))
    g.append(Group("int_minmax", K_INT, I_MINMAX_INT, [[2.0, 5.0], [5.0, 2.0], [-4.0, -4.0]], "table", expect=[[2.0, 5.0], [2.0, 5.0], [-4.0, -4.0]]))
    # one-directional seeds: sin(seed1(x, is_dir, dk)) on VD<1, double> and VD<1, VD<2, double>>
    xs1 = rng.uniform(-3, 3, 8)
    g.append(Group("seed1", K_SEED1, 0, np.c_[xs1, np.tile([1.0, 0.0], 4), np.tile([-1.0, 0.0, 1.0, 1.0], 2)], "seed1"))
    g += dn_groups(rng)
    lo = 0
    for gr in g:
        gr.lo, gr.hi = lo, lo + len(gr.data)
        lo = gr.hi
    return g


GROUPS = build_groups()
RECORDS = np.ascontiguousarray(np.vstack([gr.records() for gr in GROUPS]))
BY_NAME = {gr.name: gr for gr in GROUPS}
assert len(BY_NAME) == len(GROUPS)


def run_program(exe, tmp_dir, tag):
    """exe <records> <results>, once, under a time limit; returns the (records, NOUT) results"""
    fin, fout = os.path.join(str(tmp_dir), tag + "_in.bin"), os.path.join(str(tmp_dir), tag + "_out.bin")
    RECORDS.tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, (r.stdout + r.stderr)[-3000:])
    out = np.fromfile(fout, dtype=np.float64)
    assert out.size == len(RECORDS) * NOUT, (out.size, len(RECORDS))
    return out.reshape(len(RECORDS), NOUT)


def build_host(tmp_dir, include=CSRC):
    """tests/host_device_math.cpp with plain g++ (the library path of va_rt.hpp); test_host_device_math.py builds the sanitized one"""
    exe = os.path.join(str(tmp_dir), "host_device_math")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", include, os.path.join(ROOT, "tests", "host_device_math.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe
