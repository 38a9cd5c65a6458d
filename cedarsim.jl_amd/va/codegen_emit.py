"""Expressions and statements of one Verilog-A module as C++ text (see codegen.py for what is assembled from them).

An `Emitter` knows the module (node and parameter numbering, which variables carry derivatives); a `Pass` says what is
being emitted: `eval` over the dual type R, an analog function over its template type S, or a plain-double walk (`setup`,
`noise`, `opvars`).  Every expression yields (code, type) with type in int | real | dual.
"""
import itertools
from dataclasses import dataclass, replace

from .frontend import FLOW_ACCESS, POTENTIAL_ACCESS, VAError, _is_zero

MAX_NODES = 8

_F1 = {"exp", "ln", "sqrt", "sin", "cos", "tan", "sinh", "cosh", "tanh", "atan", "asin", "acos", "asinh", "acosh", "atanh", "abs",
       "floor", "ceil", "limexp"}
_F2 = {"pow", "min", "max", "atan2", "hypot"}
_NOISE_SOURCES = ("white_noise", "flicker_noise")
# calls whose value does not depend on their arguments (a noise source contributes no current to the stamp)
_CONSTANT_CALLS = {"$temperature": ("env.temperature", "real"), "$mfactor": ("1.0", "real"), "$port_connected": ("1", "int"), "$abstime": ("0.0", "real"),
                   "$realtime": ("0.0", "real"), "white_noise": ("0.0", "real"), "flicker_noise": ("0.0", "real")}
_VT_PER_KELVIN = "(1.3806503e-23 / 1.602176462e-19)"


@dataclass(frozen=True)
class Pass:
    S: str                    # C++ name of the scalar type that 'dual' values have in this pass
    vars: dict                # variable in scope -> int | real | dual
    plain: bool = False       # no duals at all: probes are real, block locals are double
    contrib: str = "stamp"    # what a contribution becomes: "stamp" (sums into I / Q), "noise" (a record per source), "none"
    infunc: bool = False      # inside an analog function: no probes, no contributions, every real is S
    hoist: object = None      # eval side of the setup/eval split: where bias-independent values come from (codegen_split.Hoist)


def walk(e):
    if isinstance(e, (tuple, list)):
        if isinstance(e, tuple):
            yield e
        for c in e:
            yield from walk(c)


def _has_ddt(e):
    return any(n[0] == "call" and n[1] == "ddt" for n in walk(e) if len(n) >= 2)


def is_noise_source(e):
    return e[0] == "call" and e[1] in _NOISE_SOURCES


class Emitter:
    def __init__(self, module):
        self.m = module
        if len(module.nodes) > MAX_NODES:
            raise VAError("module %s has %d nodes; the engine's stamp record holds %d" % (module.name, len(module.nodes), MAX_NODES))
        self.node_ix = {n: i for i, n in enumerate(module.nodes)}
        self.param_ix = {p[0]: i for i, p in enumerate(module.params)}
        self.ddx_nodes = self._ddx_nodes()
        self.all_vars = dict(module.vars)
        for n in walk(module.analog):
            if n and n[0] == "block" and isinstance(n[2], dict):
                self.all_vars.update(n[2])
        self.dual = set()
        self._infer_dual()
        self.tmp = itertools.count(1)   # numbers sw%d_ / o%d_ / r%d_: one sequence per module, through every function and pass

    # ---- analyses ----
    def _ddx_nodes(self):
        order = []
        for n in walk([self.m.analog] + [f.body for f in self.m.functions.values()]):
            if len(n) >= 3 and n[0] == "call" and n[1] == "ddx":
                probe = n[2][1]
                if probe[0] != "call" or probe[1] not in POTENTIAL_ACCESS:
                    raise VAError("ddx(): the second argument must be a potential probe V(a) or V(a,b)")
                for a in probe[2]:
                    if a[1] not in order:
                        order.append(a[1])
        return order

    def _is_dual(self, e):
        k = e[0]
        if k in ("num", "str"):
            return False
        if k in ("id", "index"):
            return e[1] in self.dual
        if k == "un":
            return self._is_dual(e[2])
        if k == "bin":
            if e[1] in ("<", "<=", ">", ">=", "==", "!=", "&&", "||", "&", "|", "^", "<<", ">>", "%"):
                return False
            return self._is_dual(e[2]) or self._is_dual(e[3])
        if k == "tern":
            return self._is_dual(e[2]) or self._is_dual(e[3])
        if k == "call":
            name = e[1]
            if name in POTENTIAL_ACCESS or name in FLOW_ACCESS or name == "ddx":
                return True
            if name.startswith("$") and name[1:] not in _F1 and name[1:] not in _F2 and name not in ("$limit",):
                return False
            if name in ("floor", "ceil", "$floor", "$ceil") + _NOISE_SOURCES:
                return False
            return any(self._is_dual(a) for a in e[2])
        return False

    def _infer_dual(self):
        def mark(name, cause):
            if name not in self.dual and self.all_vars.get(name) == "real" and cause():
                self.dual.add(name)
                return True
            return False
        changed = True
        while changed:
            changed = False
            for n in walk(self.m.analog):
                if not n:
                    continue
                if n[0] == "assign":
                    changed |= mark(n[1], lambda: self._is_dual(n[2]))
                if n[0] == "assign_idx":
                    changed |= mark(n[1], lambda: self._is_dual(n[3]))
                if n[0] == "call" and n[1] in self.m.functions and any(self._is_dual(a) for a in n[2]):
                    for (nm, kind), a in zip(self.m.functions[n[1]].args, n[2]):
                        if kind in ("output", "inout") and a[0] == "id":
                            changed |= mark(a[1], lambda: True)

    def q_mask(self):
        """Bit k set: node k receives a ddt() contribution somewhere in the analog block."""
        mask = 0
        for n in walk(self.m.analog):
            if not (n and n[0] == "contrib" and _has_ddt(n[3])):
                continue
            nodes = self.m.branch_nodes(n[2])
            vb = self.m.find_vbranch(nodes)
            if (n[1] in POTENTIAL_ACCESS and not _is_zero(n[3])) or (n[1] in FLOW_ACCESS and vb is not None):
                mask |= 1 << self.node_ix[vb[0]]
            elif n[1] in FLOW_ACCESS:
                for nd in nodes:
                    mask |= 1 << self.node_ix[nd]
        return mask

    def module_var_types(self):
        return {nm: "int" if ty == "integer" else ("dual" if nm in self.dual else "real") for nm, ty in self.m.vars.items() if ty != "string"}

    def local_types(self, decls, ctx):
        """types of the variables a block declares, under pass `ctx`"""
        return {nm: "int" if ty == "integer" else ("dual" if ctx.infunc or (nm in self.dual and not ctx.plain) else "real") for nm, ty in decls.items()}

    def decl(self, nm, t, scalar, pad="  "):
        suffix = " = 0"
        if nm in self.m.arrays:
            lo, hi = self.m.arrays[nm]
            suffix = "[%d] = {}" % (hi - lo + 1)
        return "%s%s v_%s%s;" % (pad, {"int": "int", "real": "double", "dual": scalar}[t], nm, suffix)

    # ---- expressions ----
    def cast(self, code, ty, to, S):
        if ty == to:
            return code
        if to == "dual":
            return "%s(%s)" % (S, code) if ty == "real" else "%s((double)(%s))" % (S, code)
        if to == "real":
            if ty == "int":
                return "(double)(%s)" % code
            return "va::val(%s)" % code
        if to == "int":
            return "va::to_int(%s)" % code
        raise VAError("cast %s -> %s" % (ty, to))

    @staticmethod
    def promote(a, b):
        return "dual" if "dual" in (a, b) else ("real" if "real" in (a, b) else "int")

    def _array(self, name, ctx):
        if name not in ctx.vars or name not in self.m.arrays:
            raise VAError("'%s' is not an array variable" % name)
        return self.m.arrays[name]

    def expr(self, e, ctx):
        k = e[0]
        S = ctx.S
        if ctx.hoist is not None:
            hoisted = ctx.hoist.load_static(e, ctx.vars)
            if hoisted is not None:
                return hoisted
        if k == "num":
            if e[2]:
                return str(e[1]), "int"
            v = e[1]
            if v != v:
                return "NAN", "real"
            if v in (float("inf"), float("-inf")):
                return ("INFINITY" if v > 0 else "-INFINITY"), "real"
            return repr(float(v)), "real"
        if k == "id":
            name = e[1]
            if name in ctx.vars:
                cached = ctx.hoist.load_var(name, ctx.vars[name]) if ctx.hoist is not None else None
                return cached if cached is not None else ("v_" + name, ctx.vars[name])
            if name in self.param_ix:
                ty = self.m.params[self.param_ix[name]][1]
                if ty == "string":
                    raise VAError("string parameter '%s' cannot be used in an expression" % name)
                return "p_" + name, ("int" if ty == "integer" else "real")
            raise VAError("undefined identifier '%s' in module %s" % (name, self.m.name))
        if k == "str":
            raise VAError("string in an arithmetic expression")
        if k == "index":
            name = e[1]
            lo, hi = self._array(name, ctx)
            ic, it = self.expr(e[2], ctx)
            return "v_%s[va::clamp_index(%s, %d, %d)]" % (name, self.cast(ic, it, "int", S), lo, hi), ctx.vars[name]
        if k == "un":
            c, t = self.expr(e[2], ctx)
            if e[1] == "-":
                return "(-%s)" % c, t
            if e[1] == "!":
                return "(va::truth(%s) ? 0 : 1)" % c, "int"
            return "(~%s)" % self.cast(c, t, "int", S), "int"
        if k == "bin":
            return self._bin(e, ctx)
        if k == "tern":
            c, _ = self.expr(e[1], ctx)
            a, ta = self.expr(e[2], ctx)
            b, tb = self.expr(e[3], ctx)
            t = self.promote(ta, tb)
            return "(va::truth(%s) ? %s : %s)" % (c, self.cast(a, ta, t, S), self.cast(b, tb, t, S)), t
        if k == "call":
            return self.call(e, ctx)
        raise VAError("cannot generate %r" % (e,))

    def _bin(self, e, ctx):
        op, S = e[1], ctx.S
        a, ta = self.expr(e[2], ctx)
        b, tb = self.expr(e[3], ctx)
        if op in ("+", "-", "*"):
            return "(%s %s %s)" % (a, op, b), self.promote(ta, tb)
        if op == "/":   # always real division (the reference maps `/` to Julia's `/`, src/vasim.jl:221-232)
            t = self.promote(self.promote(ta, tb), "real")
            return "va::v_div(%s, %s)" % (self.cast(a, ta, "real", S) if ta == "int" else a, self.cast(b, tb, "real", S) if tb == "int" else b), t
        if op == "**":
            t = self.promote(self.promote(ta, tb), "real")
            if ta == "dual" and tb != "dual":
                return "va::v_pow(%s, %s)" % (a, b), "dual"
            return "va::v_pow(%s, %s)" % (self.cast(a, ta, t, S), self.cast(b, tb, t, S)), t
        if op == "%":
            if ta == "int" and tb == "int":
                return "(%s %% %s)" % (a, b), "int"
            return "::fmod(%s, %s)" % (self.cast(a, ta, "real", S), self.cast(b, tb, "real", S)), "real"
        if op in ("<", "<=", ">", ">=", "==", "!="):
            av = a if ta == "int" else self.cast(a, ta, "real", S)
            bv = b if tb == "int" else self.cast(b, tb, "real", S)
            return "((%s %s %s) ? 1 : 0)" % (av, op, bv), "int"
        if op in ("&&", "||"):
            return "((va::truth(%s) %s va::truth(%s)) ? 1 : 0)" % (a, op, b), "int"
        return "(%s %s %s)" % (self.cast(a, ta, "int", S), op, self.cast(b, tb, "int", S)), "int"

    def probe(self, acc, nodes, ctx):
        if ctx.infunc:
            raise VAError("branch probes inside analog functions are not supported")
        nodes = self.m.branch_nodes(nodes)
        ty = "real" if ctx.plain else "dual"
        if acc in FLOW_ACCESS:
            vb = self.m.find_vbranch(nodes)
            if vb is None:
                raise VAError("flow probe %s(%s): only the current of a voltage branch can be probed" % (acc, ",".join(nodes)))
            return ("n%d_" if vb[1] > 0 else "(-n%d_)") % self.node_ix[vb[0]], ty
        for n in nodes:
            if n not in self.node_ix:
                raise VAError("unknown node '%s' in module %s" % (n, self.m.name))
        if len(nodes) == 1:
            return "n%d_" % self.node_ix[nodes[0]], ty
        return "(n%d_ - n%d_)" % (self.node_ix[nodes[0]], self.node_ix[nodes[1]]), ty

    def call(self, e, ctx):
        name, args = e[1], e[2]
        if name in POTENTIAL_ACCESS or name in FLOW_ACCESS:
            return self.probe(name, [a[1] for a in args], ctx)
        if name in _CONSTANT_CALLS:
            return _CONSTANT_CALLS[name]
        if name == "$vt":
            if args:
                c, t = self.expr(args[0], ctx)
                return "(%s * %s)" % (c, _VT_PER_KELVIN), self.promote(t, "real")
            return "(env.temperature * %s)" % _VT_PER_KELVIN, "real"
        if name in ("$param_given", "$given"):
            pn = self.m.aliases.get(args[0][1], args[0][1])
            if pn not in self.param_ix:
                raise VAError("$param_given(%s): no such parameter" % pn)
            return "g_" + pn, "int"
        if name == "$simparam":
            if args[0][0] == "str" and args[0][1] == "gmin":
                return "env.gmin", "real"
            if len(args) > 1:
                return self.expr(args[1], ctx)
            raise VAError("$simparam(\"%s\") has no value" % (args[0][1],))
        if name == "$limit":
            return self.expr(args[0], ctx)
        if name == "ddt":
            raise VAError("ddt() is only supported as an additive (possibly scaled) term of a contribution")
        if name == "ddx":
            c, t = self.expr(args[0], ctx)
            if ctx.plain:
                raise VAError("ddx() in a module with noise sources is not supported by the noise pass")
            ix = [self.ddx_nodes.index(a[1]) for a in args[1][2]]
            c = self.cast(c, t, "dual", ctx.S)
            if len(ix) == 1:
                return "va::ddx1(%s, %d)" % (c, ix[0]), "dual"
            return "va::ddx2(%s, %d, %d)" % (c, ix[0], ix[1]), "dual"
        return self._math_call(name, args, ctx)

    def _math_call(self, name, args, ctx):
        S = ctx.S
        base = name[1:] if name.startswith("$") else name
        base = "log10" if base == "log" else base
        if base in _F1 or base == "log10":
            c, t = self.expr(args[0], ctx)
            if base in ("floor", "ceil"):
                return "va::v_%s(%s)" % (base, self.cast(c, t, "real", S) if t == "int" else c), "real"
            if base == "abs" and t == "int":
                return "va::v_abs(%s)" % c, "int"
            t2 = self.promote(t, "real")
            return "va::v_%s(%s)" % (base, self.cast(c, t, t2, S)), t2
        if base in _F2:
            a, ta = self.expr(args[0], ctx)
            b, tb = self.expr(args[1], ctx)
            t = self.promote(ta, tb)
            if base in ("min", "max") and t == "int":
                return "va::v_%s(%s, %s)" % (base, a, b), "int"
            t = self.promote(t, "real")
            if base == "pow" and ta == "dual" and tb != "dual":
                return "va::v_pow(%s, %s)" % (a, b), "dual"
            return "va::v_%s(%s, %s)" % (base, self.cast(a, ta, t, S), self.cast(b, tb, t, S)), t
        if name in self.m.functions:
            return self.user_call(self.m.functions[name], args, ctx)
        raise VAError("unknown function '%s' in module %s" % (name, self.m.name))

    def user_call(self, f, args, ctx):
        if len(args) != len(f.args):
            raise VAError("function %s expects %d arguments, got %d" % (f.name, len(f.args), len(args)))
        S = ctx.S
        ev = [self.expr(a, ctx) if kind != "output" else (None, None) for (nm, kind), a in zip(f.args, args)]
        # outputs whose target variable is dual force the dual instantiation as well
        anydual = any(t == "dual" for c, t in ev if c is not None)
        FS = S if anydual else "double"
        fty = "dual" if anydual else "real"
        call_args, pre, post = [], [], []
        has_out = any(kind != "input" for _, kind in f.args)
        for (nm, kind), a, (c, t) in zip(f.args, args, ev):
            aty = "int" if f.vars.get(nm, "real") == "integer" else fty
            if kind == "input":
                call_args.append(self.cast(c, t, aty, S))
                continue
            if a[0] != "id" or a[1] not in ctx.vars:
                raise VAError("output argument of %s must be a variable" % f.name)
            tn = "o%d_" % next(self.tmp)
            init = " = " + self.cast(c, t, aty, S) if kind == "inout" else ""
            pre.append("%s %s%s;" % ("int" if aty == "int" else FS, tn, init))
            call_args.append(tn)
            post.append("v_%s = %s;" % (a[1], self.cast(tn, aty, ctx.vars[a[1]], S)))
        rty = "int" if f.rtype == "integer" else fty
        callc = "f_%s<%s>(%s)" % (f.name, FS, ", ".join(["env"] + call_args))
        if not has_out:
            return callc, rty
        rt = "int" if rty == "int" else FS
        return "([&]() -> %s { %s %s r_ = %s; %s return r_; }())" % (rt, " ".join(pre), rt, callc, " ".join(post)), rty

    # ---- statements: one method per kind, -> lines ----
    def stmt(self, st, ctx, ind):
        while st[0] == "event":
            st = st[1]
        if st[0] in ("task", "null"):
            return []
        emit = self._STATEMENTS.get(st[0])
        if emit is None:
            raise VAError("cannot generate statement %r" % (st,))
        return emit(self, st, ctx, ind)

    def _assign(self, st, ctx, ind):
        name = st[1]
        if name not in ctx.vars:
            raise VAError("assignment to undeclared variable '%s' in module %s" % (name, self.m.name))
        c, t = self.expr(st[2], ctx)
        return ["%sv_%s = %s;" % ("  " * ind, name, self.cast(c, t, ctx.vars[name], ctx.S))]

    def _assign_idx(self, st, ctx, ind):
        name = st[1]
        lo, hi = self._array(name, ctx)
        ic, it = self.expr(st[2], ctx)
        c, t = self.expr(st[3], ctx)
        return ["%sv_%s[va::clamp_index(%s, %d, %d)] = %s;" % ("  " * ind, name, self.cast(ic, it, "int", ctx.S), lo, hi, self.cast(c, t, ctx.vars[name], ctx.S))]

    def _contrib(self, st, ctx, ind):
        if ctx.infunc:
            raise VAError("contribution inside an analog function")
        acc, nodes, rhs, pad = st[1], self.m.branch_nodes(st[2]), st[3], "  " * ind
        if acc in POTENTIAL_ACCESS:
            if _is_zero(rhs):
                # V(a,b) <+ 0: node collapse, resolved structurally on the host (the two nodes are merged before
                # the circuit reaches the engine)
                return ["%s/* V(%s) <+ 0: node collapse handled at circuit build */" % (pad, ",".join(nodes))]
            return self._branch_contrib(nodes, 1, rhs, ctx, pad) if ctx.contrib == "stamp" else []
        if acc not in FLOW_ACCESS:
            raise VAError("unknown access function %s" % acc)
        if ctx.contrib == "noise" and is_noise_source(rhs):
            return self._noise_record(nodes, rhs, ctx, pad)
        if ctx.contrib != "stamp" or is_noise_source(rhs):
            return []
        if self.m.find_vbranch(nodes) is not None:   # current contribution to a voltage / switch branch
            return self._branch_contrib(nodes, 0, rhs, ctx, pad)
        return self._flow_contrib(nodes, rhs, ctx, pad)

    def _noise_record(self, nodes, rhs, ctx, pad):
        """`I(a,b) <+ white_noise(pwr, name)` / `flicker_noise(pwr, exp, name)` become records
        (src/va_env.jl:92-101: the power is an observable, the source an epsilon of the linearisation)"""
        nargs = [x for x in rhs[2] if x[0] != "str"]
        pc, pt = self.expr(nargs[0], ctx)
        ec, et = (self.expr(nargs[1], ctx) if rhs[1] == "flicker_noise" else ("0.0", "real"))
        a = self.node_ix[nodes[0]]
        b = self.node_ix[nodes[1]] if len(nodes) > 1 else -1
        return ["%sif (n_ < va::MAX_NOISE) { out[n_].a = %d; out[n_].b = %d; out[n_].pwr = %s; out[n_].ex = %s; ++n_; }" %
                (pad, a, b, self.cast(pc, pt, "real", ctx.S), self.cast(ec, et, "real", ctx.S))]

    def _flow_contrib(self, nodes, rhs, ctx, pad):
        """`I(a,b) <+ f + ddt(q)`: f into the node sums of I, q into those of Q.  The sums are kept in locals (i0_, q0_, ...) and
        stored once at the end: the caller's I[] / Q[] live in scratch (the function is not inlined), a read-modify-write
        there per contribution"""
        a = self.node_ix[nodes[0]]
        b = self.node_ix[nodes[1]] if len(nodes) > 1 else None
        out = []
        for part, c in self._parts(rhs, ctx):
            acc = ("i", "q")[part]
            out.append("%sif (PART != %d) { const %s c_ = %s; %s%d_ += c_;%s }" % (pad, 1 - part, ctx.S, c, acc, a, (" %s%d_ -= c_;" % (acc, b)) if b is not None else ""))
        return out

    def _branch_contrib(self, nodes, kind, rhs, ctx, pad):
        """Contribution to a voltage / switch branch: state (0 CURRENT, 1 VOLTAGE) and value as in src/vasim.jl:128-180."""
        S = ctx.S
        name, sgn = self.m.find_vbranch(nodes)
        k = [self.m.branch_node(key) for key in self.m.vbranches].index(name)
        return ["%sif (bs%d_ != %d) { bs%d_ = %d; bv%d_ = %s(0.0); bq%d_ = %s(0.0); }" % (pad, k, kind, k, kind, k, S, k, S)] + \
            ["%sif (PART != %d) %s%d_ %s %s;" % (pad, 1 - part, ("bv", "bq")[part], k, "+=" if sgn > 0 else "-=", c) for part, c in self._parts(rhs, ctx)]

    def _parts(self, rhs, ctx):
        """(part, value as a dual) for the parts of a contribution that are there: 0 resistive, 1 under ddt()"""
        for part, ast in enumerate(self.split_ddt(rhs)):
            if ast is not None:
                c, t = self.expr(ast, ctx)
                yield part, self.cast(c, t, "dual", ctx.S)

    def split_ddt(self, e):
        """(resistive AST or None, reactive AST or None)"""
        k = e[0]
        if k == "call" and e[1] == "ddt":
            return None, e[2][0]
        if not _has_ddt(e):
            return e, None
        if k == "bin" and e[1] in ("+", "-"):
            ar, aq = self.split_ddt(e[2])
            br, bq = self.split_ddt(e[3])

            def comb(x, y):
                if x is None and y is None:
                    return None
                if y is None:
                    return x
                if x is None:
                    return y if e[1] == "+" else ("un", "-", y)
                return ("bin", e[1], x, y)
            return comb(ar, br), comb(aq, bq)
        if k == "un" and e[1] == "-":
            r, q = self.split_ddt(e[2])
            return (None if r is None else ("un", "-", r)), (None if q is None else ("un", "-", q))
        if k == "bin" and e[1] == "*":
            for x, y, left in ((e[2], e[3], True), (e[3], e[2], False)):
                if _has_ddt(x) and not _has_ddt(y):
                    r, q = self.split_ddt(x)

                    def mul(z):
                        return None if z is None else (("bin", "*", z, y) if left else ("bin", "*", y, z))
                    return mul(r), mul(q)
        if k == "bin" and e[1] == "/" and _has_ddt(e[2]) and not _has_ddt(e[3]):
            r, q = self.split_ddt(e[2])
            return (None if r is None else ("bin", "/", r, e[3])), (None if q is None else ("bin", "/", q, e[3]))
        if k == "tern":
            ar, aq = self.split_ddt(e[2])
            br, bq = self.split_ddt(e[3])
            zero = ("num", 0.0, False)
            r = None if ar is None and br is None else ("tern", e[1], ar or zero, br or zero)
            q = None if aq is None and bq is None else ("tern", e[1], aq or zero, bq or zero)
            return r, q
        raise VAError("ddt() must appear as an additive (possibly scaled) term of a contribution")

    def _if(self, st, ctx, ind):
        pad = "  " * ind
        c, _ = self.expr(st[1], ctx)
        out = ["%sif (va::truth(%s)) {" % (pad, c)] + self.stmt(st[2], ctx, ind + 1)
        if st[3] is not None:
            out += ["%s} else {" % pad] + self.stmt(st[3], ctx, ind + 1)
        return out + ["%s}" % pad]

    def _block(self, st, ctx, ind):
        pad = "  " * ind
        out = ["%s{" % pad]
        if st[2]:
            types = self.local_types(st[2], ctx)
            ctx = replace(ctx, vars=dict(ctx.vars, **types), hoist=ctx.hoist and ctx.hoist.shadowed(types))
            out += [self.decl(nm, t, ctx.S, pad + "  ") for nm, t in types.items()]
        for s in st[3]:
            out += self.stmt(s, ctx, ind + 1)
        return out + ["%s}" % pad]

    def _case(self, st, ctx, ind):
        pad, S = "  " * ind, ctx.S
        c, t = self.expr(st[1], ctx)
        sv = "sw%d_" % next(self.tmp)
        out = ["%s{ const double %s = %s;" % (pad, sv, self.cast(c, t, "real", S) if t != "real" else c)]
        first, default = True, None
        for conds, body in st[2]:
            if conds is None:
                default = body
                continue
            tests = []
            for cd in conds:
                cc, ct = self.expr(cd, ctx)
                tests.append("%s == %s" % (sv, self.cast(cc, ct, "real", S) if ct != "real" else cc))
            out.append("%s%sif (%s) {" % (pad, "" if first else "} else ", " || ".join(tests)))
            out += self.stmt(body, ctx, ind + 1)
            first = False
        if default is not None:
            out.append("%s%s{" % (pad, "" if first else "} else "))
            out += self.stmt(default, ctx, ind + 1)
            first = False
        if not first:
            out.append("%s}" % pad)
        return out + ["%s}" % pad]

    def _for(self, st, ctx, ind):
        pad = "  " * ind
        init = self.stmt(st[1], ctx, 0)[0]
        c, _ = self.expr(st[2], ctx)
        upd = self.stmt(st[3], ctx, 0)[0].rstrip(";")
        return ["%sfor (%s va::truth(%s); %s) {" % (pad, init, c, upd)] + self.stmt(st[4], ctx, ind + 1) + ["%s}" % pad]

    def _while(self, st, ctx, ind):
        pad = "  " * ind
        c, _ = self.expr(st[1], ctx)
        return ["%swhile (va::truth(%s)) {" % (pad, c)] + self.stmt(st[2], ctx, ind + 1) + ["%s}" % pad]

    def _repeat(self, st, ctx, ind):
        pad = "  " * ind
        c, t = self.expr(st[1], ctx)
        k = next(self.tmp)
        return ["%sfor (int r%d_ = 0, n%d_ = %s; r%d_ < n%d_; ++r%d_) {" % (pad, k, k, self.cast(c, t, "int", ctx.S), k, k, k)] + \
            self.stmt(st[2], ctx, ind + 1) + ["%s}" % pad]

    _STATEMENTS = {"assign": _assign, "assign_idx": _assign_idx, "contrib": _contrib, "if": _if, "block": _block, "case": _case, "for": _for,
                   "while": _while, "repeat": _repeat}
