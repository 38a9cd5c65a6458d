"""Verilog-A → C++ (HIP device + host) code generator — the MI355X counterpart of `make_spice_device`
(src/vasim.jl:649-867), which turns a parsed module into a Julia device functor.

For every module one function template is emitted:

    template <class R> void eval_<module>(const double* P, const R* V, const va::Env& env, R* I, R* Q)

P  : parameter values in declaration order followed by the same number of "given" flags
V  : node voltages (ports then internal nets), seeded as dual numbers by the dispatcher
I/Q: per-node sums of the resistive currents / the charges under ddt() leaving the node through the device
     (`I(a,b) <+ f + ddt(q)` adds f to I[a], −f to I[b], q to Q[a], −q to Q[b])

plus a registry (names of modules, nodes, parameters) and `va_gen::stamp(module, …)`, which seeds the
duals, runs the module and scatters values and derivatives into the engine's wide stamp record
[I(8) | Q(8) | G(8×8) | C(8×8)].  The same header is compiled into libcedarhip.so (device) and into the
test oracle (host), so a model added to the VA library is available to both after a rebuild.

Typing: VA `integer` → int, VA `real` → double unless a fixed-point pass finds that the variable can
depend on a node voltage, in which case it is the dual type R.  Analog functions are templates over one
scalar type S, instantiated with R when any argument is dual.

This file assembles: the functions of one module (`generate_module`) and the header around all of them
(`generate_header`).  Expressions and statements are written by codegen_emit.py, the setup / eval split by codegen_split.py.
"""
from dataclasses import dataclass

from .codegen_emit import Emitter, Pass, is_noise_source, walk
from .codegen_split import Split


@dataclass
class ModuleCode:
    """What generating one module yields: its namespace, and what the registry and the dispatchers say about it."""
    module: object
    lines: list
    n_cache: int      # doubles in the constant block C that setup() fills
    op_names: list    # the (* desc *) observables, in the order opvars() stores them
    has_noise: bool
    q_mask: int
    ddx_nodes: list


def _param_decls(m):
    """`p_<name>` / `g_<name>` locals for the parameters (and $param_given flags) the analog block reads"""
    used = set()
    for n in walk([m.analog]):
        if n and n[0] == "id":
            used.add(n[1])
        if n and n[0] == "call" and n[1] in ("$param_given", "$given"):
            used.add("?" + m.aliases.get(n[2][0][1], n[2][0][1]))
    out = []
    for i, (nm, ty, _, _) in enumerate(m.params):
        if ty == "string":
            continue
        if nm in used:
            out.append("  const %s p_%s = %sP[%d];" % ("int" if ty == "integer" else "double", nm, "(int)" if ty == "integer" else "", i))
        if "?" + nm in used:
            out.append("  const int g_%s = P[%d] != 0.0 ? 1 : 0;" % (nm, len(m.params) + i))
    return out


def _function(g, f):
    targs = []
    for nm, kind in f.args:
        ty = "int" if f.vars.get(nm) == "integer" else "S"
        targs.append("%s%s v_%s" % (ty, "&" if kind != "input" else "", nm))
    rt = "int" if f.rtype == "integer" else "S"
    out = ["template <class S> VA_HD %s f_%s(%s) {" % (rt, f.name, ", ".join(["const va::Env& env"] + targs))]
    argn = {nm for nm, _ in f.args}
    vars_ = {nm: "int" if ty == "integer" else "dual" for nm, ty in f.vars.items()}
    out += [g.decl(nm, t, "S") for nm, t in vars_.items() if nm not in argn]
    out.append("  (void)env;")
    out += g.stmt(f.body, Pass("S", vars_, infunc=True), 1)
    return out + ["  return v_%s;" % f.name, "}"]


def generate_module(m):
    g = Emitter(m)
    vars_ = g.module_var_types()
    param_decls = _param_decls(m)
    nodes = range(len(m.nodes))

    def preamble(signature, scalar, unused, first=()):
        """what every function over the analog block starts with"""
        return [signature + " {", "  VA_KEEP_RETURN_ADDRESS;", *first] + param_decls + [g.decl(nm, t, scalar) for nm, t in vars_.items()] + \
            ["  " + " ".join("(void)%s;" % u for u in unused)]

    def plain_walk(signature, contrib, first=()):
        """the analog block over plain doubles, with the contributions replaced by `contrib`"""
        out = preamble(signature, "double", ("env", "V", "P"), first)
        out += ["  const double n%d_ = V[%d]; (void)n%d_;" % (k, k, k) for k in nodes]
        ctx = Pass("double", {k: ("real" if t == "dual" else t) for k, t in vars_.items()}, plain=True, contrib=contrib)
        for st in m.analog:
            out += g.stmt(st, ctx, 1)
        return out

    out = ["// ---- module %s: %d ports, %d internal nodes, %d parameters ----" % (m.name, len(m.ports), len(m.internal), len(m.params)),
           "namespace m_%s {" % m.name]
    for f in m.functions.values():
        out += _function(g, f)
    # setup(P, env, C): the bias-independent statements; eval(P, C, V, ...): the rest (see codegen_split.py)
    S, E, n_cache = Split(g, vars_).run()
    out += preamble("VA_HD_NOINLINE void setup(const double* P, const va::Env& env, double* C)", "double", ("env", "P", "C")) + S + ["}"]
    # PART: -1 everything; 0 the resistive sums I[] only; 1 the charge sums Q[] only — two half-evaluations on two wavefronts
    # (the engine's function split of a compiled device: what a half does not store, the compiler drops)
    # CP: the pointer type of the parameter and constant blocks — `const double*`, or va::lds_cptr when the caller has staged them
    # into LDS (then every P[i] / C[i] is a ds_read that waits on the LDS counter alone instead of a flat load behind every scratch store)
    out += preamble("template <class R, int PART, class CP = const double*> VA_HD_NOINLINE void eval(CP P, CP C, const R* V, const va::Env& env, R* I, R* Q)",
                    "R", ("env", "V", "P", "C"))
    # node voltages read once, node sums accumulated in registers
    out += ["  const R n%d_ = V[%d]; R i%d_ = R(0.0), q%d_ = R(0.0); (void)n%d_;" % (k, k, k, k, k) for k in nodes]
    out += ["  int bs%d_ = 0; R bv%d_ = R(0.0), bq%d_ = R(0.0);" % (k, k, k) for k in range(len(m.vbranches))]
    out += E
    for k, key in enumerate(m.vbranches):
        kb, a = g.node_ix[m.branch_node(key)], g.node_ix[key[0]]
        vab = "n%d_" % a if len(key) == 1 else "(n%d_ - n%d_)" % (a, g.node_ix[key[1]])
        out.append("  i%d_ += n%d_;%s" % (a, kb, (" i%d_ -= n%d_;" % (g.node_ix[key[1]], kb)) if len(key) > 1 else ""))
        out.append("  i%d_ += (bs%d_ == 1 ? %s : n%d_) - bv%d_; q%d_ -= bq%d_;" % (kb, k, vab, kb, k, kb, k))
    for k in nodes:
        out += ["  if (PART != 1) I[%d] = i%d_;" % (k, k), "  if (PART != 0) Q[%d] = q%d_;" % (k, k)]
    out.append("}")
    # noise pass: contributions replaced by noise records
    has_noise = any(n and is_noise_source(n) for n in walk(m.analog))
    if has_noise:
        out += plain_walk("VA_HD_NOINLINE int noise(const double* P, const double* V, const va::Env& env, va::NoiseRec* out)", "noise", ["  int n_ = 0;"])
        out += ["  return n_;", "}"]
    # operating-point pass: the variables declared with a (* desc *) attribute are the module's observables
    # (src/vasim.jl:742-753, 841-843)
    op_names = [nm for nm in m.var_desc if vars_.get(nm) in ("real", "dual", "int")]
    if op_names:
        out += plain_walk("VA_HD_NOINLINE void opvars(const double* P, const double* V, const va::Env& env, double* op)", "none")
        out += ["  op[%d] = (double)v_%s;" % (k, nm) for k, nm in enumerate(op_names)] + ["}"]
    out.append("}  // namespace m_%s" % m.name)
    return ModuleCode(m, out, n_cache, op_names, has_noise, g.q_mask(), g.ddx_nodes)


# ---- the header around the modules ----
_SCATTER = """
// Seeds the duals, evaluates module `mod` and scatters into the wide stamp record
// st = [I(8) | Q(8) | G(8x8) | C(8x8)], every entry scaled by the multiplicity m.
template <int NT, class R> VA_HD void scatter(const R* I, const R* Q, double m, double* st) {
  for (int k = 0; k < NT; ++k) {
    st[k] = m * va::val(I[k]); st[8 + k] = m * va::val(Q[k]);
    for (int j = 0; j < NT; ++j) { st[16 + k * 8 + j] = m * va::val(I[k].d[j]); st[80 + k * 8 + j] = m * va::val(Q[k].d[j]); }
  }
}"""
_BLOCK_SIZES = """\
// doubles of module `mod`'s parameter block [values | given flags] and of its constant block (device-side sizes: a kernel
// that stages the blocks of its instances into LDS)"""
_STAMP = """\
// the same without a stored constant block (host-side callers, one-off evaluations): setup into a local block first
VA_HD_NOINLINE void stamp(int mod, const double* P, const double* v, const va::Env& env, double m, double* st) {
  double C[MAX_CACHE];
  setup(mod, P, env, C);
  stamp_c(mod, P, C, v, env, m, st);
}

// Direction-parallel evaluation: one lane per (device, node j) computes the values and the j-th column of the
// Jacobians with one-directional duals (VD<1,·>); the lane flagged `first` also writes I and Q.
// part: -1 the whole record; 0 the resistive half (I, dI/dV); 1 the charge half (Q, dQ/dV) — the two halves of a device may run
// on different wavefronts."""
_STAMP_DIR_LDS = """
// stamp_dir_c with the parameter and constant blocks in LDS (tran_persistent_kernel stages them once per transient): the large
// models get an instantiation that reads them with LDS instructions, every other module goes through the generic pointers"""
_DIR_STORE = """\
        if (part != 1) { if (first) st[k] = m * va::val(I[k]); st[16 + k * 8 + dir] = m * va::val(I[k].d[0]); }
        if (part != 0) { if (first) st[8 + k] = m * va::val(Q[k]); st[80 + k * 8 + dir] = m * va::val(Q[k].d[0]); }"""


def _is_large(m):
    """A large model: the engine splits it into a resistive and a charge half (ch_engine.hip, slot bits 29/30) and stages its
    parameter and constant blocks into LDS."""
    return len(m.params) >= 64


def _dispatch(signature, cases, default):
    """`signature { switch (mod) { case <id>: <text> ... default: <default> } }`; cases: [(module id, text after "case N: ")]"""
    return [signature + " {", "  switch (mod) {"] + ["    case %d: %s" % c for c in cases] + ["    default: " + default, "  }", "}"]


def _stamp_case(c, n_dir, seed, evals, store):
    """case body of the stamp dispatchers: seed the node voltages as duals with n_dir directions, evaluate, store"""
    nt, nd = len(c.module.nodes), len(c.ddx_nodes)
    R = "va::VD<%d, double>" % n_dir if nd == 0 else "va::VD<%d, va::VD<%d, double>>" % (n_dir, nd)
    out = ["{", "      typedef %s R;" % R, "      R V[%d], I[%d], Q[%d];" % (nt, nt, nt)]
    for k, node in enumerate(c.module.nodes):
        out.append("      V[%d] = va::%s, %d, (R*)nullptr);" % (k, seed % (k, k), c.ddx_nodes.index(node) if node in c.ddx_nodes else -1))
    return "\n".join(out + ["      " + e for e in evals] + store + ["    } break;"])


def _stamp_dir_case(c, cp, split):
    """one lane's direction of module c; cp: pointer type of P and C ("" the plain one); split: evaluate as two halves"""
    name = c.module.name
    if split:
        # the whole record (CEDARHIP_VA_NOSPLIT, a diagnostic) is the two halves in sequence — no third instantiation of a
        # 57 k-instruction function
        evals = ["if (part != %d) m_%s::eval<R, %d%s>(P, C, V, env, I, Q);" % (1 - part, name, part, cp) for part in (0, 1)]
    else:
        # a small model is never split: ONE evaluation (two half instantiations would run the shared front end twice)
        evals = ["m_%s::eval<R, -1>(P, C, V, env, I, Q);" % name]
    return _stamp_case(c, 1, "seed1(v[%d], dir == %d", evals,
                       ["      for (int k = 0; k < %d; ++k) {" % len(c.module.nodes), _DIR_STORE, "      }"])


def generate_header(modules, source_tag=""):
    """C++ header text for a list of parsed modules (module id = position in the list)."""
    code = [generate_module(m) for m in modules]
    ids = list(enumerate(code))

    def strings(xs):
        return ", ".join('"%s"' % x for x in xs) or '""'
    out = ["// GENERATED by cedarsim.jl_amd/va/codegen.py — do not edit.  %s" % source_tag,
           "#pragma once", '#include "../va_rt.hpp"', "", "namespace va_gen {", ""]
    for c in code:
        out += c.lines + [""]
    # registry
    out.append("struct ModuleInfo { const char* name; int n_ports, n_nodes, n_params; unsigned q_mask; const char* const* node_names; const char* const* param_names; };")
    for c in code:
        out.append("static const char* const nodes_%s[] = {%s};" % (c.module.name, strings(c.module.nodes)))
        out.append("static const char* const params_%s[] = {%s};" % (c.module.name, strings(p[0] for p in c.module.params)))
    out += ["static const char* const opnames_%s[] = {%s};" % (c.module.name, strings(c.op_names)) for c in code]
    out.append("static const int N_OPVARS[] = {%s};" % (", ".join(str(len(c.op_names)) for c in code) or "0"))
    out.append("static const char* const* const OPNAMES[] = {%s};" % (", ".join("opnames_%s" % c.module.name for c in code) or "nullptr"))
    out.append("static const int N_MODULES = %d;" % len(code))
    out.append("static const ModuleInfo MODULES[] = {")
    for c in code:
        m = c.module
        out.append('  {"%s", %d, %d, %d, %du, nodes_%s, params_%s},' % (m.name, len(m.ports), len(m.nodes), len(m.params), c.q_mask, m.name, m.name))
    if not code:
        out.append('  {"", 0, 0, 0, 0u, nullptr, nullptr},')
    out += ["};", _SCATTER]
    out.append("static const int N_CACHE[] = {%s};" % (", ".join(str(c.n_cache) for c in code) or "0"))
    out.append("constexpr int MAX_CACHE = %d;" % max([1] + [c.n_cache for c in code]))
    # dispatchers on the module id
    out.append(_BLOCK_SIZES)
    out += _dispatch("VA_HD int param_doubles(int mod)", [(i, "return %d;" % (2 * len(c.module.params))) for i, c in ids], "return 0;")
    out += _dispatch("VA_HD int cache_doubles(int mod)", [(i, "return %d;" % c.n_cache) for i, c in ids], "return 0;")
    out.append("// Per-instance constants of module `mod`: C[0 .. N_CACHE[mod]) from the parameter block and the temperature")
    out += _dispatch("VA_HD_NOINLINE void setup(int mod, const double* P, const va::Env& env, double* C)",
                     [(i, "m_%s::setup(P, env, C); break;" % c.module.name) for i, c in ids], "break;")
    out += _dispatch("VA_HD_NOINLINE void stamp_c(int mod, const double* P, const double* C, const double* v, const va::Env& env, double m, double* st)",
                     [(i, _stamp_case(c, len(c.module.nodes), "seed(v[%d], %d", ["m_%s::eval<R, -1>(P, C, V, env, I, Q);" % c.module.name],
                                      ["      scatter<%d, R>(I, Q, m, st);" % len(c.module.nodes)])) for i, c in ids], "break;")
    out.append(_STAMP)
    out += _dispatch("VA_HD_NOINLINE void stamp_dir_c(int mod, const double* P, const double* C, const double* v, const va::Env& env, double m, int dir, bool first, int part, double* st)",
                     [(i, _stamp_dir_case(c, "", _is_large(c.module))) for i, c in ids], "break;")
    out.append(_STAMP_DIR_LDS)
    out += _dispatch("VA_HD_NOINLINE void stamp_dir_lds(int mod, va::lds_cptr P, va::lds_cptr C, const double* v, const va::Env& env, double m, int dir, bool first, int part, double* st)",
                     [(i, _stamp_dir_case(c, ", va::lds_cptr", True)) for i, c in ids if _is_large(c.module)],
                     "stamp_dir_c(mod, (const double*)P, (const double*)C, v, env, m, dir, first, part, st); break;")
    out += ["", "// operating-point variables (the (* desc *) observables) of module `mod` at node voltages v"]
    out += _dispatch("VA_HD_NOINLINE void opvars(int mod, const double* P, const double* v, const va::Env& env, double* op)",
                     [(i, "m_%s::opvars(P, v, env, op); break;" % c.module.name) for i, c in ids if c.op_names], "break;")
    out += ["", "// noise sources of module `mod` at node voltages v: records (node a, node b or -1, power, flicker exponent)"]
    out += _dispatch("VA_HD_NOINLINE int noise(int mod, const double* P, const double* v, const va::Env& env, va::NoiseRec* out)",
                     [(i, "return m_%s::noise(P, v, env, out);" % c.module.name) for i, c in ids if c.has_noise], "return 0;")
    out += ["", "}  // namespace va_gen"]
    return "\n".join(out) + "\n"
