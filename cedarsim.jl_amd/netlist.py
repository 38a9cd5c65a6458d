"""SPICE-subset netlist → flat `Circuit`.

Covers exactly what the benchmark and test decks of the reference use: `R C L V I B E G M X` lines,
`DC / PWL / PULSE / SIN` sources, `.subckt/.ends` with parameters, `.param`, `.model` (BSIM4 level
14/54, with `name.N` binning), `.include`, `.lib` (sections), `.option`, `.temp`, `.tran`, `.if/.elseif/
.else/.endif`, quoted expressions, SPICE magnitudes.  Semantics follow the reference front-end:

  * magnitudes t g meg k m u mil n p f a, case-insensitive, matched at the END of the token
    (src/spectre.jl:402-415, :441-456) and multiplied in decimal so `0.22u == 0.22e-6` exactly
    (Dec64 there, `decimal.Decimal` here; test/basic.jl:626-637)
  * model binning: bins named `name.N`; bin chosen by `lmin <= scale*l < lmax && wmin <= scale*w < wmax`
    (src/spectre.jl:677, :718-722, :1162-1176); no bin → NoBinException
  * level 14/54 → BSIM4; `nmos`/`pmos` → TYPE=±1 (src/spectre.jl:589-643)
  * `m=` multiplies down the hierarchy (src/spectre.jl:942-952, src/simulate_ir.jl:43-48)
  * `.option temp/gmin/scale` and `.temp` feed SimSpec unless overridden (src/spectre.jl:1529-1544)
  * unsupported statements are ignored with a warning (src/spectre.jl:1391-1393)

What lives where:
  * spice_expr.py: numbers and expressions (`parse_number`, `eval_expr`, both re-exported here).  Its docstring has the grammar
    and the two places where it is not what the earlier translation to Python source accepted: nested ternaries evaluate, and
    comparison chains and `//` are errors.
  * here, reading: the lexical layer, then `_Reader` (one per `parse_spice` call: subcircuit stack, include directories and
    resolver, one method per directive) fills a `ParsedNetlist` with the statement records `Params / If / ElseIf / Else / EndIf /
    Device`.  Expressions stay text until a build asks for their value, so a branch that is not taken may hold anything.
  * here, flattening: `ParsedNetlist.build` hands one `_Flattener` (circuit, overrides, used overrides, model indices, one method
    per element letter) the statements; nothing of a build is kept on the netlist, so builds of one netlist do not meet.
    After a taken `.if` or `.elseif` no later branch of that level is taken and no later condition evaluated.
"""
import os
import re
import warnings
from collections import namedtuple

from .circuit import DC, PULSE, PWL, SIN, CedarError, Circuit
from .spice_expr import eval_expr, parse_number  # noqa: F401  (both are part of this module's surface)
from .va.build import HERE as _VA_DIR
from .va.frontend import parse_va_file
from .va.registry import has_module


class NoBinException(CedarError):
    pass


# ---- lexical layer --------------------------------------------------------------------------------
def _logical_lines(text):
    """Join '+' continuations, drop comments; keeps the first line (title) out."""
    lines = []
    for raw in text.splitlines():
        line = raw.rstrip()
        if not line.strip():
            continue
        st = line.lstrip()
        if st.startswith("*"):
            continue
        # inline comments
        for c in (" $", "\t$", ";"):
            i = line.find(c)
            if i >= 0:
                line = line[:i]
        if st.startswith("+"):
            if lines:
                lines[-1] += " " + st[1:]
            continue
        lines.append(line.strip())
    return lines


def _tokenize(line):
    """Split a logical line into tokens; quoted expressions, {...} and (...) groups survive;
    `a = b` becomes `a=b`."""
    line = re.sub(r"\s*=\s*", "=", line)
    toks, cur, depth, quote = [], "", 0, None
    for ch in line:
        if quote:
            cur += ch
            if ch == quote:
                quote = None
            continue
        if ch == "'":
            quote = "'"
            cur += ch
        elif ch in "({":
            depth += 1
            cur += ch
        elif ch in ")}":
            depth -= 1
            cur += ch
        elif ch in " \t," and depth == 0:
            if cur:
                toks.append(cur)
                cur = ""
        else:
            cur += ch
    if cur:
        toks.append(cur)
    return toks


def _split_params(tokens):
    """Separate positional tokens from key=value tokens."""
    pos, kw = [], {}
    for t in tokens:
        if "=" in t and not t.startswith("'"):
            k, v = t.split("=", 1)
            kw[k.lower()] = v
        else:
            pos.append(t)
    return pos, kw


class Subckt:
    def __init__(self, name, ports, params):
        self.name, self.ports, self.params = name, ports, params  # params: ordered dict name → expr text
        self.body = []   # statement records, in deck order


Params = namedtuple("Params", "exprs")      # .param: ordered dict name → expression text
If = namedtuple("If", "cond")               # .if (cond): the expression text
ElseIf = namedtuple("ElseIf", "cond")
Else = namedtuple("Else", "")
EndIf = namedtuple("EndIf", "")
Device = namedtuple("Device", "name tokens")   # element line: lower-case name, the tokens after it


class ParsedNetlist:
    """Result of `parse_spice`: statements + models; `build(**overrides)` flattens to a `Circuit`.

    Parameter overrides use the reference's dotted naming: `R1=...` for a top-level `.param`,
    `var"x1.r_load"` ≙ `"x1.r_load"` for a parameter inside instance x1 (test/sweep.jl:342-371).
    """

    def __init__(self):
        self.title = ""
        self.top = Subckt("<top>", [], {})
        self.subckts = {}
        self.models = {}        # base name → list of (full name, type, params dict)
        self.options = {}
        self.tran = None        # (tstep, tstop)
        self.warnings = []

    def add_spectre_models(self, text):
        """Register the `model` cards of a Spectre-language file (e.g. the ASAP7 `7nm_TT.scs` the reference's parser
        tests hold) so that SPICE instance lines can name them."""
        for name, (master, params) in parse_spectre_models(text).items():
            self.models.setdefault(name, []).append((name, master, params))

    def add_model_cards(self, cards):
        """Register model cards given as {name: {"master": module-or-type, "params": {param: value}}}."""
        for name, card in cards.items():
            self.models.setdefault(name.lower(), []).append((name.lower(), card["master"].lower(), dict(card["params"])))

    # -- SimSpec --
    def _spec(self, overrides):
        spec = {"temp": 27.0, "gmin": 1e-12, "scale": 1.0}
        for k in spec:
            if k in self.options:
                spec[k] = eval_expr(self.options[k], {})
        return tuple(overrides.pop(k, v) for k, v in spec.items())

    def find_bin(self, base, l, w, scale=1.0):
        """find_bin (src/spectre.jl:1162-1176): half-open ranges on scale*l, scale*w."""
        bins = self.models[base]
        if len(bins) == 1 and "." not in bins[0][0]:
            return bins[0]
        L, W = scale * l, scale * w
        for b in bins:
            p = b[2]
            if p.get("lmin", 0.0) <= L < p.get("lmax", 1.0) and p.get("wmin", 0.0) <= W < p.get("wmax", 1.0):
                return b
        raise NoBinException("NoBinException: no bin for BinnedModel %s of size (l=%s, w=%s)." % (base, L, W))

    def build(self, **overrides):
        ov = {k.lower(): float(v) for k, v in overrides.items()}
        temp, gmin, scale = self._spec(ov)
        ckt = Circuit(temp=temp, gmin=gmin, scale=scale)
        ckt.title = self.title
        ckt._netlist = self
        return _Flattener(self, ckt, ov).run()

    # level → compiled Verilog-A module (src/spectre.jl:589-630: 17/72 → bsimcmg107); TYPE/DEVTYPE from nmos/pmos (:632-643)
    _VA_LEVELS = {17: "bsimcmg", 72: "bsimcmg"}
    _VA_TYPE_PARAM = {"bsimcmg": ("devtype", {"nmos": 1, "pmos": 0})}

    def _va_model(self, name):
        """(module name, card parameters) when `name` is a compiled Verilog-A module or a `.model` card of one."""
        base = str(name).lower()
        if base in self.models:
            full, mtype, params = self.models[base][0]
            mod = None
            if has_module(mtype):
                mod = mtype
            elif mtype in ("bsimcmg107", "bsimcmg_va", "bsimcmg") and has_module("bsimcmg"):
                mod = "bsimcmg"
            elif mtype in ("nmos", "pmos") and int(params.get("level", 0)) in self._VA_LEVELS and has_module(self._VA_LEVELS[int(params["level"])]):
                mod = self._VA_LEVELS[int(params["level"])]
            if mod is None:
                return None
            card = {k: v for k, v in params.items() if k not in ("level", "version") or mod != "bsimcmg"}
            card.pop("level", None)
            if mod in self._VA_TYPE_PARAM:   # TYPE/DEVTYPE from nmos|pmos or type=n|p (src/spectre.jl:632-643)
                pn, mp = self._VA_TYPE_PARAM[mod]
                ty = card.pop("type", None)
                if mtype in ("nmos", "pmos"):
                    card.setdefault(pn, mp[mtype])
                elif ty in ("n", "p"):
                    card.setdefault(pn, mp["nmos" if ty == "n" else "pmos"])
            return mod, card
        if base not in self.subckts and has_module(base):
            return base, {}
        return None


_Scope = namedtuple("_Scope", "prefix node_map env mult")   # one subcircuit instance while it is expanded
_Line = namedtuple("_Line", "letter full pos kw m m_given")   # one element line in its scope: full name, multiplier applied


def _selected(body, val):
    """The statements of `body` that its `.if / .elseif / .else / .endif` select.  One (enclosing branch live, a branch of this
    level already taken) per open `.if`; a condition is evaluated only where its value decides something."""
    levels, live = [], True
    for st in body:
        kind = type(st)
        if kind is If:
            levels.append((live, live and bool(val(st.cond))))
            live = levels[-1][1]
        elif kind is ElseIf or kind is Else:
            outer, taken = levels[-1]
            live = outer and not taken and (kind is Else or bool(val(st.cond)))
            levels[-1] = (outer, taken or live)
        elif kind is EndIf:
            live = levels.pop()[0]
        elif live:
            yield st


class _Flattener:
    """One `ParsedNetlist.build`: the circuit being filled, the overrides and which of them were used, and the index of every
    model card already added to the circuit."""

    def __init__(self, nl, ckt, ov):
        self.nl, self.ckt, self.ov = nl, ckt, ov
        self.used_ov, self.model_ix = set(), {}

    def run(self):
        self.expand(self.nl.top, _Scope("", {}, {}, 1.0), {})
        unused = set(self.ov) - self.used_ov
        if unused:
            raise CedarError("unknown parameter(s) in override: %s" % ", ".join(sorted(unused)))
        return self.ckt

    def override(self, env, prefix, k):
        if prefix + k in self.ov:
            env[k] = self.ov[prefix + k]
            self.used_ov.add(prefix + k)
            return True
        return False

    def environment(self, sub, outer, inst_params):
        """Parameters of one instance of `sub`: the defaults declared on the .subckt line, then the instance's own, then the
        `.param` statements of the body (whatever `.if` they stand in), each unless a sweep override names it."""
        env, prefix = dict(outer.env), outer.prefix
        for k, expr in sub.params.items():
            env[k] = eval_expr(expr, env)
        env.update(inst_params)
        for st in sub.body:
            if type(st) is Params:
                for k, expr in st.exprs.items():
                    if self.override(env, prefix, k):
                        continue
                    env[k] = inst_params[k] if k in inst_params and prefix else eval_expr(expr, env)
        for k in inst_params:
            self.override(env, prefix, k)
        return env

    def expand(self, sub, outer, inst_params):
        """`outer` carries the instance's prefix, port map and multiplier, and the environment AROUND the instance."""
        sc = outer._replace(env=self.environment(sub, outer, inst_params))
        val = lambda expr: eval_expr(expr, sc.env)  # noqa: E731
        for st in _selected(sub.body, val):
            if type(st) is Params:
                continue
            pos, kw = _split_params(st.tokens)
            m_given = "m" in kw
            m = sc.mult * (val(kw.pop("m")) if m_given else 1.0)
            handler = self.ELEMENTS.get(st.name[0])
            if handler is None:
                self.nl.warnings.append("Statement ignored: %s" % st.name)
                warnings.warn("Statement ignored: %s" % st.name)
            else:
                handler(self, sc, _Line(st.name[0], sc.prefix + st.name, pos, kw, m, m_given), val)

    def node(self, sc, n):
        n = n.lower()
        if n in ("0", "gnd", "gnd!"):
            return 0
        if n in sc.node_map:
            return sc.node_map[n]
        return self.ckt.net(sc.prefix + n)

    # -- one method per element letter (or pair) --
    def resistor(self, sc, ln, val):
        a, b = self.node(sc, ln.pos[0]), self.node(sc, ln.pos[1])
        rest, kw = ln.pos[2:], ln.kw
        if "r" in kw:
            self.ckt.R(ln.full, a, b, val(kw["r"]), m=ln.m)
        elif "l" in kw or (rest and parse_number(rest[0]) is None and not rest[0].startswith("'") and rest[0].lower() not in sc.env):
            # semiconductor resistor with a model: r = rsh*(l-short)/(w-narrow) (simpledevices.jl:66-70)
            mp = {}
            if rest and rest[0].lower() in self.nl.models:
                mp = self.nl.models[rest[0].lower()][0][2]
            if "r" in mp:  # `.model rm r R=1` (test/basic.jl:585-587)
                self.ckt.R(ln.full, a, b, mp["r"], m=ln.m)
                return
            self.ckt.R(ln.full, a, b, None, m=ln.m, rsh=mp.get("rsh", 50.0), w=val(kw["w"]) if "w" in kw else 1e-6,
                       l=val(kw["l"]) if "l" in kw else 1e-6, narrow=mp.get("narrow", 0.0), short=mp.get("short", 0.0))
        else:
            self.ckt.R(ln.full, a, b, val(rest[0]), m=ln.m)

    def reactive(self, sc, ln, val):
        add = self.ckt.C if ln.letter == "c" else self.ckt.L
        add(ln.full, self.node(sc, ln.pos[0]), self.node(sc, ln.pos[1]), val(ln.kw[ln.letter]) if ln.letter in ln.kw else val(ln.pos[2]), m=ln.m)

    def source(self, sc, ln, val):
        dc, tran, ac = _source(ln.pos[2:], ln.kw, val)
        add = self.ckt.V if ln.letter == "v" else self.ckt.I
        add(ln.full, self.node(sc, ln.pos[0]), self.node(sc, ln.pos[1]), dc=dc, tran=tran, m=ln.m, ac=ac)

    def bsource(self, sc, ln, val):
        # bsource (spectre_env.jl:127-140): v= / i= / r= / c=
        a, b = self.node(sc, ln.pos[0]), self.node(sc, ln.pos[1])
        kw = ln.kw
        if "v" in kw:
            self.ckt.V(ln.full, a, b, tran=DC(val(kw["v"])), m=ln.m)
        elif "i" in kw:
            self.ckt.I(ln.full, a, b, tran=DC(val(kw["i"])), m=ln.m)
        elif "r" in kw:
            self.ckt.R(ln.full, a, b, val(kw["r"]), m=ln.m)
        elif "c" in kw:
            self.ckt.C(ln.full, a, b, val(kw["c"]), m=ln.m)
        else:
            raise CedarError("BSOURCE with args %s not supported." % kw)

    def controlled(self, sc, ln, val):
        pos, kw = ln.pos, ln.kw
        if len(pos) >= 5:
            add = self.ckt.E if ln.letter == "e" else self.ckt.G
            add(ln.full, *[self.node(sc, p) for p in pos[:4]], gain=val(pos[4]), m=ln.m)
        else:  # two-terminal form: vol=/cur=/value= constant source
            v = kw.get("vol", kw.get("cur", kw.get("value", "0")))
            add = self.ckt.V if ln.letter == "e" else self.ckt.I
            add(ln.full, self.node(sc, pos[0]), self.node(sc, pos[1]), dc=val(v), m=ln.m)

    def mosfet(self, sc, ln, val):
        place = self._va_instance if self.nl._va_model(ln.pos[4]) is not None else self._mos
        place(ln.full, [self.node(sc, p) for p in ln.pos[:4]], ln.pos[4], ln.kw, val, ln.m)

    def instance(self, sc, ln, val):
        target, nodes, nl = ln.pos[-1].lower(), ln.pos[:-1], self.nl
        if target in nl.subckts:
            sub, m = nl.subckts[target], ln.m
            if len(nodes) != len(sub.ports):
                raise CedarError("subckt %s expects %d nodes, got %d" % (target, len(sub.ports), len(nodes)))
            nm = {p: self.node(sc, n) for p, n in zip(sub.ports, nodes)}
            if not ln.m_given and "m" in sub.params:  # `.subckt r10 a b m=10`: default multiplicity (test/basic.jl:563)
                m = sc.mult * eval_expr(sub.params["m"], sc.env)
            ip = {k: val(v) for k, v in ln.kw.items()}
            self.expand(sub, _Scope(ln.full + ".", nm, sc.env, m), ip)
        elif nl._va_model(target) is not None:
            # a compiled Verilog-A module (`.hdl "file.va"`, test/basic.jl:359-381) or a model card of one
            self._va_instance(ln.full, [self.node(sc, p) for p in nodes], target, ln.kw, val, ln.m)
        elif target in nl.models:
            # PDK style "X… nfet_06v0 W= L=": the model used as a 4-terminal subcircuit
            self._mos(ln.full, [self.node(sc, p) for p in nodes[:4]], target, ln.kw, val, ln.m)
        else:
            raise CedarError("unknown subcircuit or model '%s'" % target)

    ELEMENTS = {"r": resistor, "c": reactive, "l": reactive, "v": source, "i": source, "b": bsource, "e": controlled, "g": controlled,
                "m": mosfet, "x": instance}

    def _va_instance(self, full, nodes, model, kw, val, m):
        mod, card = self.nl._va_model(model)
        params = dict(card)
        params.update({k: val(v) for k, v in kw.items()})
        self.ckt.VA(full, mod, nodes, params=params, m=m)

    def _mos(self, full, nodes, model, kw, val, m):
        base = model.lower()
        if base not in self.nl.models:
            raise CedarError("unknown model '%s'" % model)
        p = {k: val(v) for k, v in kw.items()}
        if "w" not in p or "l" not in p:
            raise CedarError("MOSFET %s needs w= and l=" % full)
        full_name, mtype, params = self.nl.find_bin(base, p["l"], p["w"], self.ckt.scale)
        if full_name not in self.model_ix:
            self.model_ix[full_name] = self.ckt.add_model(full_name, mtype, params)
        self.ckt.M(full, nodes[0], nodes[1], nodes[2], nodes[3], self.model_ix[full_name], p["w"], p["l"],
                   nf=p.get("nf"), m=m, as_=p.get("as"), ad=p.get("ad"), ps=p.get("ps"), pd=p.get("pd"))


def _source(rest, kw, val):
    """`[DC] v` / `DC v` / `PWL(...)` / `PULSE(...)` / `SIN(...)` / `AC mag` (src/spectre.jl:1021-1062)."""
    dc, tran, ac = None, None, 0.0
    i = 0
    rest = list(rest)
    if "dc" in kw:
        dc = val(kw["dc"])
    if "ac" in kw:
        ac = val(kw["ac"])
    while i < len(rest):
        t = rest[i]
        tl = t.lower()
        if tl == "dc":
            dc = val(rest[i + 1])
            i += 2
        elif tl == "ac":  # AC mag [phase]: the phase is parsed and ignored (src/simpledevices.jl:293 "TODO phase")
            ac = val(rest[i + 1]) if i + 1 < len(rest) else 1.0
            i += 2
            while i < len(rest) and parse_number(rest[i]) is not None:
                i += 1
        elif re.match(r"^(pwl|pulse|sin)\b", tl):
            fn = re.match(r"^(pwl|pulse|sin)", tl).group(1)
            args = tl[len(fn):].strip()
            if not args and i + 1 < len(rest):
                i += 1
                args = rest[i]
            args = args.strip()
            if args.startswith("("):
                args = args[1:-1]
            vals = [val(a) for a in _tokenize(args)]
            if fn == "pwl":
                tran = PWL(vals)
            elif fn == "pulse":
                tran = PULSE(*vals)
            else:
                tran = SIN(*vals)
            i += 1
        else:
            dc = val(t)
            i += 1
    return dc, tran, ac


def parse_spectre_models(text):
    """`model <name> <master> key=value ...` statements of a Spectre-language card file (`+` continuations, `//`
    comments; everything else is ignored).  Returns {name: (master, {param: value})} with lower-case keys; values
    are numbers where they parse (magnitude suffixes as in src/spectre.jl:402-415) and strings otherwise."""
    models, cur = {}, None
    for raw in text.splitlines():
        line = raw.split("//")[0].strip()
        if not line:
            continue
        if line.lower().startswith("model "):
            toks = line.split()
            cur = {}
            models[toks[1].lower()] = (toks[2].lower(), cur)
            line = " ".join(toks[3:])
        elif line.startswith("+") and cur is not None:
            line = line[1:]
        else:
            cur = None
            continue
        for k, v in re.findall(r"([A-Za-z_]\w*)\s*=\s*(\S+)", line):
            num = parse_number(v)
            cur[k.lower()] = v.lower() if num is None else num
    return models


class _Reader:
    """One `parse_spice` call: the netlist being filled, the stack of open `.subckt`s (shared by all included files), the resolver
    and the include directories of the file being read.  `read` keeps the `.lib` section filter of its file."""

    def __init__(self, nl, include_dirs, lib_resolver):
        self.nl, self.include_dirs, self.lib_resolver = nl, include_dirs, lib_resolver
        self.stack = [nl.top]

    def read(self, text, section=None):
        """Statements of one file; with `section`, only what stands between `.lib <section>` and `.endl`."""
        in_section = section is None
        for line in _logical_lines(text):
            toks = _tokenize(line)
            if not toks:
                continue
            head = toks[0].lower()
            if section is not None:
                if head == ".lib" and len(toks) == 2:
                    in_section = toks[1].lower() == section
                    continue
                if head == ".endl":
                    in_section = False
                if not in_section:
                    continue
            if head == ".end":
                break
            if head in self.DIRECTIVES:
                self.DIRECTIVES[head](self, head, toks, line)
            elif head.startswith("."):
                self.nl.warnings.append("Statement ignored: %s" % head)
            else:
                self.stack[-1].body.append(Device(head, toks[1:]))

    def subckt(self, head, toks, line):
        if head == ".ends":
            if len(self.stack) > 1:
                self.stack.pop()
            return
        pos, kw = _split_params(toks[2:])
        pos = [p for p in pos if p.lower() != "params:"]
        sub = Subckt(toks[1].lower(), [p.lower() for p in pos], dict(kw))
        self.nl.subckts[sub.name] = sub
        self.stack.append(sub)

    def param(self, head, toks, line):
        self.stack[-1].body.append(Params(_split_params(toks[1:])[1]))

    def model(self, head, toks, line):
        name, mtype = toks[1].lower(), toks[2].lower()
        env = _global_env(self.nl.top)
        params = {k: eval_expr(v, env) for k, v in _split_params(toks[3:])[1].items()}
        base = name.split(".")[0] if re.match(r".*\.\d+$", name) else name
        self.nl.models.setdefault(base, []).append((name, mtype, params))

    def hdl(self, head, toks, line):
        # Verilog-A sources are compiled ahead of time (cedarsim.jl_amd/va/build.py); here only check that every
        # module of the named file is in the compiled library (test/basic.jl:359-381)
        path = toks[1].strip("'\"")
        for c in [path] + [os.path.join(d, path) for d in list(self.include_dirs) + [os.path.join(_VA_DIR, "library")]]:
            if os.path.isfile(c):
                for vm in parse_va_file(c):
                    if not has_module(vm.name):
                        raise CedarError("Verilog-A module '%s' of %s is not compiled into the model library: add the file to "
                                         "CEDARHIP_VA_SOURCES (or va/library) and rebuild" % (vm.name, path))
                return
        raise CedarError("cannot resolve %s %r" % (head, path))

    def include(self, head, toks, line):
        path = toks[1].strip("'\"")
        section = toks[2].lower() if (head == ".lib" and len(toks) > 2) else None
        content = self.lib_resolver(path) if self.lib_resolver is not None else None
        if content is None:
            content = next((c for c in [path] + [os.path.join(d, path) for d in self.include_dirs] if os.path.isfile(c)), None)
        if content is None:
            raise CedarError("cannot resolve %s %r" % (head, path))
        outer_dirs = self.include_dirs
        if os.path.isfile(content):
            self.include_dirs = list(outer_dirs) + [os.path.dirname(content)]
            with open(content) as f:
                content = f.read()
        if section is not None and not re.search(r"(?im)^\s*\.lib\s+%s\s*$" % re.escape(section), content):
            section = None  # library without that section: take it whole
        self.read(content, section)   # included files have no title line
        self.include_dirs = outer_dirs

    def option(self, head, toks, line):
        if head == ".temp":
            self.nl.options["temp"] = toks[1]
        else:
            self.nl.options.update(_split_params(toks[1:])[1])

    def tran(self, head, toks, line):
        env = _global_env(self.nl.top)
        self.nl.tran = (eval_expr(toks[1], env), eval_expr(toks[2], env))

    def conditional(self, head, toks, line):
        cond = line[len(head):].strip().strip("()")
        self.stack[-1].body.append({".if": If(cond), ".elseif": ElseIf(cond), ".else": Else(), ".endif": EndIf()}[head])

    def skip(self, head, toks, line):
        pass

    DIRECTIVES = {".subckt": subckt, ".ends": subckt, ".param": param, ".model": model, ".hdl": hdl, "ahdl_include": hdl,
                  ".include": include, ".inc": include, ".lib": include, ".option": option, ".options": option, ".temp": option,
                  ".tran": tran, ".if": conditional, ".elseif": conditional, ".else": conditional, ".endif": conditional}
    DIRECTIVES.update(dict.fromkeys((".global", ".endl", ".control", ".endc", ".ac", ".dc", ".op", ".print", ".plot", ".save", ".ic",
                                     ".nodeset", ".noise"), skip))


def _global_env(top):
    """The top-level `.param`s read so far, as far as they evaluate."""
    env = {}
    for st in top.body:
        if type(st) is Params:
            for k, expr in st.exprs.items():
                try:
                    env[k] = eval_expr(expr, env)
                except CedarError:
                    pass
    return env


def parse_spice(text, include_dirs=(), lib_resolver=None):
    """Parse SPICE text.  `lib_resolver(path) -> text or filename or None` lets the caller satisfy
    `.lib "jlpkg://GF180MCUPDK/..."` style references (the reference resolves them through Julia
    packages that are not available here; see DESIGN.md §6 substitute cards)."""
    nl = ParsedNetlist()
    lines = text.splitlines()
    if lines:
        nl.title = lines[0].lstrip("* ").strip()
        text = "\n".join(lines[1:])
    _Reader(nl, include_dirs, lib_resolver).read(text)
    return nl


def parse_spice_file(path, include_dirs=(), lib_resolver=None):
    with open(path) as f:
        text = f.read()
    return parse_spice(text, [os.path.dirname(os.path.abspath(path))] + list(include_dirs), lib_resolver)
