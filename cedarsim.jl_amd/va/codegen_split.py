"""Setup / eval split of a module's analog block (binding-time analysis).

The reference constant-folds everything that depends only on the instance parameters when it compiles the circuit
(`DefaultSim` parameters are compile-time constants, src/circuitodesystem.jl:57-62).  Here the analog block is split
into `setup(P, env, C)`, which runs the bias-independent statements once per instance and parameter change and stores
what the rest needs into the per-instance constant block C, and `eval(P, C, V, ...)`, the bias-dependent remainder.
The analysis is flow-sensitive (BSIM code reuses its temporaries T0..T9 for both kinds of value): walking the statements
in order, `state[var]` is the slot of C that holds the variable's current value, or None once it depends on a node
voltage (by data, or by being assigned under a bias-dependent condition).  Conditions that are themselves
bias-independent are kept as control flow on both sides (their truth value is a slot); where the branches disagree
about a variable, a merge slot (both static) or a materialisation `v = C[slot]` at the end of the static branch is made.

Slots are numbered as they are made and written `@N@` in the text; `Split.run` drops the stores nobody loads and renumbers
the rest densely.
"""
import itertools
import re
from dataclasses import dataclass, replace

from .codegen_emit import Pass, walk
from .frontend import FLOW_ACCESS, POTENTIAL_ACCESS, VAError


@dataclass(frozen=True)
class Hoist:
    """What the eval pass knows at one statement: which variables sit in C, and where setup code for a hoisted value goes."""
    split: "Split"
    setup: Pass       # the pass that computes hoisted values (plain doubles)
    state: dict       # variable -> slot of C holding its value | -1 never assigned | None bias-dependent
    sink: list        # setup lines of the statement being split, or None where nothing may be hoisted (inside a loop)
    pad: str          # indentation of lines added to `sink`

    def shadowed(self, local_types):
        return replace(self, state=dict(self.state, **dict.fromkeys(local_types)))

    def load_var(self, name, ty):
        slot = self.state.get(name)
        return None if slot is None else self.split.load(slot, ty)

    def load_static(self, e, vars_):
        """A bias-independent sub-expression of a bias-dependent statement: evaluated by setup() at this point of the (static)
        control flow, loaded here.  None when `e` is not one, or not worth a slot."""
        sp = self.split
        if self.sink is None or not _worth_hoisting(e) or not sp.is_static(e, self.state, vars_):
            return None
        c, t = sp.g.expr(e, self.setup)
        slot = next(sp.slots)
        self.sink.append((slot, "%sC[@%d@] = (double)(%s);" % (self.pad, slot, c)))
        return sp.load(slot, t)


def _worth_hoisting(e):
    if e[0] == "bin":
        return e[1] in ("/", "**")
    return e[0] == "call" and not e[1].startswith("$") and e[1] not in POTENTIAL_ACCESS and e[1] not in FLOW_ACCESS and e[1] not in ("ddx", "ddt", "white_noise", "flicker_noise")


class Split:
    """One run over one module: `run()` -> (setup lines, eval lines, number of doubles in C)."""

    def __init__(self, emitter, vars_):
        self.g, self.m, self.vars = emitter, emitter.m, vars_
        self.slots, self.used = itertools.count(), set()   # slots made, slots that eval loads

    def run(self):
        state = {nm: -1 for nm in self.vars if nm not in self.m.arrays}
        sc = Pass("double", {k: ("real" if t == "dual" else t) for k, t in self.vars.items()}, plain=True, contrib="none")
        ec = Pass("R", dict(self.vars))
        S, E = [], []
        for st in self.m.analog:
            s_, e_ = self.stmt(st, state, False, sc, ec, 1)
            S += s_
            E += e_
        final = {k: i for i, k in enumerate(sorted(self.used))}

        def finish(lines):
            out = []
            for ln in lines:
                if isinstance(ln, tuple):
                    if ln[0] not in final:
                        continue
                    ln = ln[1]
                out.append(re.sub(r"@(\d+)@", lambda mo: str(final[int(mo.group(1))]), ln))
            return out
        return finish(S), finish(E), len(final)

    # ---- slots ----
    def load(self, slot, ty):
        if slot < 0:   # never assigned so far: Verilog-A variables start at zero
            return ("0", "int") if ty == "int" else ("0.0", "real")
        self.used.add(slot)
        return ("(int)C[@%d@]" % slot, "int") if ty == "int" else ("C[@%d@]" % slot, "real")

    def _materialise(self, name, slot, ty, pad):
        c, t = self.load(slot, ty)
        return "%sv_%s = %s;" % (pad, name, self.g.cast(c, t, ty, "R"))

    def _make_dynamic(self, st, state, ec, E, pad):
        """what `st` may assign is bias-dependent from here on: variables that sat in C get their value first"""
        for nm in sorted(self._assigned(st)):
            if state.get(nm) is not None:
                if nm in ec.vars:
                    E.append(self._materialise(nm, state[nm], ec.vars[nm], pad))
                state[nm] = None

    # ---- binding times ----
    def is_static(self, e, state, vars_):
        k = e[0]
        if k in ("num", "str"):
            return True
        if k == "id":
            if e[1] in vars_:
                return state.get(e[1]) is not None
            return e[1] in self.g.param_ix
        if k == "index":
            return False
        if k == "un":
            return self.is_static(e[2], state, vars_)
        if k == "bin":
            return self.is_static(e[2], state, vars_) and self.is_static(e[3], state, vars_)
        if k == "tern":
            return all(self.is_static(x, state, vars_) for x in e[1:4])
        if k == "call":
            name = e[1]
            if name in POTENTIAL_ACCESS or name in FLOW_ACCESS or name in ("ddx", "ddt", "$simparam", "$limit", "$abstime", "$realtime"):
                return False     # $simparam("gmin") changes between launches of one solve (gmin stepping)
            if name in ("$param_given", "$given", "$mfactor", "$port_connected", "white_noise", "flicker_noise"):
                return True
            if name in self.m.functions and any(kind != "input" for _, kind in self.m.functions[name].args):
                return False
            return all(self.is_static(a, state, vars_) for a in e[2] if a[0] != "str")
        return False

    def _assigned(self, st):
        """names that a statement subtree may assign (output arguments of analog functions included)"""
        out = set()
        for n in walk(st):
            if not n or not isinstance(n[0], str):
                continue
            if n[0] in ("assign", "assign_idx"):
                out.add(n[1])
            elif n[0] == "call" and n[1] in self.m.functions:
                for (nm, kind), a in zip(self.m.functions[n[1]].args, n[2]):
                    if kind != "input" and a[0] == "id":
                        out.add(a[1])
        return out

    # ---- statements: one method per kind ----
    def stmt(self, st, state, dyn, sc, ec, ind):
        """-> (setup lines, eval lines); setup lines that only store a slot are (slot, text) pairs, dropped later if unused.
        `dyn`: under bias-dependent control.  `sc` / `ec`: the setup and eval passes with the variables in scope here."""
        while st is not None and st[0] == "event":
            st = st[1]
        if st is None or st[0] in ("task", "null"):
            return [], []
        split = self._STATEMENTS.get(st[0])
        if split is None:
            raise VAError("cannot generate statement %r" % (st,))
        return split(self, st, state, dyn, sc, ec, ind)

    def _at(self, ec, sc, state, sink, ind):
        """the eval pass at one statement: loads from `state`, hoists into `sink` what `sc` computes"""
        return replace(ec, hoist=Hoist(self, sc, state, sink, "  " * ind))

    def _assign(self, st, state, dyn, sc, ec, ind):
        name, pad = st[1], "  " * ind
        if name not in ec.vars:
            raise VAError("assignment to undeclared variable '%s' in module %s" % (name, self.m.name))
        if not (name in state and not dyn and not self._assigned(st[2]) and self.is_static(st[2], state, ec.vars)):
            return self._opaque(st, state, dyn, sc, ec, ind)
        c, t = self.g.expr(st[2], sc)
        state[name] = slot = next(self.slots)
        return ["%sv_%s = %s;" % (pad, name, self.g.cast(c, t, sc.vars[name], "double")), (slot, "%sC[@%d@] = (double)v_%s;" % (pad, slot, name))], []

    def _opaque(self, st, state, dyn, sc, ec, ind):
        """bias-dependent assignments, array assignments and contributions: on the eval side, as the plain emitter writes them"""
        S = []
        outs = self._assigned(st)
        E = self.g.stmt(st, self._at(ec, sc, state, S, ind), ind)
        for nm in outs:
            if nm in state:
                state[nm] = None
        return S, E

    def _case(self, st, state, dyn, sc, ec, ind):
        """lowered to an if / else-if chain on `selector == label`"""
        sel, default, chain = st[1], None, []
        for conds, body in st[2]:
            if conds is None:
                default = body
                continue
            test = None
            for cd in conds:
                t1 = ("bin", "==", sel, cd)
                test = t1 if test is None else ("bin", "||", test, t1)
            chain.append((test, body))
        node = default
        for test, body in reversed(chain):
            node = ("if", test, body, node)
        return self.stmt(node, state, dyn, sc, ec, ind)

    def _if(self, st, state, dyn, sc, ec, ind):
        cond, pad = st[1], "  " * ind
        if not dyn and not self._assigned(cond) and self.is_static(cond, state, ec.vars):
            return self._if_static(st, state, sc, ec, ind)
        S, E = [], []
        self._make_dynamic(st, state, ec, E, pad)
        c, _ = self.g.expr(cond, self._at(ec, sc, state, S, ind))
        SA, EA = self.stmt(st[2], state, True, sc, ec, ind + 1)
        SB, EB = self.stmt(st[3], state, True, sc, ec, ind + 1)
        S += SA + SB
        E += ["%sif (va::truth(%s)) {" % (pad, c)] + EA + (["%s} else {" % pad] + EB if EB else []) + ["%s}" % pad]
        return S, E

    def _if_static(self, st, state, sc, ec, ind):
        """a bias-independent condition: control flow on both sides, its truth value in a slot"""
        pad, S, E = "  " * ind, [], []
        cs, _ = self.g.expr(st[1], sc)
        kc = next(self.slots)
        S.append((kc, "%sC[@%d@] = va::truth(%s) ? 1.0 : 0.0;" % (pad, kc, cs)))
        stA, stB = dict(state), dict(state)
        SA, EA = self.stmt(st[2], stA, False, sc, ec, ind + 1)
        SB, EB = self.stmt(st[3], stB, False, sc, ec, ind + 1)
        post = []
        for nm in list(state):
            a, b = stA.get(nm), stB.get(nm)
            if a == b:
                state[nm] = a
            elif a is not None and b is not None:
                km = next(self.slots)
                post.append((km, "%sC[@%d@] = (double)v_%s;" % (pad, km, nm)))
                state[nm] = km
            else:
                (EA if a is not None else EB).append(self._materialise(nm, a if a is not None else b, ec.vars[nm], pad + "  "))
                state[nm] = None
        S += ["%sif (va::truth(%s)) {" % (pad, cs)] + SA + ["%s} else {" % pad] + SB + ["%s}" % pad] + post
        if EA or EB:
            self.used.add(kc)
            E += ["%sif (C[@%d@] != 0.0) {" % (pad, kc)] + EA + (["%s} else {" % pad] + EB if EB else []) + ["%s}" % pad]
        return S, E

    def _block(self, st, state, dyn, sc, ec, ind):
        pad = "  " * ind
        S, E = ["%s{" % pad], ["%s{" % pad]
        saved = {}
        if st[2]:
            types = self.g.local_types(st[2], ec)
            ec = replace(ec, vars=dict(ec.vars, **types))
            sc = replace(sc, vars=dict(sc.vars, **{nm: "int" if t == "int" else "real" for nm, t in types.items()}))
            for nm, t in types.items():
                E.append(self.g.decl(nm, t, "R", pad + "  "))
                S.append(self.g.decl(nm, sc.vars[nm], "double", pad + "  "))
                saved[nm] = state.get(nm, "absent")
                if nm in self.m.arrays:
                    state.pop(nm, None)
                else:
                    state[nm] = -1
        n_body = 0
        for s1 in st[3]:
            s_, e_ = self.stmt(s1, state, dyn, sc, ec, ind + 1)
            S += s_
            E += e_
            n_body += len(e_)
        for nm, old in saved.items():
            if old == "absent":
                state.pop(nm, None)
            else:
                state[nm] = old
        S.append("%s}" % pad)
        # nothing bias-dependent in this block: no block on the eval side
        return S, (E + ["%s}" % pad] if n_body else [])

    def _loop(self, st, state, dyn, sc, ec, ind):
        """for / while / repeat: on the eval side as a whole, nothing hoisted out of it"""
        E = []
        self._make_dynamic(st, state, ec, E, "  " * ind)
        return [], E + self.g.stmt(st, self._at(ec, sc, state, None, ind), ind)

    _STATEMENTS = {"assign": _assign, "assign_idx": _opaque, "contrib": _opaque, "case": _case, "if": _if, "block": _block, "for": _loop,
                   "while": _loop, "repeat": _loop}
