"""Case corpus of the SPICE front end (cedarsim_jl_amd.netlist / .spice_expr), shared by tests/golden/make_netlist_trace.py,
which records what the commit BEFORE the front end was rewritten did with it, and tests/test_netlist_golden.py, which holds the
rewritten front end to that record.

Expressions: `HAND_EXPRESSIONS` (text, environment) and `random_expression(seed)` over `RANDOM_ENV`.
Decks: `DECKS`, name -> (function returning the parsed netlist, list of override sets for `build`).
`expression_trace` / `deck_trace` turn either into what the trace file holds."""
import hashlib
import json
import os
import random

from cedarsim_jl_amd.circuit import CedarError
from cedarsim_jl_amd.netlist import NoBinException, eval_expr, parse_spice, parse_spice_file
from cedarsim_jl_amd.workloads import CMG_INVERTER_DECK, INVERTER_NETLIST, gf180_resolver

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- expressions ------------------------------------------------------------------------------------------------------------
E = {"a": 2.0, "b": -3.0, "c": 0.0, "s": 0.5}
_OPERATORS = ["a+b", "a-b", "a*b", "a/b", "a^2", "a**2", "a^0.5", "-a", "+a", "!a", "!c", "a==2", "a==b", "a!=2", "a!=b", "a<b", "b<a",
              "a<=2", "a<=b", "a>b", "b>a", "a>=2", "b>=a", "a&&b", "c&&b", "a||b", "c||b", "2&&3", "0||3", "0&&3", "2||3",
              "c ? a : b", "a ? a : b", "(a+b)*s", "((a))", "10-3-2", "16/4/2", "2*3/4", "2/3*4", "a - b - s", "a^b^2", "2^3^2"]
_PRECEDENCE = [  # every adjacent pair of levels, both ways round
    "c || a ? 1 : 2", "a ? 0 || 3 : 2", "c ? 1 : 0 || 3", "c ? 1 : c && 3", "a && c ? 1 : 2",
    "1 || 0 && 0", "0 && 0 || 5", "c && a || b", "a || c && b",
    "!c && a", "!a && b", "a && !c", "c || !c", "!a || b", "!!a", "!!c",
    "!a==b", "!a==2", "!(a)==0", "(!a)==0", "!a<b", "!-a", "!+c",
    "a+1 < b+10", "1 < 2 + 3", "a == 1+1", "1+1 == a", "a-1 >= 1", "b*2 <= -6", "3 > 1 + 1 + 1", "(a<b)<1", "(a>b)==(b<a)", "a<(b<1)",
    "a+b*s", "a*b+s", "a-b/s", "a/b-s", "a+b*s-a/b",
    "a*-b", "-a*b", "a/-b", "- -a", "-+-a", "a- -b", "a+-b", "a--b", "a*+b", "-a+b", "-a-b",
    "-a^2", "2**-1", "-a**-2", "2^-b", "(-a)^2", "a^-b^2", "-2^2", "+2^2", "2^-2^2", "a^-1*4", "-a^2*3", "a*b^2", "a+b^2", "b^2", "b**3",
    "1+(!c)", "a*(!c)", "(!c)+(!a)", "-(a<b)", "-(c>1)", "-(b<a)", "(a>b)+(a>0)", "(a>b)*5", "(a>b)/(b>a)", "(a>b)^2", "2^(a>b)",
    "a<b || b<a", "a<b && b<a", "a==2 && b==-3", "a==2 ? 10 : 20", "a!=2 ? 10 : 20", "!a ? 10 : 20", "-a ? 1 : 2", "c ? 1 : -2",
]
_FUNCTIONS = [
    "sqrt(16)", "sqrt(a)", "exp(1)", "exp(b)", "ln(10)", "log(10)", "log10(1000)", "abs(b)", "abs(a)", "min(a,b)", "max(a,b)", "min(1,2,3)",
    "max(1,2,3)", "min(1,2,)", "pow(2,10)", "pow(a,b)", "pow(b,2)", "pwr(b,2)", "pwr(-8,0.5)", "pwr(a,0.5)", "int(3.7)", "int(-3.7)", "nint(2.5)",
    "nint(-2.5)", "nint(0.4)", "nint(-0.4)", "nint(3.5)", "floor(-1.5)", "floor(1.5)", "ceil(1.2)", "ceil(-1.2)", "sin(1)", "cos(1)", "tan(1)",
    "atan(1)", "sinh(1)", "cosh(1)", "tanh(1)", "sgn(b)", "sgn(a)", "sgn(c)", "pi", "true", "false", "2*pi", "true+true", "!false",
    "min(a,b)+max(a,b)", "sqrt(a*a+b*b)", "exp(ln(a))", "sin(pi/2)", "atan(1)*4", "max(a<b, s)", "min(a>b, 5)", "sqrt(a>b)", "abs(-(a>b))",
    "int(a>b)", "sgn(a>b)", "floor(s)", "ceil(s)", "SQRT(16)", "Max(A,B)", "sqrt (16)", "max( a , b )", "max(-a,-b)", "pow(2,-1)", "min(!a, 1)",
]
_NUMBERS = ["1k", "1meg", "1mil", "2.5m", "1u", "10ns", "1f", "1a", "1t", "1g", "5v", "1e3k", "1K", "1MEG", "1E3", "1k+1", "2*1.5meg", "0.22u*2",
            ".5k+1", "1e-3k+0", "3hz*2", "1.e3+1", "1.+1", "2x+1", "2e+1", "1e3k*2", "5v+1mv", "1e+3+1", "1e-3-1", "1.5e3meg/2", "0.1+0.2",
            "1e308*10", "-1e308*10", "1e-320/1e10", "0*-1", "3.3333333333333e-10*3", "1mil*2", "100n/1u", "-1k", "+1k", "- 1k", "1 k"]
_QUOTING = ["'a+1'", "{a+1}", " ' a + 1 ' ", "'{a+1}'", "{'a+1'}", "'1k'", "{1k}", "{a}", "'a'", "''", "'", "{", "'a+1}", "('a')"]
_ERRORS = [  # each prefix, in the order the earlier front end decided between them
    "a $ 1", "a = 1", "a # b", "a & b", "a | b", "a % b", "foo+1", "c ? foo : 1", "a ? 1 : foo", "c && foo", "foo $ 1", "1 $ foo", "foo(1)", "x1.r+1",
    "a +", "* a", "1/c", "a/(b+3)", "sqrt(b)", "exp(1000)", "10**400", "(-8)^0.5", "b^0.5", "ln(0)", "ln(b)", "log10(c)", "a b", "1 2", "a 1", "1 a",
    "(a", "a)", "()", "min(2)", "min()", "sqrt", "sqrt+1", "abs(1,2)", "pow(1)", "pi(2)", "a(2)", "", " ", "a<>b", "a : b", "a ? b : c : s", "a ,b", "a==!c",
    "1+!c", "-!c", "a*!c", "a<!c", "2^!c", "a !", "a ! b", "! ", "a &&", "|| a", "a == ", "a < = b", "a ** ", "^2", "a^^2", "a***b", "sqrt(,1)", "sqrt(1 2)",
    "c^-1", "0^-1", "(a>a)^-1", "pwr(c,-1)", "tan(pi/2)*0", "cosh(1000)", "sinh(1000)", "pow(10,400)", "pow(b,0.5)", "sqrt(-c)", "int(1e308*10)", "a.b", "a..b+1",
]
_SHADOWING = [("pi*2", {"pi": 3.0}), ("sqrt+1", {"sqrt": 4.0}), ("sqrt(4)", {"sqrt": 4.0}), ("true", {"true": 5.0}), ("max", {"max": 7}),
              ("max(1,2)", {"maxx": 7}), ("false||e", {"e": 2.5}), ("x1.r*2", {"x1.r": 5.0}), ("x1.x2.r+_p", {"x1.x2.r": 5.0, "_p": 1.0}),
              ("r_load*2", {"r_load": 5}), ("a1+a_1", {"a1": 1.0, "a_1": 2.0}), ("1e3+e3", {"e3": 1.0}), ("2e*3", {"e": 7.0}), ("k*1k", {"k": 2.0})]
_QUIRKS = [("s ? 1/s : 0", {"s": 0.0}), ("s ? 1/s : 0", {"s": 4.0}), ("c ? 1/c : 7", E), ("a ? 7 : 1/c", E), ("c && 1/c", E), ("a || 1/c", E),
           ("a && 1/c", E), ("c ? sqrt(b) : 1", E), ("a ? 1 : ln(c)", E)]
# what the rewrite changes on purpose; make_netlist_trace.py writes their expected values by hand
NESTED_TERNARIES = [("a ? (b ? 1 : 2) : 3", 1.0), ("c ? 1 : b ? 2 : 3", 2.0), ("c ? 1 : c ? 2 : 3", 3.0), ("(c ? 1 : 2)", 2.0), ("1 + (a ? 2 : 3)", 3.0),
                    ("max(c ? 1 : 2, 3)", 3.0), ("a ? c ? 1 : 2 : 3", 2.0), ("(a ? 1 : 2) ? (c ? 3 : 4) : 5", 4.0), ("c ? 1/c : (a ? 1/a : 1/c)", 0.5)]
REJECTED_ACCIDENTS = ["a<b<1", "1<a<3", "a==a==1", "a<b>c", "a//b", "7//2", "a // s"]

HAND_EXPRESSIONS = ([(t, E) for t in _OPERATORS + _PRECEDENCE + _FUNCTIONS + _NUMBERS + _QUOTING + _ERRORS] + _SHADOWING + _QUIRKS
                    + [(t, E) for t, _ in NESTED_TERNARIES] + [(t, E) for t in REJECTED_ACCIDENTS])

RANDOM_ENV = {"a": 2.0, "b": -3.0, "c": 0.0, "s": 0.5}
N_RANDOM = 2000
_LITERALS = ["0", "1", "2", "3", "0.5", "1.5", "10", "1k", "2m", "1e-3", "2.5e2", ".25", "5v", "4.", "7", "0.1"]
_UNARY_FUNCS = ["sqrt", "exp", "ln", "log", "log10", "abs", "int", "nint", "floor", "ceil", "sin", "cos", "tan", "atan", "sinh", "cosh", "tanh", "sgn"]
_BINARY_FUNCS = ["min", "max", "pow", "pwr"]


def random_expression(seed):
    """One expression of the grammar in spice_expr's docstring: nesting depth at most 4 (parentheses and function arguments), the
    names of RANDOM_ENV, at most one ternary (at the top, where the earlier front end could read it), one comparison per level and
    never two `/` in a row — chains, `//` and nested ternaries are in the hand-written list, with hand-written expectations."""
    rng = random.Random(seed)
    sp = lambda: " " if rng.random() < 0.25 else ""  # noqa: E731

    def atom(d):
        r = rng.random()
        if d == 0 or r < 0.62:
            return rng.choice(_LITERALS) if rng.random() < 0.5 else rng.choice(sorted(RANDOM_ENV) + ["pi", "true", "false"])
        if r < 0.80:
            return "(" + sp() + logic(d - 1) + sp() + ")"
        if r < 0.94:
            return rng.choice(_UNARY_FUNCS) + "(" + logic(d - 1) + ")"
        return rng.choice(_BINARY_FUNCS) + "(" + logic(d - 1) + sp() + "," + sp() + logic(d - 1) + ")"

    def power(d):
        out = atom(d)
        if rng.random() < 0.08:
            out += sp() + rng.choice(["^", "**"]) + sp() + rng.choice(["", "", "-", "+"]) + power(d)
        return out

    def chain(d, operand, ops, more):
        out = operand(d)
        while rng.random() < more:
            out += sp() + rng.choice(ops) + sp() + operand(d)
        return out

    def signed(d):
        return rng.choice(["", "", "", "", "", "", "-", "+"]) + power(d)

    def arith(d):
        return chain(d, lambda d: chain(d, signed, ["*", "*", "/"], 0.18), ["+", "-"], 0.25)

    def compare(d):
        out = arith(d)
        if rng.random() < 0.15:
            out += sp() + rng.choice(["==", "!=", "<", "<=", ">", ">="]) + sp() + arith(d)
        return out

    def logic(d):
        negated = lambda d: ("!" + sp() if rng.random() < 0.08 else "") + compare(d)  # noqa: E731
        return chain(d, lambda d: chain(d, negated, ["&&"], 0.08), ["||"], 0.08)

    out = logic(4)
    if rng.random() < 0.15:
        out += sp() + "?" + sp() + logic(4) + sp() + ":" + sp() + logic(4)
    return rng.choice(["%s", "%s", "'%s'", "{%s}"]) % out


def expression_trace(text, env):
    """`float.hex()` of the value, or "CedarError"."""
    try:
        return eval_expr(text, dict(env)).hex()
    except CedarError:
        return "CedarError"


# ---- decks --------------------------------------------------------------------------------------------------------------------
RESISTORS = """* resistor forms
.param rv=2k
.model rm r r=1
.model rsheet r rsh=20 narrow=0.1u short=0.2u
r1 a 0 1k
r2 a b r=rv
r3 b 0 rm
r4 b c rsheet w=2u l=10u
r5 c 0 nomodel
r6 c 0 'rv*2' m=2
r7 c 0 rsheet l=5u
r8 a c rv
r9 a c l=3u w=1.5u
v1 a gnd 1
"""
CAPS_INDUCTORS = """* c and l, positional and by keyword
.param cv=1p
c1 a 0 1p
c2 a b c=2p
c3 a b 'cv*3' m=2
l1 b 0 1u
l2 b c l='2u' m=3
v1 a 0 1
"""
SOURCES = """* every source form
.param amp=5
v1 a 0 5
v2 b 0 DC 3
v3 c 0 dc=2 ac=0.5
v4 d 0 AC 1 45
v5 e 0 AC
i1 a 0 1m
v6 f 0 PWL(0 0 1n 5)
v7 g 0 PWL (0 0 1n amp 2n 0)
v8 h 0 PULSE(0 amp 1n 1n 1n 10n 20n)
v9 i 0 PULSE (0 5 1n)
v10 j 0 SIN(0 1 1meg)
i2 k 0 SIN (0.5 0.1 1e7 0 0 90)
v11 l 0 DC 1 AC 2 PWL(0 1 1n 2)
i3 m 0 dc 1 ac 1 0 sin(0 'amp/5' 1k) m=2
v12 n 0 'amp*2'
i4 n 0 dc=1m
v13 o 0 pwl(0,0,1n,1)
"""
BSOURCE = """* b sources
b1 a 0 v=1
b2 a b i='1m'
b3 b 0 r=1k
b4 b 0 c=1p m=2
"""
CONTROLLED = """* e and g
.param gain=2
e1 out 0 in 0 gain
g1 out 0 in 0 1m m=2
e2 a 0 vol=3
g2 a 0 cur='1m'
e3 b 0 value=gain
g3 b 0
e4 c 0 cur=4
v1 in 0 1
"""
MOS = """* BSIM4 cards, one shared by two instances, one used as a subcircuit
.param wn=1u
.model n1 nmos level=54 vth0=0.5 toxe=2n
.model p1 pmos level=14 vth0=-0.5
m1 d g 0 0 n1 w=wn l=1u nf=2 as=1p ad=1p ps=1u pd=1u m=2
m2 d g 0 0 n1 w='2*wn' l=0.5u
m3 d g vdd vdd p1 w=1u l=1u
x4 d g 0 0 n1 w=1u l=1u
v1 vdd 0 1
"""
VA_MODULES = """* compiled Verilog-A modules and model cards of them
.hdl "cedar_basic.va"
.param rr=2k
.model dmod va_diode is=3e-14 rs=2
.model mm va_mos1 vto=0.6
x1 vcc 0 va_resistor r=rr
x2 a 0 dmod n=1.2
m1 d g 0 0 mm w=2u l=1u
m2 d g 0 0 va_mos1 w=1u m=2
x3 d g 0 0 mm
v1 vcc 0 dc=1
"""
CMG_LEVEL72 = """* BSIM-CMG through level 72, and through a card whose master is the module
.model nmos_lvt nmos level=72 version=107 l=2.1e-8 nfin=2 tfin=6.5e-9 hfin=3.2e-8 eot=1e-9 phig=4.3 igcmod=1 gidlmod=1
.model pmos_lvt pmos level=72 l=2.1e-8 nfin=3 tfin=6.5e-9 hfin=3.2e-8 eot=1e-9 phig=4.8
mneg Q D VSS VSS nmos_lvt
mpos Q D VDD VDD pmos_lvt
xn Q D VSS VSS ncard nfin=4
xp Q D VDD VDD pcard
VVDD VDD 0 1.0
VD D 0 AC 1 SIN (0.5 0.4 1e7)
.TRAN 1e-9 4.0e-7
.END
"""
HIERARCHY = """* subcircuits, parameters and multipliers
.param top_r=1k
.subckt leaf a b rl=100
r1 a b 'rl'
.ends
.subckt mid a b params: k=2
.param inner=3
x1 a n leaf rl='k*inner'
x2 n b leaf m=2
r2 a b 'inner*top_r'
.ends mid
.subckt r10 a b m=10
r1 a b 1
.ends
x1 in 0 mid k=4 m=3
x2 in 0 mid
x3 in 0 r10
x4 in 0 r10 m=2
x5 in gnd mid inner=8
v1 in 0 1
.ends
"""
IF_CHAIN = """* if / elseif / else
.param s=1
.if (s==1)
r1 a 0 1
.elseif (s==2)
r2 a 0 2
.else
r3 a 0 3
.endif
v1 a 0 1
"""
IF_CHAIN_S1 = "* if / elseif / else\n.param s=1\nr1 a 0 1\nv1 a 0 1\n"   # what IF_CHAIN is with s=1
_IF_NESTED = ("* nested conditionals\n.param s=1 t=0\n", """.if (t)
.if (s==1)
r4 a 0 4
.else
r5 a 0 5
.endif
.elseif (s==1)
.if (t==0)
r6 a 0 6
.elseif (s==1)
r7 a 0 7
.else
r8 a 0 8
.endif
r9 a 0 9
.elseif (s==2)
r10 a 0 10
.else
.if (s==3)
r11 a 0 11
.endif
r12 a 0 12
.endif
""", """.subckt sub a b sel=0
.if (sel)
r1 a b 1
.else
c1 a b 1p
.endif
.ends
x1 a 0 sub sel=1
x2 a 0 sub
v1 a 0 1
""")
IF_NESTED = "".join(_IF_NESTED)
IF_SKIPS_BAD_BRANCH = """* a branch that is not taken may hold anything
.param s=0
.if (s)
r1 a 0 'undefined_name*2'
r2 a 0 '1 +* 2'
.else
r3 a 0 3
.endif
v1 a 0 1
"""
DIRECTIVES = """  *  the title line
.option temp=50 gmin=1e-14
.options scale=0.5
.temp 75
.param tstop=1u
.tran 1n 'tstop*2'
.model n1 nmos level=54 vth0='0.4+tstop*1e5' lmin=0 lmax=1 wmin=0 wmax=1
.global vdd
.op
.print v(a)
.fourier 1k v(a)
.measure tran x max v(a)
q1 a b c npn
d1 a 0 dmodel
r1 a 0 1 $ a comment
r2 a 0 2 ; another
r3 a
+ 0
+    3
* a whole-line comment

   * an indented one
R4 A GND 4
r5 a gnd! 5
m1 a a 0 0 n1 w=1u l=1u
V1 a 0 1
.END
r6 a 0 6
"""
_TEXTS = {"inc1.cir": "r_inc a 0 1\n.param pinc=3\n.subckt fromlib a b\nr1 a b 'pinc'\n",   # the .subckt stays open across the file's end
          "inc2.cir": ".ends\n.include 'inc3.cir'\n",
          "inc3.cir": "r_inc3 a 0 3\n",
          "lib1.lib": "r_outside a 0 99\n.lib slow\nr_slow a 0 10\n.endl\n.lib fast\nr_fast a 0 1\n.param pfast=2\n.endl fast\nr_after a 0 98\n",
          "lib2.lib": "r_whole a 0 7\n.end\nr_never a 0 1\n"}
INCLUDES = """* .include and .lib through a resolver
.include "inc1.cir"
.inc inc2.cir
.lib "lib1.lib" fast
.lib 'lib2.lib' nosuch
r_main a 0 'pfast*pinc'
x1 a 0 fromlib
v1 a 0 1
"""
FAULTS = {   # decks that fail while they are flattened
    "bsource_error": "* t\nb1 a 0 q=1\n",
    "mos_missing_wl": "* t\n.model n1 nmos level=54\nm1 d g 0 0 n1 w=1u\n",
    "mos_unknown_model": "* t\nm1 d g 0 0 nope w=1u l=1u\n",
    "x_wrong_port_count": "* t\n.subckt leaf a b\nr1 a b 1\n.ends\nx1 a b c leaf\n",
    "x_unknown_target": "* t\nx1 a 0 no_such_thing r=1\nv1 a 0 1\n",
    "undefined_parameter": "* t\nr1 a 0 'nope*2'\n",
    "bad_model_parameter": "* t\n.model n1 nmos level=54 notaparam=1\nm1 d g 0 0 n1 w=1u l=1u\n",
    "negative_multiplier": "* t\nr1 a 0 1 m=-1\n",
}
PARSE_FAULTS = {   # decks that fail while they are read
    "include_unresolved": "* t\n.include 'not_there.cir'\n",
    "hdl_unresolved": "* t\n.hdl 'not_there.va'\n",
    "hdl_unknown_module": "* t\n.hdl \"uncompiled_module.va\"\n",
    "model_with_undefined_parameter": "* t\n.model n1 nmos level=54 vth0='nope'\n",
    "tran_with_undefined_parameter": "* t\n.tran 1n tstop\n",
}


def _text(text, **kw):
    return lambda: parse_spice(text, **kw)


def _binned():
    body = open(os.path.join(GOLD, "bins_nmos_3p3.cir")).read().split("\n", 1)[1]
    return parse_spice("* binning\n.param wv=1u lv=1u\nm0 d1 g s1 b nmos_3p3 W=wv l=lv\n" + body)


def _cmg_level72():
    nl = parse_spice(CMG_LEVEL72)
    nl.add_model_cards({"Ncard": {"master": "BSIMCMG107", "params": {"type": "n", "l": 2.1e-8, "nfin": 2.0, "level": 110.0, "version": 107.0}},
                        "pcard": {"master": "bsimcmg", "params": {"type": "p", "l": 2.1e-8}}})
    return nl


def _cmg_inverter_array():   # the deck of workloads.cmg_inverter_array(2, cards)
    insts = ["mneg%d q%d D VSS VSS nmos_lvt\nmpos%d q%d D VDD VDD pmos_lvt" % (k, k, k, k) for k in range(2)]
    nl = parse_spice(CMG_INVERTER_DECK % {"amp": 0.01, "insts": "\n".join(insts)})
    nl.add_model_cards(json.load(open(os.path.join(GOLD, "asap7_tt_lvt_cards.json")))["cards"])
    return nl


def _spectre_cards():
    nl = parse_spice("* cards of a Spectre file\nxn q d 0 0 nmos_x\nmp q d vdd vdd pmos_x nfin=3\nv1 vdd 0 1\n")
    nl.add_spectre_models("model nmos_x bsimcmg type=n l=21n\n+ nfin=2 // comment\nmodel pmos_x bsimcmg type=p\n+ l = 21n\n")
    return nl


DECKS = {
    "resistors": (_text(RESISTORS), [{}, {"rv": 5e3}]),
    "caps_inductors": (_text(CAPS_INDUCTORS), [{}, {"CV": 2e-12}]),
    "sources": (_text(SOURCES), [{}, {"amp": 2.5}]),
    "bsource": (_text(BSOURCE), [{}]),
    "controlled": (_text(CONTROLLED), [{}, {"gain": -1.0}]),
    "mos": (_text(MOS), [{}, {"wn": 3e-6}, {"temp": 85.0, "gmin": 1e-13, "scale": 2.0}]),
    "binned": (_binned, [{}, {"wv": 0.22e-6, "lv": 0.28e-6}, {"wv": 1e-3}, {"scale": 0.5}, {"lv": 0.5e-6}]),
    "bins_file": (lambda: parse_spice_file(os.path.join(GOLD, "bins_nmos_3p3.cir")), [{}]),
    "va_modules": (_text(VA_MODULES), [{}, {"rr": 3e3}]),
    "cmg_level72": (_cmg_level72, [{}]),
    "cmg_inverter_array": (_cmg_inverter_array, [{}]),
    "spectre_cards": (_spectre_cards, [{}]),
    "hierarchy": (_text(HIERARCHY), [{}, {"top_r": 2e3}, {"x1.inner": 5.0}, {"x1.k": 7.0}, {"x1.x1.rl": 1.0}, {"x5.inner": 1.0, "X2.INNER": 2.0},
                                     {"nonexistent": 1.0}, {"x2.k": 9.0}, {"top_r": 1.0, "x1.nonexistent": 2.0}]),
    "if_chain": (_text(IF_CHAIN), [{}, {"s": 2.0}, {"s": 3.0}]),
    "if_nested": (_text(IF_NESTED), [{}, {"s": 2.0}, {"s": 3.0}, {"t": 1.0}, {"t": 1.0, "s": 2.0}, {"s": 4.0}, {"x2.sel": 1.0}]),
    "if_skips_bad_branch": (_text(IF_SKIPS_BAD_BRANCH), [{}, {"s": 1.0}]),
    "directives": (_text(DIRECTIVES), [{}, {"tstop": 5e-6}, {"temp": 0.0}]),
    "includes": (_text(INCLUDES, lib_resolver=_TEXTS.get), [{}, {"pinc": 4.0}]),
    "include_file": (_text("* a file found through include_dirs\n.include 'bins_nmos_3p3.cir'\n.lib bins_nmos_3p3.cir nosuch\n", include_dirs=[GOLD]), [{}]),
    "dff": (lambda: parse_spice_file(os.path.join(GOLD, "DFF_cap_all.cir"), lib_resolver=gf180_resolver), [{}, {"gmin": 1e-12}]),
    "inverter": (_text(INVERTER_NETLIST, lib_resolver=gf180_resolver), [{}]),
    "empty": (_text(""), [{}]),
}
DECKS.update({name: (_text(text), [{}]) for name, text in FAULTS.items()})
DECKS.update({name: (_text(text, include_dirs=[GOLD]), [{}]) for name, text in PARSE_FAULTS.items()})
# (deck, index of the override set) -> deck that says the same without conditionals: the `.if` branches that the earlier front
# end took wrongly (after a taken `.if`, the `.else` behind an `.elseif`) are recorded from these
CORRECTED = {("if_chain", 0): _text(IF_CHAIN_S1),                                                     # s=1: r1, and no r3
             ("if_nested", 0): _text(_IF_NESTED[0] + "r6 a 0 6\nr9 a 0 9\n" + _IF_NESTED[2]),         # s=1 t=0: no r8, no r12
             ("if_nested", 3): _text(_IF_NESTED[0] + "r4 a 0 4\n" + _IF_NESTED[2]),                   # s=1 t=1: no r12
             ("if_nested", 4): _text(_IF_NESTED[0] + "r5 a 0 5\n" + _IF_NESTED[2])}                   # s=2 t=1: no r10


def _canon(x):
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        return "nan" if x != x else x.hex()
    if isinstance(x, dict):
        return sorted((k, _canon(v)) for k, v in x.items())
    return [_canon(v) for v in x]


def _digest(x):
    return hashlib.sha256(json.dumps(_canon(x)).encode()).hexdigest()[:16]


def circuit_groups(nl, c):
    """The flattened circuit and what the netlist holds beside it, by field group (not digested: for comparing two builds)."""
    return {"nodes": c.node_names,
            "devices": [c.dev_names, c.dev_kind, c.dev_node, c.dev_ipar, c.dev_par, c.dev_mult],
            "sources": [[(dc, w.kind, w.par, w.ts, w.ys) for dc, w in c.sources], c.source_ac],
            "models": [c.model_names, c.models],
            "va_par": c.va_par,
            "spec": [c.temp, c.gmin, c.scale],
            "tran_options": [nl.tran, nl.options],
            "warnings": nl.warnings}


def deck_trace(parse, overrides):
    """One entry per override set: {group: 16 hex digits of its sha256}, or the class name of what `build` raised; the class name
    alone where reading the deck raised already."""
    try:
        nl = parse()
    except (CedarError, NoBinException) as e:
        return type(e).__name__
    out = []
    for ov in overrides:
        try:
            out.append({k: _digest(v) for k, v in circuit_groups(nl, nl.build(**ov)).items()})
        except (CedarError, NoBinException) as e:
            out.append(type(e).__name__)
    return out
