"""`.measure` cards and measure constructors (cedarsim.jl_amd/measure.py) on the CPU: every supported SPICE form, refusal by name of
`PARAM=` and of an unknown node, and the symbols-to-rows step against a circuit's observables (no GPU: nothing here loads the engine)."""
import ctypes as C
import math

import pytest

from cedarsim_jl_amd import Circuit, CedarError, PWL
from cedarsim_jl_amd import measure as M


def rc():
    c = Circuit()
    c.V("vin", "in", 0, tran=PWL([0.0, 0.0, 1e-12, 1.0, 1.0, 1.0]))
    c.R("r1", "in", "out", 1e3)
    c.C("c1", "out", 0, 1e-12)
    c.observe_node("in")
    c.observe_node("out")
    c.observe_branch("vin")
    return c


def test_trig_targ():
    m = M.parse_measure(".measure tran tpd TRIG v(in) VAL=0.5 RISE=1 TARG v(out) VAL=0.5 RISE=2 TD=1n")
    assert m == M.delay("tpd", M.event("in", 0.5, "rise", 1), M.event("out", 0.5, "rise", 2, 1e-9))
    m = M.parse_measure(".MEAS TRAN Slew trig V(out) val = 0.1 fall=last targ v( out , in ) val=-0.9 cross=3")
    assert m.name == "slew" and m.trig == M.event("out", 0.1, "fall", "last") and m.targ == M.event(("out", "in"), -0.9, "cross", 3)


def test_when_and_find():
    assert M.parse_measure(".meas tran t50 when v(out)=0.5") == M.when("t50", "out", 0.5, "cross", 1)
    assert M.parse_measure(".meas tran t50 when v(out) val=500m fall=2 td=2n") == M.when("t50", "out", 0.5, "fall", 2, 2e-9)
    assert M.parse_measure(".meas tran t50 when v(out)=0.5 last") == M.when("t50", "out", 0.5, "cross", "last")
    assert M.parse_measure(".meas tran ix find i(vin) when v(out)=0.5 rise=1") == M.find_when("ix", "vin.i", M.event("out", 0.5, "rise"))
    assert M.parse_measure(".meas tran v1 find v(out,in) at=1.5n") == M.find_at("v1", ("out", "in"), 1.5e-9)


@pytest.mark.parametrize("word, make", [("avg", M.avg), ("rms", M.rms), ("min", M.vmin), ("max", M.vmax), ("pp", M.pp), ("integ", M.integ), ("integral", M.integ)])
def test_windows(word, make):
    assert M.parse_measure(".measure tran x %s v(out) from=1n to=2u" % word.upper()) == make("x", "out", 1e-9, 2e-6)
    m = M.parse_measure(".measure tran x %s i(vin)" % word)
    assert m == make("x", "vin.i") and m.frm == -math.inf and m.to == math.inf


def test_cards_of_a_deck():
    deck = """* rc
vin in 0 pwl(0 0 1p 1)
r1 in out 1k
c1 out 0 1p
.tran 1p 10n
.measure tran tpd trig v(in) val=0.5 rise=1
+ targ v(out) val=0.5 rise=1 ; the delay
* .measure tran commented max v(out)
.MEAS tran peak max v(out)
.end
"""
    got = M.measure_cards(deck)
    assert [m.name for m in got] == ["tpd", "peak"] and got[0].kind == "delay" and got[0].targ == M.event("out", 0.5, "rise") and got[1] == M.vmax("peak", "out")
    assert M.measure_cards("r1 a b 1k\n.end\n") == []


@pytest.mark.parametrize("card, text", [
    (".measure tran p2 param='tpd*2'", "p2: PARAM="),
    (".measure tran p2 param = tpd", "p2: PARAM="),
    (".measure tran d1 deriv v(out) at=1n", "d1: DERIV"),
    (".measure ac g max vdb(out)", "g: only TRAN"),
    (".measure tran x trig v(in) val=0.5", "x: TRIG without TARG"),
    (".measure tran x when v(out)=0.5 rise=0", "count"),
    (".measure tran x when v(out)=0.5 slope=1", "x: unknown option 'slope=1'"),
    (".measure tran x avg out", "x: expected v(node)"),
    (".measure tran x find v(out)", "x: FIND needs"),
    (".measure tran x when v(out)=abc", "x: the level must be a number"),
    (".measure tran x median v(out)", "x: unknown measurement 'MEDIAN'"),
    ("r1 a b 1k", "not a .measure card"),
])
def test_refusals_name_the_measure(card, text):
    with pytest.raises(CedarError) as e:
        M.parse_measure(card)
    assert text in str(e.value), str(e.value)


def test_symbols_to_rows():
    c = rc()
    names, arr = M.resolve_measures(c, [M.delay("tpd", M.event("in", 0.5, "rise"), M.event("node_out", 0.5, "rise", "last", 1e-9)), M.avg("iavg", "vin.i", 0.0, 5e-9),
                                        M.find_when("dv", ("out", "in"), M.event("out", 0.1)), M.vmax("ir", "r1.i"), M.rms("vc", "c1.v")])
    assert names == ["tpd", "iavg", "dv", "ir", "vc"] and C.sizeof(M.ChMeasureSpec) == 112 and C.sizeof(M.ChMeasureSide) == 40
    i_in, i_out, i_br = c.obs.index(("v", c._n("in"))), c.obs.index(("v", c._n("out"))), c.obs.index(("i", c.dev_names.index("vin")))
    d = arr[0]
    assert (d.kind, d.s1.row_a, d.s1.row_b, d.s1.level, d.s1.edge, d.s1.count, d.s1.td) == (1, i_in, -1, 0.5, 1, 1, -math.inf)
    assert (d.s2.row_a, d.s2.row_b, d.s2.edge, d.s2.count, d.s2.td) == (i_out, -1, 1, -1, 1e-9)
    assert (arr[1].kind, arr[1].s1.row_a, arr[1].s1.row_b, arr[1].frm, arr[1].to) == (5, i_br, -1, 0.0, 5e-9)
    assert (arr[2].kind, arr[2].s1.row_a, arr[2].s2.row_a, arr[2].s2.row_b, arr[2].s2.scale) == (2, i_out, i_out, i_in, 1.0)
    assert (arr[3].kind, arr[3].s1.row_a, arr[3].s1.row_b, arr[3].s1.scale) == (8, i_in, i_out, 1e-3)        # r1.i = (v(in) - v(out)) / R
    assert (arr[4].kind, arr[4].s1.row_a, arr[4].s1.row_b, arr[4].s1.scale) == (6, i_out, -1, 1.0)            # c1.v = v(out) - 0
    # KINDS and EDGES are the C enums, in order
    assert M.KINDS == ("when", "delay", "find_when", "find_at", "integ", "avg", "rms", "min", "max", "pp") and M.EDGES == {"rise": 1, "fall": 2, "cross": 3}


def test_unknown_and_unobserved_symbols_are_refused_by_name():
    c = rc()
    with pytest.raises(CedarError, match="measure 'tpd': unknown node or device 'nix'"):
        M.resolve_measures(c, [M.parse_measure(".measure tran tpd when v(nix)=0.5")])
    with pytest.raises(CedarError, match="measure 'q': unknown node or device 'out,nix'"):
        M.resolve_measures(c, [M.vmax("q", ("out", "nix"))])
    with pytest.raises(CedarError, match="measure 'ic': unknown node or device 'c1.i'"):
        M.resolve_measures(c, [M.avg("ic", "c1.i")])
    c2 = Circuit()
    c2.V("vin", "in", 0, dc=1.0)
    c2.R("r1", "in", "out", 1e3)
    c2.C("c1", "out", 0, 1e-12)
    c2.observe_node("out")
    with pytest.raises(CedarError, match="measure 'a': node 'in' is not observed"):
        M.resolve_measures(c2, [M.avg("a", "in")])
    with pytest.raises(CedarError, match="measure 'a' is defined twice"):
        M.resolve_measures(c, [M.avg("a", "in"), M.rms("a", "out")])
    with pytest.raises(CedarError, match="measure 'ir': the current of resistor 'r1'"):
        M.resolve_measures(c, [M.vmax("ir", "r1.i")], with_sens=True)
    with pytest.raises(CedarError, match="edge must be"):
        M.event("out", 0.5, "up")
