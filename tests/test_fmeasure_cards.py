"""`.measure ac` / `.measure noise` cards, the constructors and the helpers' conventions (cedarsim.jl_amd/acmeasure.py) on the CPU: every
supported SPICE form, the refusals by name, `ac_measure_cards` skipping TRAN cards, and the symbols-to-rows step against a circuit's
MNA rows (no GPU: nothing here loads the engine)."""
import ctypes as C
import math

import numpy as np
import pytest

from cedarsim_jl_amd import Circuit, CedarError
from cedarsim_jl_amd import acmeasure as A
from cedarsim_jl_amd import measure as M


def rc():
    c = Circuit()
    c.V("vin", "in", 0, dc=0.0, ac=1.0)
    c.R("r1", "in", "out", 1e3)
    c.C("c1", "out", 0, 1e-12)
    return c


def test_when_and_find():
    assert A.parse_ac_measure(".measure ac fug when vdb(out)=0 fall=1") == A.fwhen("fug", A.db("out"), 0.0, "fall", 1)
    assert A.parse_ac_measure(".MEAS AC f1 WHEN VP( out ) VAL = -45 cross=last fd=1k") == A.fwhen("f1", A.phase("out"), -45.0, "cross", "last", 1e3)
    assert A.parse_ac_measure(".meas ac f1 when vm(out,in)=0.5 last td=10") == A.fwhen("f1", A.mag(("out", "in")), 0.5, "cross", "last", 10.0)
    assert A.parse_ac_measure(".meas ac pm find vp(out) when vdb(out)=0 fall=1") == A.ffind_when("pm", A.phase("out"), A.fevent(A.db("out"), 0.0, "fall"))
    assert A.parse_ac_measure(".meas ac a0 find vdb(out) at=1k") == A.ffind_at("a0", A.db("out"), 1e3)
    assert A.parse_ac_measure(".meas ac x find vr(out) at=1meg").sig == A.re("out") and A.parse_ac_measure(".meas ac x find vi(out) at=1").sig == A.im("out")
    assert A.parse_ac_measure(".meas ac x find v(out) at=1").sig == A.mag("out")                 # v() of an AC card is the magnitude
    assert A.parse_ac_measure(".meas ac x find idb(vin) at=1").sig == A.db("vin.i")
    assert A.parse_ac_measure(".meas ac x find vdb(out) at=1", xscale="lin").xscale == "lin"


@pytest.mark.parametrize("word, make", [("avg", A.favg), ("rms", A.frms), ("min", A.fmin), ("max", A.fmax), ("pp", A.fpp), ("integ", A.finteg), ("integral", A.finteg)])
def test_windows(word, make):
    assert A.parse_ac_measure(".measure ac x %s vdb(out) from=1k to=2meg" % word.upper()) == make("x", A.db("out"), 1e3, 2e6)
    m = A.parse_ac_measure(".measure noise x %s onoise" % word)
    assert m == make("x", A.Sig(None, "re")) and m.frm == -math.inf and m.to == math.inf


def test_noise_cards():
    assert A.parse_ac_measure(".meas noise vn2 integ onoise from=10 to=100k") == A.finteg("vn2", A.Sig(None, "re"), 10.0, 1e5)
    assert A.parse_ac_measure(".meas noise spot find onoise at=1k") == A.ffind_at("spot", A.Sig(None, "re"), 1e3)
    assert A.parse_ac_measure(".meas noise fc when onoise=1e-15 fall=1") == A.fwhen("fc", A.Sig(None, "re"), 1e-15, "fall", 1)
    with pytest.raises(CedarError, match="onoise"):
        A.parse_ac_measure(".meas noise x integ vdb(out)")
    with pytest.raises(CedarError, match="NOISE"):
        A.parse_ac_measure(".meas ac x integ onoise")


def test_cards_of_a_deck_skip_tran():
    deck = """* rc
vin in 0 dc 0 ac 1
r1 in out 1k
c1 out 0 1p
.ac dec 20 1k 1g
.measure tran tpd trig v(in) val=0.5 rise=1 targ v(out) val=0.5 rise=1
.measure ac f3db when vdb(out)=-3
+ fall=1   ; the corner
.meas noise vn2 integ onoise
.end
"""
    cards = A.ac_measure_cards(deck)
    assert [m.name for m in cards] == ["f3db", "vn2"] and cards[0] == A.fwhen("f3db", A.db("out"), -3.0, "fall", 1)
    assert [m.name for m in M.measure_cards(deck.replace(".measure ac", "* .measure ac").replace(".meas noise", "* .meas noise"))] == ["tpd"]
    with pytest.raises(CedarError, match="only TRAN"):        # the transient parser's own refusal stands
        M.parse_measure(".measure ac f3db when vdb(out)=-3")


@pytest.mark.parametrize("card, text", [
    (".measure tran t when v(out)=1", "only AC and NOISE"),
    (".measure dc t when v(out)=1", "only AC and NOISE"),
    (".measure ac t param='a/b'", "PARAM="),
    (".measure ac t deriv vdb(out) at=1k", "DERIV"),
    (".measure ac t trig vdb(out) val=0 rise=1 targ vdb(out) val=-3 fall=1", "TRIG / TARG"),
    (".measure ac t when out val=1", "expected vdb()"),
    (".measure ac t when vdb(out)=1 rise=0", "event count"),
    (".measure ac t when vdb(out)=1 sideways=1", "unknown option 'sideways=1'"),
    (".measure ac t find vdb(out)", "FIND needs"),
    (".measure ac t find idb(a,b) at=1", "takes one device"),
    (".measure ac t max vdb(out) from=x", "FROM must be a number"),
    (".measure ac t median vdb(out)", "unknown measurement 'MEDIAN'"),
    (".measure ac t", "incomplete"),
    ("vin in 0 1", "not a .measure card"),
])
def test_refusals_name_the_reason(card, text):
    with pytest.raises(CedarError) as e:
        A.parse_ac_measure(card)
    assert text in str(e.value), str(e.value)


def test_helper_conventions():
    """Each helper is one spec and an affine map of its value: the conventions its docstring states."""
    bw = A.bandwidth("bw", "out", ref_at=1e3)
    assert bw.kind == "when" and bw.ev == A.FEvent(A.db("out"), -A.DROP_3DB, "fall", 1, 1e3, 1e3) and (bw.gain, bw.offset) == (1.0, 0.0)
    assert A.bandwidth("bw", A.mag("out"), 1e3, drop_db=6.0).ev.sig == A.db("out") and A.bandwidth("bw", "out", 1e3, 6.0).ev.level == -6.0
    ug = A.unity_gain_freq("fug", A.db("out", scale=-1.0))
    assert ug.kind == "when" and ug.ev == A.FEvent(A.Sig("out", "db", -1.0), 0.0, "fall", 1, -math.inf, ug.ev.ref_at) and math.isnan(ug.ev.ref_at)
    pm = A.phase_margin("pm", "out")
    assert pm.kind == "find_when" and pm.sig == A.phase("out") and pm.ev.sig == A.db("out") and pm.ev.level == 0.0 and pm.ev.edge == "fall" and (pm.gain, pm.offset) == (1.0, 180.0)
    gm = A.gain_margin("gm", "out")
    assert gm.kind == "find_when" and gm.sig == A.db("out") and gm.ev.sig == A.phase("out") and gm.ev.level == -180.0 and gm.ev.edge == "fall" and (gm.gain, gm.offset) == (-1.0, 0.0)
    # the map is applied to values and sensitivities on the host; NaN stays NaN
    res = A.resolve_fmeasures([bw, pm, gm], A.mna_rows(rc()))
    val = np.array([[5.0, math.nan], [-120.0, math.nan], [-12.0, 3.0]])
    sens = np.ones((3, 2, 2))
    val, sens = res.apply(val, sens)
    assert val[0, 0] == 5.0 and val[1, 0] == 60.0 and val[2, 0] == 12.0 and val[2, 1] == -3.0 and np.isnan(val[:2, 1]).all()
    assert np.all(sens[:2] == 1.0) and np.all(sens[2] == -1.0)
    for doc in (A.bandwidth, A.unity_gain_freq, A.phase_margin, A.gain_margin):
        assert doc.__doc__ and ("Hz" in doc.__doc__ or "dB" in doc.__doc__ or "Degrees" in doc.__doc__)


def test_symbols_to_mna_rows():
    c = rc()
    i_out, i_in, i_vin = c.mna_index("v", "out"), c.mna_index("v", "in"), c.mna_index("i", "vin")
    ms = [A.fwhen("a", A.db("out"), -3.0, "fall", ref_at=1e3), A.ffind_when("b", A.phase(("out", "in"), scale=2.0), A.fevent(A.mag("vin.i"), 1e-4, "rise", "last", 5.0)),
          A.ffind_at("c", A.re("r1.v"), 1e6, xscale="lin"), A.finteg("d", A.im("node_out"), 1e3, 1e6), A.fmax("e", A.db10(("0", "out")))]
    res = A.resolve_fmeasures(ms, A.mna_rows(c))
    assert res.names == list("abcde") and C.sizeof(A.ChFMeasureSpec) == 144 and C.sizeof(A.ChFMeasureSide) == 56
    s = res.specs
    assert (s[0].kind, s[0].xscale, s[0].s1.row_a, s[0].s1.row_b, s[0].s1.sig, s[0].s1.edge, s[0].s1.count, s[0].s1.level, s[0].s1.ref_at) == (0, 1, i_out, -1, 3, 2, 1, -3.0, 1e3)
    assert (s[1].kind, s[1].s1.row_a, s[1].s1.sig, s[1].s1.count, s[1].s1.fd, s[1].s2.row_a, s[1].s2.row_b, s[1].s2.scale, s[1].s2.sig) == (1, i_vin, 2, -1, 5.0, i_out, i_in, 2.0, 5)
    assert math.isnan(s[1].s1.ref_at)
    assert (s[2].kind, s[2].xscale, s[2].at, s[2].s1.row_a, s[2].s1.row_b, s[2].s1.sig) == (2, 0, 1e6, i_in, i_out, 0)        # r1.v = v(in) - v(out)
    assert (s[3].kind, s[3].frm, s[3].to, s[3].s1.sig) == (3, 1e3, 1e6, 1) and (s[4].kind, s[4].s1.row_a, s[4].s1.scale, s[4].s1.sig) == (7, i_out, -1.0, 4)
    assert s[4].frm == -math.inf and s[4].to == math.inf
    for bad, text in (([A.ffind_at("x", A.db("nosuch"), 1.0)], "unknown node or device 'nosuch'"), ([ms[0], ms[0]], "defined twice"),
                      ([A.ffind_at("x", A.db(("0", "0")), 1.0)], "ground on both sides"), ([A.ffind_at("x", A.Sig(None, "re"), 1.0)], "noise analysis"),
                      ([M.when("t", "out", 0.5)], "not a frequency-domain measure"), ([A.ffind_at("x", A.Sig("out", "loud"), 1.0)], "not a signal")):
        with pytest.raises(CedarError) as e:
            A.resolve_fmeasures(bad, A.mna_rows(c))
        assert text in str(e.value), str(e.value)
    with pytest.raises(CedarError, match="xscale"):
        A.ffind_at("x", "out", 1.0, xscale="octave")
    with pytest.raises(CedarError, match="edge"):
        A.fevent("out", 0.0, "up")
    assert set(A.STATUS) == {0, 1, 2, 3, 4, 5}
