"""Waveform measurements over a transient — the `.measure` cards of a SPICE deck and their constructors.

    when("t50", "q", 2.5, edge="rise")                     time of an event (threshold crossing)
    delay("tpd", event("clk", 2.5), event("q", 2.5))       trig event to targ event
    find_when("vx", "x", event("q", 2.5))                  another signal at the event
    find_at("v1n", "q", 1e-9)                              a signal at a time
    integ / avg / rms / vmin / vmax / pp ("iavg", "vvdd.i", frm=0.0, to=1e-7)
    parse_measure(".measure tran tpd trig v(clk) val=2.5 rise=1 targ v(q) val=2.5 rise=1")
    measure_cards(deck_text)                               every .measure / .meas card of a deck

A signal is a symbol as `sol[...]` takes it ("q", "node_q", "l1.i", "r1.v", "r1.i") or a pair (a, b) for v(a) - v(b).  Handed to
`tran(..., measures=[...])` / `tran_sens(..., measures=[...])` (also on a CircuitSweep) or to `Solution.measure`, every measure is
evaluated on the GPU for all samples at once (ch_result_measure / ch_measure_rows; definitions in DESIGN.md 2.7e).  Between saved rows
the signal is the run's own dense-output polynomial; on a `saveat` grid it is piecewise linear, as in ngspice's .meas — `sol(t)`
interpolates such a grid with PCHIP instead.  Pure Python: nothing here loads the GPU binding."""
import ctypes as C
import math
import re
from typing import NamedTuple

from .circuit import DEV_R, CedarError
from .solution import _resolve_sym, _split_sym
from .spice_expr import parse_number

KINDS = ("when", "delay", "find_when", "find_at", "integ", "avg", "rms", "min", "max", "pp")   # CH_MEAS_* of include/cedarhip.h, in order
EDGES = {"rise": 1, "fall": 2, "cross": 3}                                                      # CH_EDGE_*
LAST = -1                                                                                       # CH_MEAS_LAST
STATUS = {0: "ok", 1: "event not found", 2: "empty window", 3: "non-finite row", 4: "flat interpolant at the event"}


class ChMeasureSide(C.Structure):
    """ch_measure_side of include/cedarhip.h."""
    _fields_ = [("row_a", C.c_int32), ("row_b", C.c_int32), ("scale", C.c_double), ("level", C.c_double), ("edge", C.c_int32), ("count", C.c_int32),
                ("td", C.c_double)]


class ChMeasureSpec(C.Structure):
    """ch_measure_spec of include/cedarhip.h."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("s1", ChMeasureSide), ("s2", ChMeasureSide), ("at", C.c_double), ("frm", C.c_double),
                ("to", C.c_double)]


class Event(NamedTuple):
    """The n-th (or last) crossing of `level` by `sig` in direction `edge` at or after `td`."""
    sig: object
    level: float
    edge: str = "cross"
    n: int = 1
    td: float = -math.inf


class Measure(NamedTuple):
    name: str
    kind: str
    sig: object = None        # the signal measured (find_when, find_at, windows)
    trig: Event = None        # the event (when, find_when), the trig event (delay)
    targ: Event = None
    at: float = 0.0
    frm: float = -math.inf
    to: float = math.inf


def event(sig, level, edge="cross", n=1, td=None):
    """n: 1, 2, ... or "last"."""
    edge = str(edge).lower()
    if edge not in EDGES:
        raise CedarError("edge must be 'rise', 'fall' or 'cross', not %r" % (edge,))
    n = LAST if str(n).lower() == "last" else int(n)
    if n == 0 or n < LAST:
        raise CedarError("event count must be 1, 2, ... or 'last', not %r" % (n,))
    return Event(sig, float(level), edge, n, -math.inf if td is None else float(td))


def when(name, sig, level=None, edge="cross", n=1, td=None):
    """Time of an event: `when("t50", "q", 2.5, "rise")` or `when("t50", event("q", 2.5, "rise"))`."""
    return Measure(str(name), "when", trig=sig if isinstance(sig, Event) else event(sig, level, edge, n, td))


def delay(name, trig, targ):
    """t(targ event) - t(trig event); each an `event(...)`."""
    return Measure(str(name), "delay", trig=trig, targ=targ)


def find_when(name, sig, ev):
    return Measure(str(name), "find_when", sig=sig, trig=ev)


def find_at(name, sig, at):
    return Measure(str(name), "find_at", sig=sig, at=float(at))


def _window(kind):
    def make(name, sig, frm=None, to=None):
        return Measure(str(name), kind, sig=sig, frm=-math.inf if frm is None else float(frm), to=math.inf if to is None else float(to))
    make.__name__ = {"min": "vmin", "max": "vmax"}.get(kind, kind)
    make.__doc__ = "%s of a signal over [frm, to] clipped to the run (trapezoid rule on frm, the rows inside, to)." % kind.upper()
    return make


integ, avg, rms, vmin, vmax, pp = (_window(k) for k in ("integ", "avg", "rms", "min", "max", "pp"))


# ---- SPICE cards ------------------------------------------------------------------------------------------------------------------------
_SIG_RE = re.compile(r"^([vi])\(([^(),]+)(?:,([^(),]+))?\)$")


def _signal(tok, name):
    m = _SIG_RE.match(tok)
    if not m:
        raise CedarError(".measure %s: expected v(node), v(a,b) or i(source), got '%s'" % (name, tok))
    what, a, b = m.groups()
    if what == "i":
        if b:
            raise CedarError(".measure %s: i() takes one device, got '%s'" % (name, tok))
        return a + ".i"
    return (a, b) if b else a


def _number(tok, name, what):
    v = parse_number(tok)
    if v is None:
        raise CedarError(".measure %s: %s must be a number, got '%s'" % (name, what, tok))
    return float(v)


def _event_from(sig, level, opts, name):
    """opts: the tokens behind the signal and level of one event: RISE|FALL|CROSS=n|LAST, bare LAST, TD=."""
    edge, n, td = "cross", 1, None
    for tok in opts:
        key, _, val = tok.partition("=")
        if key in EDGES and val:
            edge, n = key, (LAST if val == "last" else int(_number(val, name, key.upper())))
        elif key == "last" and not val:
            n = LAST
        elif key == "td" and val:
            td = _number(val, name, "TD")
        else:
            raise CedarError(".measure %s: unknown option '%s'" % (name, tok))
    return event(sig, level, edge, n, td)


def _take_event(toks, name):
    """[signal, VAL=level | signal=level, options...] -> Event."""
    if not toks:
        raise CedarError(".measure %s: an event needs a signal and a level" % name)
    head, rest = toks[0], toks[1:]
    if ")=" in head:
        sig, _, lv = head.rpartition("=")
        return _event_from(_signal(sig, name), _number(lv, name, "the level"), rest, name)
    if not rest or not rest[0].startswith("val="):
        raise CedarError(".measure %s: an event needs VAL=level behind '%s'" % (name, head))
    return _event_from(_signal(head, name), _number(rest[0][4:], name, "VAL"), rest[1:], name)


def parse_measure(line):
    """One `.measure` / `.meas` card -> Measure.  Forms: TRIG sig VAL=l [RISE|FALL|CROSS=n|LAST] [TD=t] TARG sig VAL=l ...;
    WHEN sig=l ... (or sig VAL=l); FIND sig WHEN sig=l ...; FIND sig AT=t; AVG|RMS|MIN|MAX|PP|INTEG sig [FROM=a] [TO=b].  Signals are
    v(a), v(a,b), i(vsrc).  `PARAM=` expressions, DERIV and analyses other than TRAN are refused by name."""
    text = re.sub(r"\(\s*([^()]*?)\s*\)", lambda m: "(" + re.sub(r"\s+", "", m.group(1)) + ")", str(line).strip().lower())
    text = re.sub(r"\s*=\s*", "=", text)
    toks = text.split()
    if not toks or toks[0] not in (".measure", ".meas"):
        raise CedarError("not a .measure card: '%s'" % str(line).strip())
    if len(toks) < 4:
        raise CedarError("incomplete .measure card: '%s'" % str(line).strip())
    if toks[1] not in ("tran",):
        raise CedarError(".measure %s: only TRAN measurements are supported, not %s" % (toks[2], toks[1].upper()))
    name, what, rest = toks[2], toks[3], toks[4:]
    if what.startswith("param=") or what == "param":
        raise CedarError(".measure %s: PARAM= expressions over other measures are not supported" % name)
    if what in ("deriv", "derivative"):
        raise CedarError(".measure %s: DERIV is not supported" % name)
    if what == "trig":
        if "targ" not in rest:
            raise CedarError(".measure %s: TRIG without TARG" % name)
        k = rest.index("targ")
        return delay(name, _take_event(rest[:k], name), _take_event(rest[k + 1:], name))
    if what == "when":
        return when(name, _take_event(rest, name))
    if what == "find":
        if len(rest) >= 2 and rest[1] == "when":
            return find_when(name, _signal(rest[0], name), _take_event(rest[2:], name))
        if len(rest) == 2 and rest[1].startswith("at="):
            return find_at(name, _signal(rest[0], name), _number(rest[1][3:], name, "AT"))
        raise CedarError(".measure %s: FIND needs WHEN ... or AT=" % name)
    if what in ("avg", "rms", "min", "max", "pp", "integ", "integral"):
        if not rest:
            raise CedarError(".measure %s: %s needs a signal" % (name, what.upper()))
        frm = to = None
        for tok in rest[1:]:
            key, _, val = tok.partition("=")
            if key == "from" and val:
                frm = _number(val, name, "FROM")
            elif key == "to" and val:
                to = _number(val, name, "TO")
            else:
                raise CedarError(".measure %s: unknown option '%s'" % (name, tok))
        return {"avg": avg, "rms": rms, "min": vmin, "max": vmax, "pp": pp, "integ": integ, "integral": integ}[what](name, _signal(rest[0], name), frm, to)
    raise CedarError(".measure %s: unknown measurement '%s'" % (name, what.upper()))


def measure_cards(text):
    """The `.measure` / `.meas` cards of a deck (continuation lines joined), parsed.  `parse_spice` itself leaves these cards alone."""
    cards = []
    for raw in str(text).splitlines():
        ln = raw.split(";")[0].strip()
        if not ln or ln.startswith("*"):
            continue
        if ln.startswith("+") and cards and cards[-1] is not None:
            cards[-1] += " " + ln[1:].strip()
            continue
        cards.append(ln if ln.lower().split()[0] in (".measure", ".meas") else None)
    return [parse_measure(c) for c in cards if c is not None]


# ---- symbols -> rows --------------------------------------------------------------------------------------------------------------------
def _rows_of(ckt, sym, name, views, with_sens):
    """(row_a, row_b, scale) of a signal among the observables of `ckt`."""
    def row(key, what):
        if key not in ckt.obs:
            raise CedarError("measure '%s': %s is not observed" % (name, what))
        return ckt.obs.index(key)

    def diff(a, b, scale, what):
        if a == 0 and b == 0:
            raise CedarError("measure '%s': %s is ground on both sides" % (name, what))
        if a == 0:
            return row(("v", b), what), -1, -scale
        return row(("v", a), what), (row(("v", b), what) if b != 0 else -1), scale

    try:
        if isinstance(sym, (tuple, list)):
            (na, _, _), (nb, _, _) = _split_sym(ckt, sym[0]), _split_sym(ckt, sym[1])
            if na is None or nb is None:
                raise KeyError(sym)
            return diff(ckt._n(na), ckt._n(nb), 1.0, "v(%s,%s)" % tuple(sym))
        node, i, fld = _split_sym(ckt, sym)
        if node is None and fld == "i" and ckt.dev_kind[i] == DEV_R:
            if with_sens:
                raise CedarError("measure '%s': the current of resistor '%s' is v / R, and R may be a parameter: measure the voltage across it" % (name, ckt.dev_names[i]))
            rs = {float(v.dev_par[i][0]) for v in (views or [ckt])}
            if len(rs) != 1:
                raise CedarError("measure '%s': resistor '%s' differs between the samples: measure the voltage across it" % (name, ckt.dev_names[i]))
            return diff(ckt.dev_node[i][0], ckt.dev_node[i][1], 1.0 / rs.pop(), "'%s'" % sym)
        r = _resolve_sym(ckt, sym)
    except KeyError:
        raise CedarError("measure '%s': unknown node or device '%s'" % (name, sym if not isinstance(sym, (tuple, list)) else ",".join(map(str, sym)))) from None
    if r[0] == "v":
        return diff(r[1], 0, 1.0, "node '%s'" % sym)
    if r[0] == "dv":
        return diff(r[1], r[2], 1.0, "'%s'" % sym)
    return row(r, "the branch current of '%s'" % sym), -1, 1.0


def resolve_measures(ckt, measures, views=None, with_sens=False):
    """(names, ctypes array of ch_measure_spec) of `measures` against the observables of `ckt`.  Unknown or unobserved symbols and
    duplicate names raise a CedarError that names the measure."""
    measures = list(measures)
    names = [m.name for m in measures]
    for n in names:
        if names.count(n) > 1:
            raise CedarError("measure '%s' is defined twice" % n)
    arr = (ChMeasureSpec * max(1, len(measures)))()

    def fill(sd, sym, ev, name):
        sd.row_a, sd.row_b, sd.scale = _rows_of(ckt, sym, name, views, with_sens)
        sd.level, sd.edge, sd.count, sd.td = (ev.level, EDGES[ev.edge], ev.n, ev.td) if ev is not None else (0.0, EDGES["cross"], 1, -math.inf)

    for k, m in enumerate(measures):
        if not isinstance(m, Measure) or m.kind not in KINDS:
            raise CedarError("not a measure: %r (build one with when, delay, find_when, find_at, integ, avg, rms, vmin, vmax, pp or parse_measure)" % (m,))
        sp = arr[k]
        sp.kind, sp.at, sp.frm, sp.to = KINDS.index(m.kind), m.at, m.frm, m.to
        if m.kind in ("when", "delay", "find_when"):
            fill(sp.s1, m.trig.sig, m.trig, m.name)
            if m.kind == "delay":
                fill(sp.s2, m.targ.sig, m.targ, m.name)
            elif m.kind == "find_when":
                fill(sp.s2, m.sig, None, m.name)
            else:
                sp.s2.row_b = -1
        else:
            fill(sp.s1, m.sig, None, m.name)
            sp.s2.row_b = -1
    return names, arr
