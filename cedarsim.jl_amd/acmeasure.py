"""Frequency-domain measurements over an AC or noise analysis — the `.measure ac` / `.measure noise` cards of a SPICE deck and
their constructors.

    fwhen("f3db", db("out"), -3.0103, edge="fall", ref_at=1e3)   frequency of an event (the level may be relative to the signal at ref_at)
    ffind_when("ph_ug", phase("out"), fevent(db("out"), 0.0, "fall"))   another signal at the event's frequency
    ffind_at("a0", db("out"), 10.0)                              a signal at a frequency
    fmin / fmax / fpp / finteg / favg / frms ("vn2", re("out"), frm=10.0, to=1e5)
    bandwidth("bw", "out", ref_at=1e3)   unity_gain_freq("fug", "out")   phase_margin("pm", "out")   gain_margin("gm", "out")
    parse_ac_measure(".measure ac f3db when vdb(out)=-3 fall=1")
    ac_measure_cards(deck_text)                                  every .measure ac / noise card of a deck (TRAN cards are skipped)

A signal is a real function of the complex response H of a symbol as `ACSolution.freqresp` takes it ("out", "node_out", "l1.i",
"r1.v") or of a pair (a, b) for v(a) - v(b): `re`, `im`, `mag`, `db` = 20 log10 |H|, `phase` in degrees, unwrapped along the grid
from its first row as `ACSolution.bode` gives it, and `db10` = 10 log10 re for a PSD row.  `scale=` multiplies H first (-1 turns an
inverting stage's response into a loop gain).  Between the rows of the frequency grid a signal is the line over log10 f
(`xscale="log"`, the default) or over f (`"lin"`), as in ngspice's .meas ac; windows integrate by the trapezoid rule in linear f.

Handed to `ac_measure(circuit, measures, freqs_hz, params=())` (also on a CircuitSweep) every measure is evaluated on the GPU for all
samples at once where the AC solve left its result (ch_ac_measure; definitions in DESIGN.md 2.7g), with its exact derivatives with
respect to `params`; `NoiseSolution.measure` / `NoiseSensSolution.measure` apply them to PSD rows (ch_freq_measure_rows).  Pure Python:
nothing here loads the GPU binding."""
import ctypes as C
import math
import re as _re
from typing import NamedTuple

from .circuit import CedarError
from .measure import EDGES, LAST, STATUS as _TRAN_STATUS
from .solution import _resolve_sym, _split_sym
from .spice_expr import parse_number

KINDS = ("when", "find_when", "find_at", "integ", "avg", "rms", "min", "max", "pp")   # CH_FMEAS_* of include/cedarhip.h, in order
SIGNALS = ("re", "im", "mag", "db", "db10", "phase")                                   # CH_FSIG_*
XSCALES = ("lin", "log")                                                               # CH_FX_*
STATUS = {**_TRAN_STATUS, 3: "non-finite signal", 5: "no operating point"}
DROP_3DB = 3.0103   # 20 log10 sqrt 2, to the digits decks use


class ChFMeasureSide(C.Structure):
    """ch_fmeasure_side of include/cedarhip.h."""
    _fields_ = [("row_a", C.c_int32), ("row_b", C.c_int32), ("scale", C.c_double), ("sig", C.c_int32), ("edge", C.c_int32), ("level", C.c_double),
                ("ref_at", C.c_double), ("count", C.c_int32), ("reserved", C.c_int32), ("fd", C.c_double)]


class ChFMeasureSpec(C.Structure):
    """ch_fmeasure_spec of include/cedarhip.h."""
    _fields_ = [("kind", C.c_int32), ("xscale", C.c_int32), ("s1", ChFMeasureSide), ("s2", ChFMeasureSide), ("at", C.c_double), ("frm", C.c_double),
                ("to", C.c_double)]


class Sig(NamedTuple):
    """A real signal `what` of the complex response of `sym`, H multiplied by `scale` first.  sym None: the output of a noise analysis."""
    sym: object
    what: str
    scale: float = 1.0


def _sig(what):
    def make(sym, scale=1.0):
        if isinstance(sym, Sig):
            return Sig(sym.sym, what, sym.scale * float(scale))
        return Sig(sym, what, float(scale))
    make.__name__ = what
    make.__doc__ = "The signal %s of a symbol's response (see the module text)." % what
    return make


re, im, mag, db, db10, phase = (_sig(k) for k in SIGNALS)


def _as_sig(s, default):
    return s if isinstance(s, Sig) else Sig(s, default)


class FEvent(NamedTuple):
    """The n-th (or last) crossing of the level by `sig` in direction `edge` at or above `fd`.  The level is `level`, or `level` plus
    the signal's own interpolated value at `ref_at` when that is given."""
    sig: Sig
    level: float
    edge: str = "cross"
    n: int = 1
    fd: float = -math.inf
    ref_at: float = math.nan


class FMeasure(NamedTuple):
    name: str
    kind: str
    sig: Sig = None          # the signal measured (find_when, find_at, windows)
    ev: FEvent = None        # the event (when, find_when)
    at: float = 1.0
    frm: float = -math.inf
    to: float = math.inf
    xscale: str = "log"
    gain: float = 1.0        # the value handed out is gain * value + offset (the helpers' conventions), its sensitivities gain * d value
    offset: float = 0.0


def _xscale(x):
    x = str(x).lower()
    if x not in XSCALES:
        raise CedarError("xscale must be 'log' or 'lin', not %r" % (x,))
    return x


def fevent(sig, level, edge="cross", n=1, fd=None, ref_at=None):
    """n: 1, 2, ... or "last".  sig: a signal (`db("out")`, ...); a bare symbol is its `db`."""
    edge = str(edge).lower()
    if edge not in EDGES:
        raise CedarError("edge must be 'rise', 'fall' or 'cross', not %r" % (edge,))
    n = LAST if str(n).lower() == "last" else int(n)
    if n == 0 or n < LAST:
        raise CedarError("event count must be 1, 2, ... or 'last', not %r" % (n,))
    return FEvent(_as_sig(sig, "db"), float(level), edge, n, -math.inf if fd is None else float(fd), math.nan if ref_at is None else float(ref_at))


def fwhen(name, sig, level=None, edge="cross", n=1, fd=None, ref_at=None, xscale="log"):
    """Frequency (Hz) of an event: `fwhen("fug", db("out"), 0.0, "fall")` or `fwhen("fug", fevent(db("out"), 0.0, "fall"))`."""
    return FMeasure(str(name), "when", ev=sig if isinstance(sig, FEvent) else fevent(sig, level, edge, n, fd, ref_at), xscale=_xscale(xscale))


def ffind_when(name, sig, ev, xscale="log"):
    """The signal `sig` at the frequency of the event `ev` (an `fevent(...)`)."""
    return FMeasure(str(name), "find_when", sig=_as_sig(sig, "db"), ev=ev, xscale=_xscale(xscale))


def ffind_at(name, sig, at, xscale="log"):
    return FMeasure(str(name), "find_at", sig=_as_sig(sig, "db"), at=float(at), xscale=_xscale(xscale))


def _window(kind):
    def make(name, sig, frm=None, to=None, xscale="log"):
        return FMeasure(str(name), kind, sig=_as_sig(sig, "re"), frm=-math.inf if frm is None else float(frm), to=math.inf if to is None else float(to),
                        xscale=_xscale(xscale))
    make.__name__ = "f" + kind
    make.__doc__ = ("%s of a signal over [frm, to] Hz clipped to the grid: the point set is frm, the rows strictly inside and to; sums are the "
                    "trapezoid rule in linear f.  A bare symbol is its `re` (a PSD row)." % kind.upper())
    return make


finteg, favg, frms, fmin, fmax, fpp = (_window(k) for k in ("integ", "avg", "rms", "min", "max", "pp"))


# ---- helpers: one spec and an affine map of its value -------------------------------------------------------------------------------------
def bandwidth(name, sig, ref_at, drop_db=DROP_3DB, xscale="log"):
    """The first frequency at which the gain has fallen `drop_db` dB below its own value at `ref_at` Hz (each sample's own reference):
    the first FALL of 20 log10 |H| through `g(ref_at) - drop_db`, counted from `ref_at` on.  Hz."""
    return FMeasure(str(name), "when", ev=fevent(db(sig), -float(drop_db), "fall", 1, float(ref_at), float(ref_at)), xscale=_xscale(xscale))


def unity_gain_freq(name, sig, xscale="log"):
    """The first frequency at which 20 log10 |H| falls through 0 dB.  Hz."""
    return FMeasure(str(name), "when", ev=fevent(db(sig), 0.0, "fall", 1), xscale=_xscale(xscale))


def phase_margin(name, sig, xscale="log"):
    """180 degrees plus the phase of H at its unity-gain frequency (the first fall of |H| through 0 dB).  The phase is unwrapped from
    the first row of the grid, so H is the loop gain with the sign that makes its low-frequency phase 0 (`db(sym, scale=-1)` flips
    an inverting stage); the grid has to start below the first pole.  Degrees."""
    return FMeasure(str(name), "find_when", sig=phase(sig), ev=fevent(db(sig), 0.0, "fall", 1), xscale=_xscale(xscale), offset=180.0)


def gain_margin(name, sig, xscale="log"):
    """Minus the gain in dB where the phase of H (unwrapped from the first row, as for `phase_margin`) first falls through -180
    degrees: positive for a stable loop.  dB."""
    return FMeasure(str(name), "find_when", sig=db(sig), ev=fevent(phase(sig), -180.0, "fall", 1), xscale=_xscale(xscale), gain=-1.0)


# ---- SPICE cards --------------------------------------------------------------------------------------------------------------------------
_SIG_RE = _re.compile(r"^(vdb|vm|vp|vr|vi|v|idb|im|ip|ir|ii|i)\(([^(),]+)(?:,([^(),]+))?\)$")
_WHAT = {"db": "db", "m": "mag", "p": "phase", "r": "re", "i": "im", "": "mag"}


def _signal(tok, name, noise):
    if tok in ("onoise", "onoise_spectrum"):
        if not noise:
            raise CedarError(".measure %s: onoise belongs to a NOISE measurement" % name)
        return Sig(None, "re")
    m = _SIG_RE.match(tok)
    if not m or noise:
        raise CedarError(".measure %s: expected %s, got '%s'" % (name, "onoise" if noise else "vdb(), vm(), vp(), vr(), vi() of a node or a pair", tok))
    fn, a, b = m.groups()
    what = _WHAT[fn[1:]]
    if fn[0] == "i":
        if b:
            raise CedarError(".measure %s: %s() takes one device, got '%s'" % (name, fn, tok))
        return Sig(a + ".i", what)
    return Sig((a, b) if b else a, what)


def _number(tok, name, what):
    v = parse_number(tok)
    if v is None:
        raise CedarError(".measure %s: %s must be a number, got '%s'" % (name, what, tok))
    return float(v)


def _take_event(toks, name, noise):
    """[signal, VAL=level | signal=level, RISE|FALL|CROSS=n|LAST, bare LAST, TD= | FD=] -> FEvent."""
    if not toks:
        raise CedarError(".measure %s: an event needs a signal and a level" % name)
    head, rest = toks[0], toks[1:]
    if ")=" in head or (noise and "=" in head):
        sig, _, lv = head.rpartition("=")
        level = _number(lv, name, "the level")
    else:
        if not rest or not rest[0].startswith("val="):
            raise CedarError(".measure %s: an event needs VAL=level behind '%s'" % (name, head))
        sig, level, rest = head, _number(rest[0][4:], name, "VAL"), rest[1:]
    edge, n, fd = "cross", 1, None
    for tok in rest:
        key, _, val = tok.partition("=")
        if key in EDGES and val:
            edge, n = key, (LAST if val == "last" else int(_number(val, name, key.upper())))
        elif key == "last" and not val:
            n = LAST
        elif key in ("td", "fd") and val:
            fd = _number(val, name, key.upper())
        else:
            raise CedarError(".measure %s: unknown option '%s'" % (name, tok))
    return fevent(_signal(sig, name, noise), level, edge, n, fd)


def parse_ac_measure(line, xscale="log"):
    """One `.measure ac` / `.measure noise` card -> FMeasure.  Forms: WHEN sig=l [RISE|FALL|CROSS=n|LAST] [FD=f] (or sig VAL=l);
    FIND sig WHEN sig=l ...; FIND sig AT=f; MIN|MAX|PP|INTEG|AVG|RMS sig [FROM=a] [TO=b].  AC signals are vdb(), vm(), vp() (degrees,
    unwrapped), vr(), vi() of a node or a pair, and the same with i for a branch current; v() is vm().  A NOISE card reads `onoise`,
    here the output PSD itself (V^2/Hz: INTEG gives V^2), of the output the analysis is asked for.  TRIG / TARG, `PARAM=`, DERIV and
    other analyses are refused by name."""
    text = _re.sub(r"\(\s*([^()]*?)\s*\)", lambda m: "(" + _re.sub(r"\s+", "", m.group(1)) + ")", str(line).strip().lower())
    text = _re.sub(r"\s*=\s*", "=", text)
    toks = text.split()
    if not toks or toks[0] not in (".measure", ".meas"):
        raise CedarError("not a .measure card: '%s'" % str(line).strip())
    if len(toks) < 4:
        raise CedarError("incomplete .measure card: '%s'" % str(line).strip())
    if toks[1] not in ("ac", "noise"):
        raise CedarError(".measure %s: only AC and NOISE measurements are read here, not %s (parse_measure reads TRAN)" % (toks[2], toks[1].upper()))
    noise = toks[1] == "noise"
    name, what, rest = toks[2], toks[3], toks[4:]
    if what.startswith("param=") or what == "param":
        raise CedarError(".measure %s: PARAM= expressions over other measures are not supported" % name)
    if what in ("deriv", "derivative"):
        raise CedarError(".measure %s: DERIV is not supported" % name)
    if what in ("trig", "targ"):
        raise CedarError(".measure %s: TRIG / TARG is a transient measurement; use WHEN or FIND ... WHEN" % name)
    if what == "when":
        return fwhen(name, _take_event(rest, name, noise), xscale=xscale)
    if what == "find":
        if len(rest) >= 2 and rest[1] == "when":
            return ffind_when(name, _signal(rest[0], name, noise), _take_event(rest[2:], name, noise), xscale)
        if len(rest) == 2 and rest[1].startswith("at="):
            return ffind_at(name, _signal(rest[0], name, noise), _number(rest[1][3:], name, "AT"), xscale)
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
        return {"avg": favg, "rms": frms, "min": fmin, "max": fmax, "pp": fpp, "integ": finteg, "integral": finteg}[what](name, _signal(rest[0], name, noise), frm, to, xscale)
    raise CedarError(".measure %s: unknown measurement '%s'" % (name, what.upper()))


def ac_measure_cards(text, xscale="log"):
    """The `.measure ac` / `.measure noise` cards of a deck (continuation lines joined), parsed; TRAN cards are skipped
    (`measure_cards` reads those)."""
    cards = []
    for raw in str(text).splitlines():
        ln = raw.split(";")[0].strip()
        if not ln or ln.startswith("*"):
            continue
        if ln.startswith("+") and cards and cards[-1] is not None:
            cards[-1] += " " + ln[1:].strip()
            continue
        cards.append(ln if ln.lower().split()[0] in (".measure", ".meas") else None)
    out = []
    for c in cards:
        if c is None:
            continue
        w = c.lower().split()
        if len(w) > 1 and w[1] == "tran":
            continue
        out.append(parse_ac_measure(c, xscale))
    return out


# ---- symbols -> rows ------------------------------------------------------------------------------------------------------------------------
def mna_rows(ckt):
    """`row_of(sym, name) -> (row_a, row_b, scale)` among the MNA rows of `ckt` (what ch_ac_measure reads)."""
    def node_pair(a, b, what, name):
        if a == 0 and b == 0:
            raise CedarError("measure '%s': %s is ground on both sides" % (name, what))
        return (b - 1, -1, -1.0) if a == 0 else (a - 1, b - 1 if b != 0 else -1, 1.0)

    def row_of(sym, name):
        try:
            if sym is None:
                raise CedarError("measure '%s': onoise belongs to a noise analysis" % name)
            if isinstance(sym, (tuple, list)):
                (na, _, _), (nb, _, _) = _split_sym(ckt, sym[0]), _split_sym(ckt, sym[1])
                if na is None or nb is None:
                    raise KeyError(sym)
                return node_pair(ckt._n(na), ckt._n(nb), "v(%s,%s)" % tuple(sym), name)
            r = _resolve_sym(ckt, sym)
        except KeyError:
            raise CedarError("measure '%s': unknown node or device '%s'" % (name, sym if not isinstance(sym, (tuple, list)) else ",".join(map(str, sym)))) from None
        if r[0] == "v":
            return node_pair(r[1], 0, "node '%s'" % sym, name)
        if r[0] == "dv":
            return node_pair(r[1], r[2], "'%s'" % sym, name)
        return ckt.mna_index("i", ckt.dev_names[r[1]]), -1, 1.0
    return row_of


NET_KINDS = "syz"   # the kinds of a network analysis in the order of their rows: kind * P^2 + j * P + k


def net_rows(n_ports):
    """`row_of(sym, name) -> (row_a, row_b, scale)` among the rows of a network analysis of `n_ports` ports (what ch_net_params reads):
    the reserved symbols "s21", "y11", "z12" — a kind letter and two digits 1 .. P, the response at the first port to the second;
    upper or lower case."""
    P = int(n_ports)

    def row_of(sym, name):
        t = sym.lower() if isinstance(sym, str) else ""
        if len(t) == 3 and t[0] in NET_KINDS and t[1:].isdigit():
            j, k = int(t[1]), int(t[2])
            if 1 <= j <= P and 1 <= k <= P:
                return NET_KINDS.index(t[0]) * P * P + (j - 1) * P + (k - 1), -1, 1.0
            raise CedarError("measure '%s': %r names a port outside 1 .. %d" % (name, sym, P))
        raise CedarError("measure '%s': a network-parameter measure reads a row such as \"s21\", \"y11\" or \"z12\", not %r" % (name, sym))
    return row_of


class Resolved(NamedTuple):
    names: list
    specs: object        # ctypes array of ch_fmeasure_spec
    gain: list           # per measure: the affine map of the helpers
    offset: list

    def apply(self, val, sens):
        """The helpers' affine maps on value[n_meas][S] and sens[n_meas][n_par][S] (in place; NaN stays NaN)."""
        for k, (g, o) in enumerate(zip(self.gain, self.offset)):
            if g != 1.0 or o != 0.0:
                val[k] = g * val[k] + o
                if sens is not None:
                    sens[k] *= g
        return val, sens


def resolve_fmeasures(measures, row_of):
    """`Resolved` of `measures` against the rows `row_of(sym, name)` names.  Unknown symbols and duplicate names raise a CedarError that
    names the measure."""
    measures = list(measures)
    names = [getattr(m, "name", None) for m in measures]
    for n in names:
        if n is not None and names.count(n) > 1:
            raise CedarError("measure '%s' is defined twice" % n)
    arr = (ChFMeasureSpec * max(1, len(measures)))()

    def fill(sd, sig, ev, name):
        if not isinstance(sig, Sig) or sig.what not in SIGNALS:
            raise CedarError("measure '%s': not a signal: %r (build one with db, mag, phase, re, im or db10)" % (name, sig))
        a, b, sc = row_of(sig.sym, name)
        sd.row_a, sd.row_b, sd.scale, sd.sig = a, b, sc * sig.scale, SIGNALS.index(sig.what)
        sd.level, sd.edge, sd.count, sd.fd, sd.ref_at = ((ev.level, EDGES[ev.edge], ev.n, ev.fd, ev.ref_at) if ev is not None
                                                         else (0.0, EDGES["cross"], 1, -math.inf, math.nan))

    for k, m in enumerate(measures):
        if not isinstance(m, FMeasure) or m.kind not in KINDS:
            raise CedarError("not a frequency-domain measure: %r (build one with fwhen, ffind_when, ffind_at, finteg, favg, frms, fmin, fmax, fpp, "
                             "bandwidth, unity_gain_freq, phase_margin, gain_margin or parse_ac_measure)" % (m,))
        sp = arr[k]
        sp.kind, sp.xscale, sp.at, sp.frm, sp.to = KINDS.index(m.kind), XSCALES.index(m.xscale), m.at, m.frm, m.to
        if m.kind in ("when", "find_when"):
            fill(sp.s1, m.ev.sig, m.ev, m.name)
            fill(sp.s2, m.sig if m.kind == "find_when" else m.ev.sig, None, m.name)
        else:
            fill(sp.s1, m.sig, None, m.name)
            fill(sp.s2, m.sig, None, m.name)
    return Resolved(names, arr, [m.gain for m in measures], [m.offset for m in measures])
