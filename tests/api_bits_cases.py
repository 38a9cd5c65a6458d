"""Cases, the stand-in engine and the one recorder shared by tests/test_api_layer_bits.py, tests/test_gpu_api_bits.py and
tests/golden/make_api_bits.py: everything the user-facing analyses (dc, tran, ac, noise, dc_sens, ac_sens, CircuitSweep and the solution
classes) do around the engine calls.

  CPU_CASES   the whole layer against `StandIn`, a class with EngineCircuit's methods whose arrays are a fixed function of their
              indices (no two entries equal) and which appends every call to a trace: the options read back out of the ctypes
              structs (x0 and its contents included), slot ids, values, the circuit's slot count at construction, small_signal.
  GPU_CASES   the same calls end to end on the smallest circuits that reach each path.

A case fills a `Rec`: name -> array (numbers, or a string for a retcode, an exception's type and text, a trace).  Only public names
are used, and the engine names to replace are found by walking `sys.modules`, so the module runs unchanged on any layout of the layer."""
import contextlib
import json
import sys
import threading
import warnings

import numpy as np

from cedarsim_jl_amd import (PWL, Circuit, CircuitSweep, Sweep, ac, ac_sens, acdec, dc, dc_sens, mag_phase_sens, noise, parse_spice, sens_opts,
                             tran)

TWO_PI = 2.0 * np.pi
W5 = TWO_PI * np.array([1e3, 1e4, 1e5, 1e6, 1e7])      # 5 frequencies as rad/s
W3 = TWO_PI * np.array([2e3, 2e5, 2e7])


# ---- circuits ------------------------------------------------------------------------------------------------------------------
def divider(r1=1e3, r2=2e3, c1=1e-9):
    """R-R-C divider; the source steps from 1.5 V to 0.5 V at 100 ns (time constant (r1 || r2) c1 = 0.67 us at the defaults)."""
    c = Circuit()
    c.V("v1", "in", 0, dc=1.5, tran=PWL([0.0, 1e-7, 1.1e-7, 1.0], [1.5, 1.5, 0.5, 0.5]))
    c.R("r1", "in", "out", r1)
    c.R("r2", "out", 0, r2)
    c.C("c1", "out", 0, c1)
    return c


def rlc(r1=50.0, l1=1e-6, c1=1e-9):
    """Series R-L-C with an AC source: an inductor branch current."""
    c = Circuit()
    c.V("v1", "in", 0, dc=1.0, ac=1.0)
    c.R("r1", "in", "a", r1)
    c.L("l1", "a", "out", l1)
    c.C("c1", "out", 0, c1)
    return c


def meter(r1=1e3, r2=3e3):
    """A 0 V source in series: `vs.v` is a difference of two nodes and `vs.i` a branch current."""
    c = Circuit()
    c.V("v1", "in", 0, dc=2.0, ac=1.0)
    c.R("r1", "in", "a", r1)
    c.V("vs", "a", "b", dc=0.0)
    c.R("r2", "b", 0, r2)
    c.C("c1", "b", 0, 1e-9)
    return c


NETLIST = """* divider with a .TRAN
V1 in 0 1.5
R1 in out 1k
R2 out 0 2k
C1 out 0 1n
.TRAN 1e-8 2e-6
.END
"""

SYMS = {
    "divider": ["node_out", "out", "in", "0", "gnd", "r1.v", "r1.i", "r2.i", "c1.v", "c1.i", "v1.v", "v1.i", "nosuch", "r9.i", "r1.q"],
    "rlc": ["node_out", "a", "0", "r1.v", "r1.i", "l1.v", "l1.i", "c1.i", "v1.i", "nosuch"],
    "meter": ["node_b", "a", "gnd", "vs.v", "vs.i", "v1.i", "r2.v", "r2.i", "c1.i", "nosuch.i"],
}


# ---- recording -----------------------------------------------------------------------------------------------------------------
class Rec(dict):
    """name -> array.  `floats=False` leaves the floating-point (timing) fields of a stats record out."""

    def __init__(self, floats):
        super().__init__()
        self.floats = floats

    def put(self, key, value):
        a = np.array(value) if isinstance(value, str) else np.asarray(value)
        assert a.dtype.kind in "fiucUb" and key not in self, (key, a.dtype)
        self[key] = a

    def do(self, key, fn):
        """The value of fn(), or the type and text of what it raises."""
        try:
            value = fn()
        except Exception as e:  # noqa: BLE001
            value = "%s: %s" % (type(e).__name__, e)
        if isinstance(value, tuple):
            for k, v in enumerate(value):
                self.put("%s/%d" % (key, k), v)
        else:
            self.put(key, value)

    def stats(self, key, st):
        if not isinstance(st, dict):
            return self.put(key, "stats: %r" % (st,))
        names = []
        for k in sorted(st):
            v = st[k]
            if k == "device_rows":
                continue
            if k == "dense_points":
                self.put("%s/dense_points" % key, "None" if v is None else np.asarray(v))
            elif isinstance(v, (int, np.integer)):
                names.append(k)
                self.put("%s/%s" % (key, k), int(v))
            elif self.floats:
                names.append(k)
                self.put("%s/%s" % (key, k), float(v))
        self.put("%s/names" % key, ",".join(names))

    def solution(self, key, sol, syms):
        self.put(key + "/t", sol.t)
        for s in syms:
            self.do("%s/[%s]" % (key, s), lambda: sol[s])
        self.put(key + "/x_final", "None" if sol.x_final is None else sol.x_final)
        self.put(key + "/rc", sol.rc)
        self.put(key + "/retcode", sol.retcode)
        self.stats(key + "/stats", sol.stats)
        self.put(key + "/params", json.dumps(sorted(sol.params.items())))
        self.put(key + "/dev_par", np.array(sol.circuit.dev_par, float))
        self.put(key + "/name_map", json.dumps(sorted(sol.default_name_map().items())))

    def sens(self, key, s, syms, pars):
        self.put(key + "/sens", s.sens)
        self.put(key + "/rc", s.rc)
        self.put(key + "/retcode", s.retcode)
        self.put(key + "/params", json.dumps([list(p) if isinstance(p, (tuple, list)) else p for p in s.params]))
        for sym in syms:
            for p in pars:
                self.do("%s/[%s,%s]" % (key, sym, p), lambda: s[sym, p])


def identical(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the stand-in engine ---------------------------------------------------------------------------------------------------------
class StandInContext:
    def __init__(self, device_id=0):
        self.device_id = device_id

    def last_error(self):
        return "stand-in error text of device %d" % self.device_id

    def va_opvars(self, module_id, par_and_given, v_nodes, temperature_k=300.15, gmin=1e-12):
        return {"module": float(module_id), "par": [float(x) for x in par_and_given], "v": [float(x) for x in v_nodes],
                "temperature_k": float(temperature_k), "gmin": float(gmin)}


_BOX = None


class Box:
    """What one `standin()` block shares: the plan (what the engine is to report) and the engines made, in order."""

    def __init__(self, plan):
        self.plan, self.engines, self.lock, self.default = dict(plan or {}), [], threading.Lock(), StandInContext(0)

    def trace(self):
        """Every engine's calls as JSON.  Engines made by worker threads (sweep groups) are ordered by their own records (which
        hold the samples' values), not by which thread came first."""
        logs = [e.log for e in self.engines]
        if any(e.thread != threading.main_thread().ident for e in self.engines):
            logs.sort(key=json.dumps)
        return json.dumps(logs)


def _floats(a):
    return [float(x) for x in np.asarray(a, float).reshape(-1)]


def _dc_record(o, n):
    x0 = _floats(np.ctypeslib.as_array(o.x0, (n,))) if o.x0 else None
    return {"abstol": o.abstol, "maxiters": o.maxiters, "n_restarts": o.n_restarts, "seed": o.seed, "tran_mode": o.tran_mode, "dv_max": o.dv_max,
            "x0": x0}


def _grid(shape, salt):
    """An array whose entries are all different and say where they sit."""
    return salt + 1e-3 * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


class StandIn:
    """EngineCircuit's methods without a library: see the module text."""

    def __init__(self, circuit, ctx=None, small_signal=False):
        self.ctx = ctx or _BOX.default
        self.circuit, self.n_mna, self.n_samples = circuit, circuit.n_mna, 1
        self.log, self.thread, self.calls = [], threading.get_ident(), 0
        circuit.to_desc(small_signal=small_signal)       # what the engine reads at construction must be buildable
        self._say("init", n_slots=len(circuit.slots), slots=[list(s) for s in circuit.slots], small_signal=bool(small_signal), n_mna=self.n_mna,
                  obs=[list(o) for o in circuit.obs], default_ctx=self.ctx is _BOX.default, device_id=self.ctx.device_id)
        with _BOX.lock:
            _BOX.engines.append(self)

    def _say(self, method, **kw):
        self.log.append(dict(method=method, **kw))

    def _stats(self, **extra):
        self.calls += 1
        st = {"nf": 3 * self.calls, "nnonliniter": 7 * self.calls, "nrestarts": self.calls, "naccept": 11, "stepper": 2, "stepper_mode": 1,
              "wall_seconds": 0.125 * self.calls, "dc_seconds": 0.0625}
        st.update(extra)
        return st

    def _outcome(self, method):
        """(rc, status[S]) as the plan asks: {"fail": {method: (rc, bad samples or "all")}, "only_S": n}."""
        S = self.n_samples
        status = np.zeros(S, np.int32)
        want = _BOX.plan.get("fail", {}).get(method)
        if want is None or _BOX.plan.get("only_S", S) != S:
            return 0, status
        rc, bad = want
        status[list(range(S)) if bad == "all" else [s for s in bad if s < S]] = rc
        return rc, status

    def _eliminate(self, a):
        """NaN in the MNA rows (last axis) of the branches the plan calls eliminated."""
        for name in _BOX.plan.get("eliminated", ()):
            a[..., self.circuit.mna_index("i", name)] = np.nan
        return a

    def set_samples(self, n):
        self._say("set_samples", n=int(n))
        self.n_samples = int(n)

    def set_params(self, slot_ids, values, lo=0, hi=None):
        v = np.asarray(values, float)
        self._say("set_params", slot_ids=[int(i) for i in slot_ids], shape=list(v.shape), values=_floats(v), lo=lo, hi=hi)

    def dc(self, opts=None, check=False):
        S, n = self.n_samples, self.n_mna
        self._say("dc", opts=None if opts is None else _dc_record(opts, S * n), check=bool(check))
        rc, status = self._outcome("dc")
        return rc, self._eliminate(_grid((S, n), 1.0)), status, self._stats()

    def tran(self, t0, t1, opts=None):
        S, n, nobs = self.n_samples, self.n_mna, len(self.circuit.obs)
        o = opts
        sv = _floats(np.ctypeslib.as_array(o.saveat, (o.n_saveat,))) if o.n_saveat else None
        self._say("tran", t0=float(t0), t1=float(t1), abstol=o.abstol, reltol=o.reltol, max_order=o.max_order, dtmin=o.dtmin, dtmax=o.dtmax, dt0=o.dt0,
                  max_steps=o.max_steps, newton_maxiters=o.newton_maxiters, saveat=sv, skip_dc=o.skip_dc, stepper=o.stepper,
                  step_control=o.step_control, dc=_dc_record(o.dc, S * n))
        rc, _ = self._outcome("tran")
        if sv is None:      # free steps: an uneven grid with one repeated time (a restart), dense-output polynomials of up to 5 points
            t = t0 + (t1 - t0) * np.array([0.0, 0.05, 0.1, 0.2, 0.2, 0.35, 0.5, 0.7, 0.85, 1.0])
            pts = np.array([0, 1, 2, 3, 1, 2, 3, 4, 5, 5], np.int32)
        else:
            t, pts = np.array(sv), np.zeros(len(sv), np.int32)
        i = np.arange(len(t))
        v = _grid((nobs, len(t), S), 2.0) + 1e-2 * ((i * i) % 7)[None, :, None]
        return rc, t, v, self._eliminate(_grid((S, n), 3.0)), self._stats(dense_points=pts, device_rows=None)

    def ac(self, freqs_hz, opts=None):
        S, n, f = self.n_samples, self.n_mna, np.asarray(freqs_hz, float)
        self._say("ac", freqs=_floats(f), opts=_dc_record(opts, S * n))
        rc, _ = self._outcome("ac")
        g = _grid((S, len(f), n), 4.0)
        return rc, self._eliminate(g - 1j * (0.5 * g + 0.25)), self._stats()

    def noise(self, out_kind, out_index, freqs_hz, opts=None):
        S, f = self.n_samples, np.asarray(freqs_hz, float)
        self._say("noise", out_kind=int(out_kind), out_index=int(out_index), freqs=_floats(f), opts=_dc_record(opts, S * self.n_mna))
        rc, _ = self._outcome("noise")
        return rc, _grid((S, len(f)), 5.0) + 10.0 * out_kind + out_index, self._stats()

    def _sens_record(self, slot_ids, rel_step, abs_step):
        so = sens_opts(rel_step=rel_step, abs_step=abs_step, n_par=len(slot_ids))     # raises on an abs_step of the wrong length, as the engine does
        return {"slot_ids": [int(i) for i in slot_ids], "rel_step": so.rel_step,
                "abs_step": _floats(np.ctypeslib.as_array(so.abs_step, (len(slot_ids),))) if so.abs_step else None}

    def dc_sens(self, slot_ids, opts=None, rel_step=None, abs_step=None):
        S, n, P = self.n_samples, self.n_mna, len(slot_ids)
        self._say("dc_sens", opts=_dc_record(opts, S * n), **self._sens_record(slot_ids, rel_step, abs_step))
        rc, status = self._outcome("dc_sens")
        sens = self._eliminate(_grid((S, P, n), 6.0))
        sens[status != 0] = np.nan
        return rc, self._eliminate(_grid((S, n), 1.0)), sens, status, self._stats()

    def ac_sens(self, slot_ids, freqs_hz, opts=None, rel_step=None, abs_step=None):
        S, n, P, f = self.n_samples, self.n_mna, len(slot_ids), np.asarray(freqs_hz, float).reshape(-1)
        self._say("ac_sens", freqs=_floats(f), opts=_dc_record(opts, S * n), **self._sens_record(slot_ids, rel_step, abs_step))
        rc, status = self._outcome("ac_sens")
        g, h = _grid((S, len(f), n), 7.0) + f[None, :, None] * 1e-9, _grid((S, len(f), P, n), 8.0) + f[None, :, None, None] * 1e-9
        x, sens = self._eliminate(g - 1j * (0.5 * g + 0.25)), self._eliminate(h + 1j * (0.25 * h - 0.5))
        dsens = self._eliminate(_grid((S, P, n), 6.0))
        sens[status != 0] = np.nan
        dsens[status != 0] = np.nan
        return rc, x, dsens, sens, status, self._stats()


@contextlib.contextmanager
def standin(plan=None):
    """Binds the stand-in over EngineCircuit, Context and default_context in every loaded module of the package that binds one."""
    global _BOX
    import cedarsim_jl_amd  # noqa: F401  (every module of the layer is loaded by now)
    box = _BOX = Box(plan)
    new = {"EngineCircuit": StandIn, "Context": StandInContext, "default_context": lambda device_id=None: box.default}
    saved = []
    for name, mod in list(sys.modules.items()):
        if mod is not None and (name == "cedarsim_jl_amd" or name.startswith("cedarsim_jl_amd.")):
            for attr in new:
                if attr in vars(mod):
                    saved.append((mod, attr, vars(mod)[attr]))
                    setattr(mod, attr, new[attr])
    try:
        yield box
    finally:
        for mod, attr, old in saved:
            setattr(mod, attr, old)
        _BOX = None


# ---- what a case records of each kind of result -----------------------------------------------------------------------------------
def _times(r, key, sol, syms, span):
    """sol(t): scalar and vector, idxs a string and a list."""
    tq = span[0] + (span[1] - span[0]) * np.array([0.0, 0.03, 0.2, 0.41, 0.77, 0.93, 1.0])
    for s in syms:
        r.do("%s/(tq,%s)" % (key, s), lambda: sol(tq, idxs=s))
    r.do(key + "/(scalar,str)", lambda: sol(float(tq[3]), idxs=syms[0]))
    r.do(key + "/(scalar,list)", lambda: np.array(sol(float(tq[3]), idxs=list(syms[:2]))))
    r.do(key + "/(tq,list)", lambda: np.array(sol(tq, idxs=list(syms[:2]))))


def _ac_like(r, key, a, syms, lists=(W5,)):
    for k, w in enumerate(lists):
        for s in syms:
            r.do("%s/freqresp%d[%s]" % (key, k, s), lambda: a.freqresp(s, w))
        r.stats("%s/stats%d" % (key, k), a.stats)


def _acsens(r, key, a, syms, pars, lists=(W5, W3, W5)):
    """H, dH/dp and the pair's magnitude / phase sensitivities at several frequency lists in a row, then .op and .dc_sens."""
    for k, w in enumerate(lists):
        _ac_like(r, "%s/w%d" % (key, k), a, syms, (w,))
        for s in syms:
            for p in pars:
                r.do("%s/w%d/sens[%s,%s]" % (key, k, s, p), lambda: a.sens(s, p, w))
    r.do(key + "/mag_phase", lambda: mag_phase_sens(a.freqresp(syms[0], W3), a.sens(syms[0], pars[0], W3)))
    r.solution(key + "/op", a.op, syms)
    r.sens(key + "/dc_sens", a.dc_sens, syms, pars)


# ---- A: the layer on the CPU ----------------------------------------------------------------------------------------------------------
SPAN = (0.0, 3.4e-6)                 # 5 time constants of the divider
GRID = np.linspace(0.0, 3.4e-6, 11)
PARS = ["r1", "v1", ("v1", "dc"), ("r1", "m"), "temp", "gmin"]
ASKED = PARS + ["r2", ("r1", "w"), "V1"]      # one that was not requested, one unknown field, another spelling


def _cpu(fn, plan=None):
    def run():
        r = Rec(floats=True)
        with standin(plan) as box, warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            r.do("raised", lambda: fn(r) or "nothing")
            r.put("warnings", json.dumps([str(w.message) for w in caught]))
            r.put("trace", box.trace())
        return r
    return run


def a_dc(r):
    r.solution("plain", dc(divider()), SYMS["divider"])
    x0 = np.array([0.25, 0.5, -0.125])
    r.solution("u0", dc(divider(), abstol=1e-12, maxiters=50, n_restarts=3, seed=4, tran_mode=True, u0=x0), SYMS["divider"])
    r.solution("observe", dc(meter(), observe=["node_b", "a", "vs.i"], ctx=StandInContext(3)), SYMS["meter"])
    r.solution("rlc", dc(rlc()), SYMS["rlc"])
    r.do("not_a_circuit", lambda: dc(42))


def a_dc_fails(r):
    r.solution("failed", dc(meter()), SYMS["meter"])


def a_tran(r):
    sol = tran(divider(), SPAN)
    r.solution("free", sol, SYMS["divider"])
    _times(r, "free", sol, ["node_out", "r1.i", "c1.i"], SPAN)
    sol = tran(rlc(), SPAN, abstol=1e-8, reltol=1e-5, saveat=GRID, max_order=3, dc_abstol=1e-13, dtmax=1e-7, stepper="host")
    r.solution("grid", sol, SYMS["rlc"])
    _times(r, "grid", sol, ["node_out", "l1.i", "l1.v"], SPAN)
    r.solution("u0", tran(meter(), SPAN, u0=[0.5, 0.25, 0.125, -1.0, -2.0], observe=["b"]), SYMS["meter"])
    r.solution("tranop", tran(divider(), SPAN, initializealg="tranop", saveat=GRID), ["out"])
    nl = parse_spice(NETLIST)
    r.solution("netlist", tran(nl), ["out", "r1.i"])
    ckt = nl.build()
    ckt._netlist = nl
    r.solution("netlist_circuit", tran(ckt), ["out"])
    r.do("no_tspan", lambda: tran(divider()))
    r.do("no_tran_card", lambda: tran(parse_spice(NETLIST.replace(".TRAN 1e-8 2e-6\n", ""))))


def a_ac_noise(r):
    a = ac(rlc(), abstol=1e-11, maxiters=20, n_restarts=2, seed=5)
    _ac_like(r, "rlc", a, SYMS["rlc"], (W5, W3))
    r.do("bode", lambda: a.bode("l1.i", W5))
    _ac_like(r, "meter", ac(meter(), ctx=StandInContext(2)), SYMS["meter"])
    r.do("no_source", lambda: ac(divider()))
    n = noise(rlc(), seed=7)
    for s in SYMS["rlc"]:
        r.do("psd[%s]" % s, lambda: n.psd(s, W5))
    r.stats("psd_stats", n.stats)
    r.do("psd_dv", lambda: noise(meter()).psd("vs.v", W3))
    r.do("psd_branch", lambda: noise(meter()).psd("vs.i", W3))
    r.do("acdec", lambda: acdec(7, 1e2, 3e5))


def a_ac_noise_fail(r):
    r.do("ac", lambda: ac(rlc()).freqresp("out", W3))
    r.do("noise", lambda: noise(rlc()).psd("out", W3))


def a_eliminated(r):
    """The 0 V source's branch row is NaN with every retcode 0: the real-valued picker and the complex one both raise."""
    r.solution("dc", dc(meter()), SYMS["meter"])
    r.sens("dc_sens", dc_sens(meter(), ["r1"]), ["vs.i", "v1.i", "b"], ["r1"])
    _ac_like(r, "ac", ac(meter()), ["vs.i", "v1.i", "vs.v"], (W3,))
    a = ac_sens(meter(), ["r1"])
    _acsens(r, "ac_sens", a, ["vs.i", "b"], ["r1"], (W3,))


def a_dc_sens(r):
    s = dc_sens(meter(), PARS, abstol=1e-12, maxiters=40, n_restarts=1, seed=2, tran_mode=True, u0=np.arange(5.0), rel_step=1e-4,
                abs_step=[0.0, 1e-3, 0.0, 0.0, 0.5, 0.0])
    r.sens("meter", s, SYMS["meter"], ASKED)
    r.solution("meter/op", s.op, SYMS["meter"])
    s = dc_sens(rlc(), ["l1", "c1"], ctx=StandInContext(1))
    r.sens("rlc", s, SYMS["rlc"], ["l1", "c1"])
    r.do("abs_step", lambda: dc_sens(divider(), ["r1", "r2"], abs_step=[1.0]))
    r.do("unknown_parameter", lambda: dc_sens(divider(), ["r7"]))


def a_ac_sens(r):
    _acsens(r, "meter", ac_sens(meter(), PARS, abstol=1e-12, maxiters=40, n_restarts=1, seed=2, rel_step=1e-4), SYMS["meter"], ASKED)
    _acsens(r, "rlc", ac_sens(rlc(), ["l1", ("v1", "dc")], abs_step=[1e-9, 0.0], ctx=StandInContext(1)), ["out", "l1.i", "l1.v"], ["l1", "v1"])
    a = ac_sens(rlc(), ["c1"])
    r.sens("dc_sens_first", a.dc_sens, ["out", "l1.i"], ["c1"])          # .dc_sens before any frequency list was asked for
    r.do("no_source", lambda: ac_sens(divider(), ["r1"]))
    r.do("abs_step", lambda: ac_sens(rlc(), ["r1"], abs_step=[1.0, 2.0]).freqresp("out", W3))


def _sweep(build, n, **kw):
    values = [1e3 * (1.0 + 0.5 * k) for k in range(n)]
    return CircuitSweep(build, Sweep(r1=values), **kw)


def _sweep_all(r, cs_of, ctx=None, sens=True, groups=False):
    """dc, tran and (sens=True) dc_sens and ac_sens through one kind of CircuitSweep; `cs_of(build)` makes it.  With groups, no call
    that fails after the engine circuits are made: whether the second group starts at all once the first has raised is a race."""
    for k, sol in enumerate(dc(cs_of(meter), abstol=1e-11, maxiters=30, n_restarts=2, seed=3, tran_mode=True, u0=np.ones(5), observe=["a"], ctx=ctx)):
        r.solution("dc/%d" % k, sol, SYMS["meter"])
    cs = cs_of(divider)
    r.put("len", [len(cs), len(list(cs))])
    sols = tran(cs, SPAN, abstol=1e-7, reltol=1e-4, initializealg="tranop", dc_abstol=1e-12, max_order=4, dtmax=1e-7, ctx=ctx)
    r.put("setup", json.dumps({k: v for k, v in cs.setup.items() if k != "seconds"}))
    for k, sol in enumerate(sols):
        r.solution("tran/%d" % k, sol, SYMS["divider"])
        _times(r, "tran/%d" % k, sol, ["out", "r1.i"], SPAN)
    for k, sol in enumerate(tran(cs_of(rlc), SPAN, saveat=GRID, u0=np.ones(4), observe=["a"], ctx=ctx)):
        r.solution("tran_grid/%d" % k, sol, ["out", "l1.i", "r1.i"])
    if not groups:
        r.do("unknown_kwarg", lambda: tran(cs_of(divider), SPAN, no_such_option=1, ctx=ctx))
    if not sens:
        return
    for k, s in enumerate(dc_sens(cs_of(meter), PARS, abstol=1e-12, seed=2, tran_mode=True, u0=np.ones(5), rel_step=1e-4, ctx=ctx)):
        r.sens("dc_sens/%d" % k, s, SYMS["meter"], ASKED)
        r.solution("dc_sens/%d/op" % k, s.op, SYMS["meter"])
    for k, a in enumerate(ac_sens(cs_of(meter), ["r1", "v1"], maxiters=40, abs_step=[0.5, 0.0], ctx=ctx)):
        _acsens(r, "ac_sens/%d" % k, a, ["b", "vs.i", "vs.v"], ["r1", "v1", "r2"], (W3, W5))
    r.do("ac_sens_no_source", lambda: ac_sens(cs_of(divider), ["r1"], ctx=ctx))


def a_sweep3(r):
    _sweep_all(r, lambda b: _sweep(b, 3))


def a_sweep_ctx(r):
    _sweep_all(r, lambda b: _sweep(b, 3), ctx=StandInContext(5))


def a_groups(r):
    _sweep_all(r, lambda b: _sweep(b, 4, groups=2), groups=True)


def a_groups_more_than_points(r):
    for k, sol in enumerate(dc(_sweep(meter, 2, groups=5))):
        r.solution("dc/%d" % k, sol, ["b"])


def a_warm(r):
    _sweep_all(r, lambda b: _sweep(b, 3, warm_start=True))
    for k, sol in enumerate(dc(_sweep(meter, 1, warm_start=True))):
        r.solution("one_point/%d" % k, sol, ["b"])


def a_warm_groups(r):
    _sweep_all(r, lambda b: _sweep(b, 4, groups=2, warm_start=True), sens=False, groups=True)


def a_shards(r):
    for rank in (0, 1, 2):
        cs = _sweep(divider, 5, rank=rank, world=3)
        for k, sol in enumerate(dc(cs)):
            r.solution("rank%d/dc/%d" % (rank, k), sol, ["out", "r1.i"])
    r.put("empty", len(dc(_sweep(divider, 1, rank=1, world=2))))


def a_tran_arrays(r):
    cs = _sweep(divider, 5, rank=1, world=2)
    rc, t, rows, st = cs.tran_arrays(SPAN, abstol=1e-7, reltol=1e-4, dc_abstol=1e-12, saveat=GRID, stepper="device", max_order=3)
    r.put("rc", rc)
    r.put("t", t)
    r.put("rows", rows)
    r.put("contiguous", bool(rows.flags["C_CONTIGUOUS"]))
    r.stats("stats", st)
    r.put("last_engine", [cs._last_engine.n_samples, type(cs._last_engine).__name__ == "StandIn"])
    rc, t, rows, st = _sweep(rlc, 3).tran_arrays(SPAN)
    r.put("free/t", t)
    r.put("free/rows", rows)


def a_sens_some_failed(r):
    s = dc_sens(_sweep(meter, 3), ["r1", "v1"])
    for k, x in enumerate(s):
        r.sens("dc_sens/%d" % k, x, ["b", "vs.i"], ["r1", "v1"])          # the failed sample's NaN branch row is handed out: its rc is not 0
        r.solution("dc_sens/%d/op" % k, x.op, ["b"])
    for k, a in enumerate(ac_sens(_sweep(meter, 3), ["r1"])):
        _acsens(r, "ac_sens/%d" % k, a, ["b", "vs.i"], ["r1"], (W3,))


def a_sens_fails(r):
    r.do("dc_sens", lambda: dc_sens(meter(), ["r1"]))
    r.do("dc_sens_sweep", lambda: dc_sens(_sweep(meter, 3), ["r1"]))
    r.do("ac_sens", lambda: ac_sens(meter(), ["r1"]).freqresp("b", W3))
    r.do("ac_sens_sweep", lambda: ac_sens(_sweep(meter, 3), ["r1"])[1].sens("b", "r1", W3))
    r.do("ac_sens_dc_sens", lambda: ac_sens(meter(), ["r1"]).dc_sens)
    r.solution("ac_sens_op", ac_sens(meter(), ["r1"]).op, ["b"])           # .op alone does not check


def a_op_of_a_model_instance(r):
    """Solution.op on a hand-built solution: the context given, and the default one fetched when called."""
    import types
    c = divider()
    mod = types.SimpleNamespace(nodes=["p", "n"], params=[("gain", "real", None, None)])
    c.va_par = [2.5, 1.0]
    c.va_instances = {"x1": (mod, {})}
    c._add("x1", c.dev_kind[1], ("in", "out"), ipar=(4, 0))
    from cedarsim_jl_amd import Solution
    sol = Solution(c, np.array([0.0, 1.0]), {("v", 1): np.array([1.5, 1.25]), ("v", 2): np.array([1.0, 0.75])}, None, 0, {})
    r.put("given", json.dumps(sol.op("X1", ctx=StandInContext(6))))
    r.put("default", json.dumps(sol.op("x1", index=0)))
    r.do("not_an_instance", lambda: sol.op("r1"))
    r.do("not_observed", lambda: Solution(c, np.array([0.0, 1.0]), {}, None, 0, {})["out"])
    r.do("branch_not_observed", lambda: Solution(c, np.array([0.0, 1.0]), {("v", 1): np.zeros(2)}, None, 0, {})["v1.i"])


SOME = {"fail": {"dc_sens": (-3, [1]), "ac_sens": (-3, [1])}, "eliminated": ["vs"]}
CPU_CASES = {
    "dc": _cpu(a_dc),
    "dc_fails": _cpu(a_dc_fails, {"fail": {"dc": (-3, "all")}}),
    "tran": _cpu(a_tran),
    "ac_noise": _cpu(a_ac_noise),
    "ac_noise_singular": _cpu(a_ac_noise_fail, {"fail": {"ac": (-2, "all"), "noise": (-2, "all")}}),
    "eliminated": _cpu(a_eliminated, {"eliminated": ["vs"]}),
    "dc_sens": _cpu(a_dc_sens),
    "ac_sens": _cpu(a_ac_sens),
    "sweep3": _cpu(a_sweep3),
    "sweep3_ctx": _cpu(a_sweep_ctx),
    "sweep3_dc_failed": _cpu(lambda r: _sweep_all(r, lambda b: _sweep(b, 3), sens=False), {"fail": {"dc": (-3, [0, 2]), "tran": (-4, "all")}}),
    "groups2": _cpu(a_groups),
    "groups_more_than_points": _cpu(a_groups_more_than_points),
    "warm": _cpu(a_warm),
    "warm_first_dc_fails": _cpu(a_warm, {"fail": {"dc": (-3, "all")}, "only_S": 1}),
    "warm_groups2": _cpu(a_warm_groups),
    "shards": _cpu(a_shards),
    "tran_arrays": _cpu(a_tran_arrays),
    "sens_some_failed": _cpu(a_sens_some_failed, SOME),
    "sens_all_failed": _cpu(a_sens_fails, {"fail": {"dc_sens": (-3, "all"), "ac_sens": (-3, "all"), "dc": (-3, "all")}}),
    "sens_singular": _cpu(a_sens_fails, {"fail": {"dc_sens": (-2, [0]), "ac_sens": (-2, [0])}}),
    "op_of_a_model_instance": _cpu(a_op_of_a_model_instance),
}


# ---- B: end to end on the GPU -----------------------------------------------------------------------------------------------------------
def _gpu(fn):
    def run():
        r = Rec(floats=False)
        fn(r)
        return r
    return run


def b_dc_tran(r):
    r.solution("dc/divider", dc(divider(), abstol=1e-12), SYMS["divider"][:12])
    r.solution("dc/meter", dc(meter(), abstol=1e-12), SYMS["meter"][:9])
    sol = tran(divider(), SPAN, abstol=1e-8, reltol=1e-6)
    r.solution("free", sol, SYMS["divider"][:12])
    _times(r, "free", sol, ["node_out", "r1.i", "c1.i"], SPAN)
    sol = tran(rlc(), SPAN, abstol=1e-8, reltol=1e-6, saveat=GRID)
    r.solution("grid", sol, SYMS["rlc"][:9])
    _times(r, "grid", sol, ["node_out", "l1.i"], SPAN)


def b_small_signal(r):
    _ac_like(r, "ac", ac(rlc(), abstol=1e-12), SYMS["rlc"][:9])
    n = noise(rlc(), abstol=1e-12)
    for s in ("out", "a", "l1.i"):
        r.do("psd[%s]" % s, lambda: n.psd(s, W5))
    r.stats("psd_stats", n.stats)
    s = dc_sens(meter(), ["r1", "v1"], abstol=1e-12)
    r.sens("dc_sens", s, SYMS["meter"][:9], ["r1", "v1"])
    r.solution("dc_sens/op", s.op, SYMS["meter"][:9])
    _acsens(r, "ac_sens", ac_sens(rlc(), ["l1", "c1"], abstol=1e-12), ["out", "l1.i", "l1.v"], ["l1", "c1"], (W5, W3))


def b_inverter_sens(r):
    from cedarsim_jl_amd.circuit import DEV_MOS
    from cedarsim_jl_amd.workloads import inverter
    c = inverter()
    pars = [(c.dev_names[c.dev_kind.index(DEV_MOS)], "w"), (c.model_names[0], "vth0")]
    s = dc_sens(c, pars, abstol=1e-12)
    r.sens("dc_sens", s, ["q", "d", "vvdd.i"], pars)
    r.solution("dc_sens/op", s.op, ["q", "d"])


def _b_sweep(r, cs_of):
    for k, sol in enumerate(dc(cs_of(meter), abstol=1e-12)):
        r.solution("dc/%d" % k, sol, SYMS["meter"][:9])
    for k, sol in enumerate(tran(cs_of(divider), SPAN, abstol=1e-8, reltol=1e-6, saveat=GRID)):
        r.solution("tran/%d" % k, sol, ["out", "r1.i", "c1.i"])
    for k, s in enumerate(dc_sens(cs_of(meter), ["r1", "v1"], abstol=1e-12)):
        r.sens("dc_sens/%d" % k, s, ["b", "vs.i", "vs.v"], ["r1", "v1"])
        r.solution("dc_sens/%d/op" % k, s.op, ["b"])
    for k, a in enumerate(ac_sens(cs_of(rlc), ["r1", "c1"], abstol=1e-12)):
        _acsens(r, "ac_sens/%d" % k, a, ["out", "l1.i"], ["r1", "c1"], (W5,))


def b_sweep3(r):
    _b_sweep(r, lambda b: _sweep(b, 3))


def b_groups2(r):
    _b_sweep(r, lambda b: _sweep(b, 4, groups=2))


def b_warm(r):
    _b_sweep(r, lambda b: _sweep(b, 3, warm_start=True))


def b_tran_arrays(r):
    cs = _sweep(divider, 5, rank=1, world=2)
    rc, t, rows, st = cs.tran_arrays(SPAN, abstol=1e-8, reltol=1e-6, saveat=GRID)
    r.put("rc", rc)
    r.put("t", t)
    r.put("rows", rows)
    r.stats("stats", st)
    r.put("samples", cs._last_engine.n_samples)


GPU_CASES = {
    "dc_tran": _gpu(b_dc_tran),
    "small_signal": _gpu(b_small_signal),
    "inverter_sens": _gpu(b_inverter_sens),
    "sweep3": _gpu(b_sweep3),
    "groups2": _gpu(b_groups2),
    "warm": _gpu(b_warm),
    "tran_arrays": _gpu(b_tran_arrays),
}


def pack(rec):
    """One case's entries as two arrays, an index (JSON: key, dtype, shape) and all the bytes: thousands of small entries would
    cost more in file headers than in content."""
    index = [[k, rec[k].dtype.str, list(rec[k].shape)] for k in rec]
    blob = b"".join(rec[k].tobytes() for k in rec)
    return np.array(json.dumps(index)), np.frombuffer(blob, np.uint8)


def unpack(index, blob):
    out, at, raw = {}, 0, blob.tobytes()
    for k, dtype, shape in json.loads(str(index)):
        n = np.dtype(dtype).itemsize * int(np.prod(shape, dtype=np.int64))
        out[k] = np.frombuffer(raw[at:at + n], np.dtype(dtype)).reshape(shape)
        at += n
    return out


def assert_recorded(got, golden, name):
    """Every entry of a case's run is, bit for bit, the recorded one (`golden`: the loaded file)."""
    want = unpack(golden[name + "/index"], golden[name + "/bytes"])
    assert list(got) == list(want), sorted(set(got) ^ set(want))[:10]
    bad = [k for k in got if not identical(got[k], want[k])]
    for k in bad[:5]:
        print("%s: %s\n  got      %r\n  recorded %r" % (name, k, got[k], want[k]))
    assert not bad, (len(bad), bad[:10])


def record(cases, log=print):
    """{name/index, name/bytes} (see `pack`) for every case whose two runs agree in every bit, and the names of those that do not."""
    rec, dropped = {}, []
    for name in cases:
        a, b = cases[name](), cases[name]()
        bad = [k for k in a if k not in b or not identical(a[k], b[k])] + [k for k in b if k not in a]
        if bad:
            dropped.append(name)
            log("%s: %d of %d entries differ between two runs (%s): case left out" % (name, len(bad), len(a), ", ".join(bad[:6])))
            continue
        rec[name + "/index"], rec[name + "/bytes"] = pack(a)
        log("%s: %d entries, raised: %s" % (name, len(a), a["raised"] if "raised" in a else "-"))
    return rec, dropped
