"""User-facing analyses — host-side mirror of CedarSim's problem surface for the hot path.

    dc(circuit; abstol…)                ≙ dc!(circ)                 src/sweeps.jl:437-448
    tran(circuit, tspan; abstol, reltol) ≙ tran!(circ, tspan)        src/sweeps.jl:450-465
    CircuitSweep(builder, sweep)         ≙ CircuitSweep(circuit, sweep)  src/sweeps.jl:390-435
    dc(cs) / tran(cs, tspan)             ≙ dc!(cs) / tran!.(…) broadcast  src/sweeps.jl:448,471-502
    sol.retcode, sol.t, sol["node_q"], sol["r.i"], sol(t, idxs=…), sol.stats   SURVEY §8(b)
    ac(circuit) → ACSolution.freqresp(sym, ωs)  ≙ ac!(circ), freqresp(ac, sym, ωs)  src/ac.jl:166-177, 267-284
    noise(circuit) → NoiseSolution.psd(sym, ωs)  ≙ noise!(circ), PSD(noise, sym, ωs) src/ac.jl:178-186, 286-305
    acdec(nd, fstart, fstop)             ≙ acdec                     src/ac.jl:307-323
    dc_sens(circuit, params) → SensSolution["node_out", "r1"]  ≙ d(sol[sys.node_out])/dp through SciMLSensitivity  test/sensitivity.jl
    ac_sens(circuit, params) → ACSensSolution.freqresp(sym, ωs), .sens(sym, par, ωs)  ≙ d(freqresp(ac, sym, ωs))/dp (ngspice: .sens … ac)

The reference loops serially over sweep points, paying a full DC + transient each
(`broadcast(sims) do sim … remake(prob, p=sim)`, src/sweeps.jl:473-480).  Here every point becomes one
*sample* of a single batched GPU solve (`ch_set_params` + one `ch_dc`/`ch_tran`); with several ranks
the points are split into contiguous shards, one per GPU, and results are gathered at the end.
All numerics run in libcedarhip.so; nothing here computes a circuit solution.
"""
import math
import warnings

import numpy as np

from .circuit import DEV_C, DEV_L, DEV_R, DEV_V, DEV_VCVS, RETCODES, CedarError, Circuit, dc_opts, tran_opts
from .engine import Context, EngineCircuit, default_context
from .sweepmap import learn_batch, sample_view
from .sweeps import shard_range, sweepify


def _split_sym(ckt, sym):
    """'node_q' / 'q' -> (node name, None, None); 'r1.i' / 'r1.v' -> (None, device index, 'i' / 'v'); anything else is a KeyError."""
    nm = str(sym).lower()
    if nm.startswith("node_"):
        nm = nm[5:]
    if nm in ckt._node_ix:
        return nm, None, None
    if "." in nm:
        dev, fld = nm.rsplit(".", 1)
        if dev in ckt.dev_names and fld in ("i", "v"):
            return None, ckt.dev_names.index(dev), fld
    raise KeyError(sym)


def _dense_eval(tt, pts, y, tq):
    """The BDF dense-output polynomials of a run at times `tq`: the step that ended at saved row i runs through its pts[i] newest rows."""
    y = np.asarray(y, float)
    out = np.empty(len(tq))
    for q, x in enumerate(tq):
        if x <= tt[0] or x >= tt[-1]:
            out[q] = y[0] if x <= tt[0] else y[-1]
            continue
        i = int(np.searchsorted(tt, x, side="left"))          # tt[i-1] < x <= tt[i]: the step that ended at row i covers x
        m = min(int(pts[i]), i + 1)
        rows = list(range(i - m + 1, i + 1))
        if m < 2 or len(set(tt[rows])) < m:
            out[q] = np.interp(x, tt[i - 1:i + 1], y[i - 1:i + 1]) if tt[i] > tt[i - 1] else y[i]
            continue
        acc = 0.0
        for a in rows:
            w = 1.0
            for b in rows:
                if b != a:
                    w *= (x - tt[b]) / (tt[a] - tt[b])
            acc += w * y[a]
        out[q] = acc
    return out


def _pchip_eval(tt, y, tq):
    """Shape-preserving cubic (PCHIP) through the saved rows at times `tq`, clipped to the run's span."""
    y = np.asarray(y, float)
    uniq = np.concatenate(([True], np.diff(tt) > 0)) if len(tt) > 1 else np.ones(len(tt), bool)   # restart steps repeat a time
    if uniq.sum() < 3:
        return np.interp(tq, tt, y)
    from scipy.interpolate import PchipInterpolator
    return PchipInterpolator(tt[uniq], y[uniq], extrapolate=False)(np.clip(tq, tt[0], tt[-1]))


class Solution:
    """Solution of one sample: time points, observables by name, retcode and stats."""

    def __init__(self, circuit, t, cols, x_final, rc, stats, params=None):
        self.circuit, self.t, self._cols, self.x_final = circuit, np.asarray(t), cols, x_final
        self.retcode = RETCODES.get(rc, str(rc))
        self.rc = rc
        self.stats = stats
        self.params = params or {}

    # -- symbolic indexing: "node_q" / "q" (node voltage), "r1.i" / "r1.v" (device current / voltage) --
    def _node_series(self, node):
        c = self.circuit
        n = c._n(node) if not isinstance(node, (int, np.integer)) else int(node)
        if n == 0:
            return np.zeros(len(self.t))
        key = ("v", n)
        if key in self._cols:
            return self._cols[key]
        if len(self.t) == 1 and self.x_final is not None:
            return np.array([self.x_final[n - 1]])
        raise KeyError("node '%s' was not observed" % node)

    def __getitem__(self, name):
        c = self.circuit
        node, i, fld = _split_sym(c, name)
        if node is not None:
            return self._node_series(node)
        v = self._node_series(c.dev_node[i][0]) - self._node_series(c.dev_node[i][1])
        if fld == "v":
            return v
        k = c.dev_kind[i]
        if k == DEV_R:
            return v / c.dev_par[i][0]
        if k in (DEV_V, DEV_L, DEV_VCVS):
            if ("i", i) in self._cols:
                return self._cols[("i", i)]
            if len(self.t) == 1 and self.x_final is not None:
                return np.array([self.x_final[c.mna_index("i", c.dev_names[i])]])
            raise KeyError("branch current of '%s' was not observed" % c.dev_names[i])
        if k == DEV_C:
            if len(self.t) < 2:
                return np.zeros(len(self.t))
            return c.dev_par[i][0] * np.gradient(v, self.t)  # post-processed derivative
        raise KeyError(name)

    def op(self, dev_name, index=-1, ctx=None):
        """Operating-point observables of a compiled Verilog-A instance at saved point `index` — `sol[sys.x1.gm]` for the
        variables a module declares with (* desc *) (src/vasim.jl:742-753).  Evaluated on the GPU from the node voltages."""
        c = self.circuit
        name = str(dev_name).lower()
        if name not in getattr(c, "va_instances", {}):
            raise KeyError("'%s' is not a compiled Verilog-A instance" % dev_name)
        i = c.dev_names.index(name)
        mid, ofs = c.dev_ipar[i]
        mod, _ = c.va_instances[name]
        v = [float(self._node_series(n)[index]) for n in c.dev_node[i][:len(mod.nodes)]]
        par = c.va_par[ofs:ofs + 2 * len(mod.params)]
        return (ctx or default_context()).va_opvars(mid, par, v, c.temp + 273.15, c.gmin)

    def default_name_map(self):
        """{solution key: column name} for every observed top-level node voltage — default_name_map (src/util.jl:239-260):
        the `node_` prefix is dropped and ground aliases are left out."""
        c = self.circuit
        out = {}
        for kind, idx in self._cols:
            if kind != "v":
                continue
            name = c.node_names[idx]
            if "." in name or name in ("0", "gnd"):
                continue
            out["node_" + name] = name
        return out

    def write_csv(self, path, name_map=None):
        """CSV.write(file, sol; name_map) (ext/CedarSimCSVExt.jl:13-19): column `t` then one column per mapped probe."""
        name_map = name_map or self.default_name_map()
        cols = [("t", self.t)] + [(name, self[key]) for key, name in name_map.items()]
        with open(path, "w") as f:
            f.write(",".join(n for n, _ in cols) + "\n")
            for i in range(len(self.t)):
                f.write(",".join(repr(float(v[i])) for _, v in cols) + "\n")
        return path

    def __call__(self, t, idxs=None):
        """`sol(t, idxs=…)` (test/gf180_dff.jl:29-33).  A run without a `saveat` grid carries, per accepted step, the number of
        newest saved points its BDF dense-output polynomial runs through (`ch_result_dense_points`): `sol(t)` evaluates exactly
        that polynomial — the value a `saveat` grid would have returned at t.  Results that are already on a `saveat` grid are
        interpolated between grid points by a shape-preserving cubic (PCHIP)."""
        names = idxs if isinstance(idxs, (list, tuple)) else [idxs]
        tt = np.asarray(self.t, float)
        tq = np.atleast_1d(np.asarray(t, float))
        pts = self.stats.get("dense_points") if isinstance(self.stats, dict) else None
        if pts is not None and len(pts) == len(tt) and np.any(np.asarray(pts) >= 2):
            out = [_dense_eval(tt, pts, self[n], tq) for n in names]
        else:
            out = [_pchip_eval(tt, self[n], tq) for n in names]
        if not np.ndim(t):
            out = [float(o[0]) for o in out]
        return out if isinstance(idxs, (list, tuple)) else out[0]


def _prepare(circuit, observe):
    if isinstance(circuit, Circuit):
        ckt = circuit
    elif hasattr(circuit, "build"):
        ckt = circuit.build()
    else:
        raise CedarError("expected a Circuit or a parsed netlist")
    if observe is None and not ckt.obs:
        ckt.observe_all_nodes()
        for i, k in enumerate(ckt.dev_kind):
            if k in (DEV_V, DEV_L, DEV_VCVS):
                ckt.observe_branch(ckt.dev_names[i])
    elif observe:
        for o in observe:
            o = str(o).lower()
            if o.endswith(".i") and o[:-2] in ckt.dev_names:
                ckt.observe_branch(o[:-2])
            else:
                ckt.observe_node(o[5:] if o.startswith("node_") else o)
    return ckt


def _solutions(ckt, t, v, xf, rc, st, S, point_params=None):
    """One Solution per sample of a batched transient: observable k of sample s is v[k, :, s]."""
    return [Solution(ckt, t, {o: (v[k, :, s] if v.size else np.zeros(0)) for k, o in enumerate(ckt.obs)},
                     xf[s] if xf is not None else None, rc, st, point_params[s] if point_params else None) for s in range(S)]


def _dc_columns(ckt, x_row):
    """{observable: one-point series} of a DC solution: node voltages and branch currents picked out of an MNA state row."""
    return {o: np.array([x_row[(o[1] - 1) if o[0] == "v" else ckt.mna_index("i", ckt.dev_names[o[1]])]]) for o in ckt.obs}


def dc(circuit, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, tran_mode=False, u0=None, observe=None, ctx=None):
    """DC operating point (CedarDCOp: sources at their .dc value, du = 0; src/dcop.jl:157-200)."""
    if isinstance(circuit, CircuitSweep):
        return circuit._run("dc", dict(abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed, tran_mode=tran_mode), ctx)
    ckt = _prepare(circuit, observe)
    eng = EngineCircuit(ckt, ctx)
    rc, x, status, st = eng.dc(dc_opts(abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed, tran_mode=tran_mode, x0=u0))
    if rc != 0:
        warnings.warn("DC operating point analysis failed. Further failures may follow.")  # src/dcop.jl:141
    return Solution(ckt, np.array([0.0]), _dc_columns(ckt, x[0]), x[0], rc, st)


def tran(circuit, tspan=None, abstol=1e-6, reltol=1e-3, u0=None, initializealg="dcop", dc_abstol=1e-10, saveat=None,
         max_order=5, observe=None, ctx=None, **kw):
    """Transient (solve(prob, IDA(); abstol, reltol, initializealg=CedarDCOp()), src/sweeps.jl:450-465).

    u0: MNA initial state → skips the DC solve (test/common.jl:36-43 `u0=` semantics).
    tspan defaults to the netlist's `.TRAN` (src/circsummary.jl:109-128)."""
    if isinstance(circuit, CircuitSweep):
        return circuit._run("tran", dict(tspan=tspan, abstol=abstol, reltol=reltol, initializealg=initializealg, dc_abstol=dc_abstol,
                                          saveat=saveat, max_order=max_order, **kw), ctx)
    if tspan is None:
        nl = circuit if hasattr(circuit, "tran") and not isinstance(circuit, Circuit) else getattr(circuit, "_netlist", None)
        if nl is None or nl.tran is None:
            raise CedarError("no tspan given and the netlist has no .TRAN statement")
        tspan = (0.0, nl.tran[1])
    ckt = _prepare(circuit, observe)
    eng = EngineCircuit(ckt, ctx)
    dco = dc_opts(abstol=dc_abstol, tran_mode=(initializealg == "tranop"), x0=None if u0 is None else np.asarray(u0, float)[None, :])
    opts = tran_opts(abstol=abstol, reltol=reltol, max_order=max_order, saveat=saveat, dc=dco, skip_dc=u0 is not None, **kw)
    rc, t, v, xf, st = eng.tran(tspan[0], tspan[1], opts)
    return _solutions(ckt, t, v, xf, rc, st, 1)[0]


def acdec(nd, fstart, fstop):
    """`.ac dec nd fstart fstop`: log-spaced frequencies in Hz (src/ac.jl:317-322)."""
    a, b = math.log10(fstart), math.log10(fstop)
    points = int(math.ceil((b - a) * nd)) + 1
    return 10.0 ** np.linspace(a, b, points)


def _resolve_sym(ckt, sym):
    """'node_vout' / 'vout' → ('v', node id); 'l3.i' → ('i', device index); 'l3.v' → ('dv', a, b)."""
    node, i, fld = _split_sym(ckt, sym)
    if node is not None:
        return ("v", ckt._n(node))
    if fld == "v":
        return ("dv", ckt.dev_node[i][0], ckt.dev_node[i][1])
    if ckt.dev_kind[i] in (DEV_V, DEV_L, DEV_VCVS):
        return ("i", i)
    raise KeyError(sym)


class ACSolution:
    """Linearisation around the DC operating point, sampled on demand (ACSol, src/ac.jl:10-13)."""

    def __init__(self, circuit, eng, opts):
        self.circuit, self._eng, self._opts = circuit, eng, opts
        self.stats = None

    def freqresp(self, sym, omegas, sample=0):
        """Complex response of `sym` to the circuit's AC sources at angular frequencies `omegas` (rad/s)."""
        ckt = self.circuit
        w = np.asarray(omegas, dtype=np.float64)
        rc, x, st = self._eng.ac(w / (2.0 * math.pi), self._opts)
        self.stats = st
        if rc != 0:
            raise CedarError("AC analysis failed (%s): %s" % (RETCODES.get(rc, rc), self._eng.ctx.last_error()))
        x = x[sample]

        def node(n):
            return np.zeros(len(w), complex) if n == 0 else x[:, n - 1]

        r = _resolve_sym(ckt, sym)
        if r[0] == "v":
            return node(r[1])
        if r[0] == "dv":
            return node(r[1]) - node(r[2])
        v = x[:, ckt.mna_index("i", ckt.dev_names[r[1]])]
        if np.any(np.isnan(v)):
            raise KeyError("branch current of '%s' was eliminated: observe it when building the circuit" % sym)
        return v

    def bode(self, sym, omegas, sample=0):
        h = self.freqresp(sym, omegas, sample)
        return np.abs(h), np.degrees(np.unwrap(np.angle(h))), np.asarray(omegas)


class NoiseSolution:
    """Output-noise analysis around the DC operating point (NoiseSol, src/ac.jl:15-20)."""

    def __init__(self, circuit, eng, opts):
        self.circuit, self._eng, self._opts = circuit, eng, opts
        self.stats = None

    def psd(self, sym, omegas, sample=0):
        """Power spectral density of `sym` (V²/Hz or A²/Hz) at angular frequencies `omegas` — PSD(noise, sym, ωs)."""
        r = _resolve_sym(self.circuit, sym)
        if r[0] == "dv":
            raise CedarError("noise output must be a node voltage or a branch current")
        w = np.asarray(omegas, dtype=np.float64)
        rc, out, st = self._eng.noise(0 if r[0] == "v" else 1, r[1], w / (2.0 * math.pi), self._opts)
        self.stats = st
        if rc != 0:
            raise CedarError("noise analysis failed (%s): %s" % (RETCODES.get(rc, rc), self._eng.ctx.last_error()))
        return out[sample]


def ac(circuit, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, ctx=None):
    """ac!(circ): DC operating point + linearisation; sample it with `.freqresp(sym, ωs)`."""
    ckt = _prepare(circuit, None)
    if not any(ckt.source_ac):
        raise CedarError("AC analysis needs at least one source with an `ac` magnitude")
    return ACSolution(ckt, EngineCircuit(ckt, ctx, small_signal=True), dc_opts(abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed))


def noise(circuit, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, ctx=None):
    """noise!(circ): resistor thermal noise referred to an output with `.psd(sym, ωs)`."""
    ckt = _prepare(circuit, None)
    return NoiseSolution(ckt, EngineCircuit(ckt, ctx, small_signal=True), dc_opts(abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed))


def _slot_of(ckt, name):
    """A parameter name as Circuit.slot takes it: "r1", "temp", ("m1", "w"), ("nfet_06v0", "vth0")."""
    n = len(ckt.slots)
    i = ckt.slot(*name) if isinstance(name, (tuple, list)) else ckt.slot(name)
    if i == n and ckt.slots.index(ckt.slots[i]) != i:   # the field already has a slot under another name (a sweep's learned slots): use that one
        first = ckt.slots.index(ckt.slots[i])
        ckt.slots.pop()
        ckt.slot_names.pop()
        return first
    return i


def _param_key(name):
    return tuple(str(x).lower() for x in name) if isinstance(name, (tuple, list)) else (str(name).lower(), None)


class SensSolution:
    """DC operating point of one sample and its derivatives with respect to the requested parameters (direct method on the GPU,
    ch_dc_sens): `s["node_out", "r1"]`, `s["v1.i", ("m1", "w")]`; `s.op` is the operating-point Solution, `s.sens` the raw
    [n_par][n_mna] array in the order of `s.params`."""

    def __init__(self, circuit, params, sens, op, rc):
        self.circuit, self.params, self.sens, self.op = circuit, list(params), np.asarray(sens), op
        self.rc, self.retcode = rc, RETCODES.get(rc, str(rc))
        self._col = {_param_key(p): k for k, p in enumerate(self.params)}

    def __getitem__(self, key):
        sym, par = key
        pk = _param_key(par)
        if pk not in self._col:
            if len(pk) == 2 and pk[1] is None and (pk[0], "dc") in self._col:
                pk = (pk[0], "dc")
            else:
                raise KeyError("no sensitivity with respect to %r was requested" % (par,))
        row = self.sens[self._col[pk]]
        ckt = self.circuit

        def node(n):
            return 0.0 if n == 0 else float(row[n - 1])

        r = _resolve_sym(ckt, sym)
        if r[0] == "v":
            return node(r[1])
        if r[0] == "dv":
            return node(r[1]) - node(r[2])
        v = float(row[ckt.mna_index("i", ckt.dev_names[r[1]])])
        if math.isnan(v) and self.rc == 0:
            raise KeyError("branch current of '%s' was eliminated: observe it when building the circuit" % sym)
        return v


def _sens_solutions(ckt, eng, params, slot_ids, dco, rel_step, abs_step, views=None, point_params=None):
    rc, x, sens, status, st = eng.dc_sens(slot_ids, dco, rel_step=rel_step, abs_step=abs_step)
    if rc != 0 and (rc != -3 or np.all(status != 0)):   # anything but "some operating points failed": nothing to hand out
        raise CedarError("DC sensitivity analysis failed (%s): %s" % (RETCODES.get(rc, rc), eng.ctx.last_error()))
    out = []
    for s in range(eng.n_samples):
        c = views[s] if views else ckt
        op = Solution(c, np.array([0.0]), _dc_columns(ckt, x[s]), x[s], int(status[s]), st, point_params[s] if point_params else None)
        out.append(SensSolution(c, params, sens[s], op, int(status[s])))
    return out


def dc_sens(circuit, params, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, tran_mode=False, u0=None, rel_step=None, abs_step=None, ctx=None):
    """DC operating point and d(solution)/d(parameter) for every name in `params` ("r1", ("m1", "w"), ("nfet_06v0", "vth0"), "temp",
    "gmin": what `Circuit.slot` takes) — the forward sensitivities of test/sensitivity.jl, by the direct method on the GPU."""
    if isinstance(circuit, CircuitSweep):
        return circuit.dc_sens(params, abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed, tran_mode=tran_mode,
                               rel_step=rel_step, abs_step=abs_step, ctx=ctx)
    ckt = _prepare(circuit, None)
    slot_ids = [_slot_of(ckt, p) for p in params]
    eng = EngineCircuit(ckt, ctx)
    dco = dc_opts(abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed, tran_mode=tran_mode, x0=None if u0 is None else np.asarray(u0, float)[None, :])
    return _sens_solutions(ckt, eng, params, slot_ids, dco, rel_step, abs_step)[0]


def mag_phase_sens(h, dh):
    """d|H|/dp and d(arg H)/dp (radians) from a complex response `h` and its derivative `dh` = dH/dp:
    (Re(conj(h) dh) / |h|, Im(dh / h))."""
    h, dh = np.asarray(h, complex), np.asarray(dh, complex)
    return np.real(np.conj(h) * dh) / np.abs(h), np.imag(dh / h)


def _ac_pick(ckt, x, sym):
    """Row of `sym` out of complex MNA phasors x[n_freq][n_mna] (the symbol rules of ACSolution.freqresp)."""
    def node(n):
        return np.zeros(x.shape[0], complex) if n == 0 else x[:, n - 1]

    r = _resolve_sym(ckt, sym)
    if r[0] == "v":
        return node(r[1])
    if r[0] == "dv":
        return node(r[1]) - node(r[2])
    v = x[:, ckt.mna_index("i", ckt.dev_names[r[1]])]
    if np.any(np.isnan(v)):
        raise KeyError("branch current of '%s' was eliminated: observe it when building the circuit" % sym)
    return v


class _ACSensRun:
    """One engine circuit (one sample per sweep point) behind the ACSensSolutions of its samples: a ch_ac_sens call per distinct
    frequency list, shared by all of them."""

    def __init__(self, ckt, eng, dco_kw, params, slot_ids, rel_step, abs_step):
        self.ckt, self.eng, self.dco_kw, self.params, self.slot_ids = ckt, eng, dict(dco_kw), list(params), list(slot_ids)
        self.rel_step, self.abs_step = rel_step, abs_step
        self._key, self._res, self._op, self.stats = None, None, None, None

    def at(self, omegas):
        w = np.ascontiguousarray(omegas, dtype=np.float64).reshape(-1)
        if self._key is None or self._key != w.tobytes():
            rc, x, dsens, sens, status, st = self.eng.ac_sens(self.slot_ids, w / (2.0 * math.pi), dc_opts(**self.dco_kw), rel_step=self.rel_step,
                                                              abs_step=self.abs_step)
            self.stats = st
            if rc != 0 and (rc != -3 or np.all(status != 0)):   # anything but "some operating points failed": nothing to hand out
                raise CedarError("AC sensitivity analysis failed (%s): %s" % (RETCODES.get(rc, rc), self.eng.ctx.last_error()))
            self._key, self._res = w.tobytes(), (x, dsens, sens, status)
        return self._res

    def op(self):
        if self._op is None:
            rc, x, status, st = self.eng.dc(dc_opts(**self.dco_kw), check=False)
            self._op = (x, status, st)
        return self._op


class ACSensSolution:
    """Small-signal response of one sample and its derivatives with respect to the requested parameters (direct method on the GPU,
    ch_ac_sens), sampled on demand like ACSolution: `.freqresp(sym, ωs)` is H, `.sens(sym, par, ωs)` the complex dH/dp
    (`mag_phase_sens(H, dH)` turns the pair into d|H|/dp and dφ/dp); `.op` is the operating-point Solution and `.dc_sens` the
    SensSolution of the same parameters."""

    def __init__(self, circuit, run, params, sample=0, point_params=None):
        self.circuit, self._run, self.params, self._s, self._pp = circuit, run, list(params), sample, point_params
        self._col = {_param_key(p): k for k, p in enumerate(self.params)}

    @property
    def stats(self):
        return self._run.stats

    def freqresp(self, sym, omegas):
        x, _, _, status = self._run.at(omegas)
        return _ac_pick(self.circuit, x[self._s], sym)

    def sens(self, sym, par, omegas):
        pk = _param_key(par)
        if pk not in self._col:
            if len(pk) == 2 and pk[1] is None and (pk[0], "dc") in self._col:
                pk = (pk[0], "dc")
            else:
                raise KeyError("no sensitivity with respect to %r was requested" % (par,))
        _, _, sens, _ = self._run.at(omegas)
        return _ac_pick(self.circuit, sens[self._s][:, self._col[pk], :], sym)

    @property
    def op(self):
        x, status, st = self._run.op()
        s = self._s
        return Solution(self.circuit, np.array([0.0]), _dc_columns(self._run.ckt, x[s]), x[s], int(status[s]), st, self._pp)

    @property
    def dc_sens(self):
        _, dsens, _, status = self._run._res if self._run._res is not None else self._run.at([0.0])
        return SensSolution(self.circuit, self.params, dsens[self._s], self.op, int(status[self._s]))


def ac_sens(circuit, params, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
    """ac!(circ) and d(response)/d(parameter) for every name in `params` (what `Circuit.slot` takes, as for dc_sens): an
    ACSensSolution.  A CircuitSweep gives a list, one per point, out of one batched solve."""
    if isinstance(circuit, CircuitSweep):
        return circuit.ac_sens(params, abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed, rel_step=rel_step, abs_step=abs_step, ctx=ctx)
    ckt = _prepare(circuit, None)
    if not any(ckt.source_ac):
        raise CedarError("AC analysis needs at least one source with an `ac` magnitude")
    slot_ids = [_slot_of(ckt, p) for p in params]
    eng = EngineCircuit(ckt, ctx, small_signal=True)
    run = _ACSensRun(ckt, eng, dict(abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed), params, slot_ids, rel_step, abs_step)
    return ACSensSolution(ckt, run, params)


class CircuitSweep:
    """Batched sweep over circuit parameters (src/sweeps.jl:390-435).

    builder: a parsed netlist (`.build(**params)`) or a callable `f(**params) -> Circuit`.
    Iterating yields one parameter dict per point (`s.params` in the reference)."""

    def __init__(self, builder, sweep, rank=0, world=1, groups="auto", warm_start=False):
        """warm_start=True: the DC operating point of the range's first point is solved alone and handed to every sample as its
        initial guess (`u0`), instead of ten `1e-7*randn` restarts per sample (src/dcop.jl:53-94).  Not the reference's behaviour
        (every `dc!` there starts cold), so it is opt-in; on the 1024-sample Monte-Carlo share of config 4 the DC phase drops from
        46 ms to 0.14 ms (profiles/r02_configs.json).  For a multistable circuit every sample then starts in the first point's basin."""
        self.warm_start = bool(warm_start)
        self.builder = builder
        self.sweep = sweepify(sweep)
        self.points = [{k: v for k, v in p if v is not None} for p in self.sweep]
        self.shape = self.sweep.shape
        self.rank, self.world = rank, world
        # groups > 1: this rank's points are split into that many contiguous groups, each a batched solve of its own with its
        # own stream and host stepper (one thread each).  A step attempt of one group costs ~36 us of kernel plus ~16 us of
        # host round trip during which the GPU would idle; a second group's kernel fills that gap (profiles/r01_notes.md),
        # and every group steps with the time steps ITS samples need.
        # Measured on one MI355X (scripts/sweep_groups.py, Monte-Carlo batch of one DFF): 8192 samples 0.46 s in one group,
        # 0.38 s in two, 0.35 s in four; no gain at 1024 samples (one launch does not fill the GPU there).  "auto": 4 groups
        # from 4096 points per rank, 2 from 2048, else 1.
        self.groups = groups if groups == "auto" else max(1, int(groups))
        self._build = builder.build if hasattr(builder, "build") else builder

    def __iter__(self):
        return iter(self.points)

    def __len__(self):
        return len(self.points)

    def _batch(self, lo, hi):
        """Base circuit + slots + per-sample values for points lo..hi (sweepmap.learn_batch); `self.setup` records what was done
        (builds, seconds, which way)."""
        base, slot_ids, vals, self.setup = learn_batch(self._build, self.points[lo:hi])
        return base, slot_ids, vals

    def _run(self, kind, kw, ctx):
        lo, hi = shard_range(len(self.points), self.rank, self.world)
        if hi <= lo:
            return []
        n = hi - lo
        G = (4 if n >= 4096 else 2 if n >= 2048 else 1) if self.groups == "auto" else min(self.groups, n)
        if G <= 1:
            return self._run_range(kind, kw, ctx, lo, hi)
        from concurrent.futures import ThreadPoolExecutor
        first = ctx if ctx is not None else default_context()
        ctxs = [first] + [Context(first.device_id) for _ in range(G - 1)]

        def work(g):
            a, b = shard_range(hi - lo, g, G)
            return self._run_range(kind, dict(kw), ctxs[g], lo + a, lo + b)

        with ThreadPoolExecutor(G) as ex:
            parts = list(ex.map(work, range(G)))
        return [sol for part in parts for sol in part]

    def _engine(self, lo, hi, ctx):
        """Points lo..hi as the samples of one engine circuit: (circuit, engine, slot ids, values[slot][sample])."""
        base, slot_ids, vals = self._batch(lo, hi)
        ckt = _prepare(base, None)
        eng = EngineCircuit(ckt, ctx)
        eng.set_samples(hi - lo)
        if slot_ids:
            eng.set_params(slot_ids, vals)
        return ckt, eng, slot_ids, vals

    def _run_range(self, kind, kw, ctx, lo, hi):
        if kind == "dc_sens":
            return self._sens_range(kw, ctx, lo, hi)
        if kind == "ac_sens":
            return self._acsens_range(kw, ctx, lo, hi)
        ckt, eng, _, vals = self._engine(lo, hi, ctx)
        S = hi - lo
        pts = self.points[lo:hi]
        x0 = None
        if self.warm_start and S > 1:
            e0 = EngineCircuit(_prepare(self._build(**pts[0]), None), ctx)
            rc0, xw, _, _ = e0.dc(dc_opts(abstol=kw.get("dc_abstol", kw.get("abstol", 1e-10)) if kind != "dc" else kw.get("abstol", 1e-10)))
            if rc0 == 0:
                x0 = np.tile(np.nan_to_num(xw[0]), (S, 1))
        if kind == "dc":
            rc, x, status, st = eng.dc(dc_opts(x0=x0, **kw))
            return [Solution(sample_view(ckt, vals, s), np.array([0.0]), _dc_columns(ckt, x[s]), x[s], int(status[s]), st, pts[s])
                    for s in range(S)]
        tspan = kw.pop("tspan")
        dco = dc_opts(abstol=kw.pop("dc_abstol", 1e-10), tran_mode=(kw.pop("initializealg", "dcop") == "tranop"), x0=x0)
        opts = tran_opts(dc=dco, **kw)
        rc, t, v, xf, st = eng.tran(tspan[0], tspan[1], opts)
        sols = _solutions(ckt, t, v, xf, rc, st, S, pts)
        for s, sol in enumerate(sols):
            sol.circuit = sample_view(ckt, vals, s)
        return sols

    def dc_sens(self, params, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, tran_mode=False, rel_step=None, abs_step=None, ctx=None):
        """Sensitivities of every sweep point with respect to `params`: one batched ch_dc_sens per sample group (the batching and
        sharding of `_run`); a list of SensSolution in sweep order, each differentiated at its own parameter point."""
        return self._run("dc_sens", dict(params=list(params), rel_step=rel_step, abs_step=abs_step,
                                          dc=dict(abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed, tran_mode=tran_mode)), ctx)

    def _sens_range(self, kw, ctx, lo, hi):
        base, slot_ids, vals = self._batch(lo, hi)
        ckt = _prepare(base, None)
        views = [sample_view(ckt, vals, s) for s in range(hi - lo)]
        ids = [_slot_of(ckt, p) for p in kw["params"]]   # declared before the engine circuit is built from the description
        eng = EngineCircuit(ckt, ctx)
        eng.set_samples(hi - lo)
        if slot_ids:
            eng.set_params(slot_ids, vals)
        return _sens_solutions(ckt, eng, kw["params"], ids, dc_opts(**kw["dc"]), kw["rel_step"], kw["abs_step"], views, self.points[lo:hi])

    def ac_sens(self, params, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
        """AC sensitivities of every sweep point with respect to `params`: one batched ch_ac_sens per sample group and frequency list
        (the batching and sharding of `_run`); a list of ACSensSolution in sweep order, each differentiated at its own point."""
        return self._run("ac_sens", dict(params=list(params), rel_step=rel_step, abs_step=abs_step,
                                          dc=dict(abstol=abstol, maxiters=maxiters, n_restarts=n_restarts, seed=seed)), ctx)

    def _acsens_range(self, kw, ctx, lo, hi):
        base, slot_ids, vals = self._batch(lo, hi)
        ckt = _prepare(base, None)
        if not any(ckt.source_ac):
            raise CedarError("AC analysis needs at least one source with an `ac` magnitude")
        views = [sample_view(ckt, vals, s) for s in range(hi - lo)]
        ids = [_slot_of(ckt, p) for p in kw["params"]]   # declared before the engine circuit is built from the description
        eng = EngineCircuit(ckt, ctx, small_signal=True)
        eng.set_samples(hi - lo)
        if slot_ids:
            eng.set_params(slot_ids, vals)
        run = _ACSensRun(ckt, eng, kw["dc"], kw["params"], ids, kw["rel_step"], kw["abs_step"])
        return [ACSensSolution(views[s], run, kw["params"], s, self.points[lo + s]) for s in range(hi - lo)]

    def tran_arrays(self, tspan, abstol=1e-6, reltol=1e-3, dc_abstol=1e-10, saveat=None, ctx=None, **kw):
        """This rank's share of the sweep as ONE batched transient, results as arrays instead of per-point Solutions: the shape
        the result gather of a sharded sweep moves (`gather_sharded`).  Returns (rc, t[n_save],
        rows[samples, n_obs, n_save], stats); observables in the order of `builder(...).obs`."""
        lo, hi = shard_range(len(self.points), self.rank, self.world)
        _, eng, _, _ = self._engine(lo, hi, ctx)
        opts = tran_opts(abstol=abstol, reltol=reltol, saveat=saveat, dc=dc_opts(abstol=dc_abstol), **kw)
        rc, t, v, xf, st = eng.tran(tspan[0], tspan[1], opts)
        self._last_engine = eng   # st["device_rows"] (the same rows still in HBM, [n_obs][n_times][samples]) lives as long as this circuit
        return rc, t, np.ascontiguousarray(np.transpose(v, (2, 0, 1))), st


def gather_sharded_device(rows, n_total, rank, world, group=None):
    """The same gather with the rows never leaving HBM: `rows` is a CUDA tensor [n_obs, n_times, n_local] (samples fastest — the
    engine's own layout, e.g. `torch.as_tensor(stats["device_rows"], device="cuda")`); one `all_gather` over RCCL; returns a CUDA
    tensor [n_obs, n_times, n_total] on every rank."""
    import torch
    import torch.distributed as dist
    max_local = -(-n_total // world)
    n_obs, n_t, n_loc = rows.shape
    buf = rows if n_loc == max_local else torch.cat((rows, rows.new_zeros((n_obs, n_t, max_local - n_loc))), dim=2)
    buf = buf.contiguous()
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf, group=group)
    parts = []
    for r in range(world):
        lo, hi = shard_range(n_total, r, world)
        parts.append(out[r][:, :, :hi - lo])
    return torch.cat(parts, dim=2)


def gather_sharded(local, n_total, rank, world, group=None, device=None):
    """All-gather per-rank result rows (one collective at the end, none in the Newton
    loop).  `local` is a float64 array [n_local, ...] for this rank's contiguous shard; returns the
    full [n_total, ...] array on every rank.  Backend nccl (= RCCL over xGMI) needs `device='cuda'`."""
    import torch
    import torch.distributed as dist
    local = np.ascontiguousarray(local, dtype=np.float64)
    tail = local.shape[1:]
    width = int(np.prod(tail)) if tail else 1
    max_rows = -(-n_total // world)
    buf = torch.zeros((max_rows, width), dtype=torch.float64, device=device or "cpu")
    if local.shape[0]:
        buf[:local.shape[0]] = torch.from_numpy(local.reshape(local.shape[0], width)).to(buf.device)
    out = [torch.zeros_like(buf) for _ in range(world)]
    dist.all_gather(out, buf, group=group)
    rows = []
    for r in range(world):
        lo, hi = shard_range(n_total, r, world)
        rows.append(out[r][:hi - lo].cpu().numpy())
    return np.concatenate(rows, axis=0).reshape((n_total,) + tuple(tail))
