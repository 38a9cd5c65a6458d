"""What the analyses of api.py share between one circuit and a sweep of them: the request record a front function resolves its
arguments into, the engine set-up (one circuit as one sample; sweep points lo..hi as the samples of one engine circuit), one
solve-and-wrap function per analysis, `CircuitSweep`, and the result gathers of a sharded sweep."""
import copy
import warnings
from typing import NamedTuple

import numpy as np

from .circuit import DEV_L, DEV_V, DEV_VCVS, CedarError, Circuit, dc_opts, tran_opts
from .engine import Context, EngineCircuit, default_context
from .acmeasure import mna_rows, net_rows, resolve_fmeasures
from .measure import resolve_measures
from .solution import (ACMeasured, ACSensRun, ACSensSolution, LoopGainSolution, MeasureSens, NetParamsSolution, NoiseRun, NoiseSensRun, NoiseSensSolution, NoiseSolution, SensSolution, Solution, TranSensSolution, _failure, _nothing_to_hand_out,
                       _param_columns, dc_solution, need_ac_source)
from .sweepmap import learn_batch, sample_view
from .sweeps import shard_range, sweepify

_DC_KEYWORDS = ("abstol", "maxiters", "n_restarts", "seed", "tran_mode")


def dc_keywords(given):
    """The DC options among a front function's arguments (its `locals()`), as `dc_opts` takes them."""
    return {k: given[k] for k in _DC_KEYWORDS if k in given}


class Request(NamedTuple):
    """What one call of an analysis asks for, resolved once: read by the single-circuit path and by every group of a sweep."""
    kind: str                 # "dc" | "tran" | "ac" | "noise" | "dc_sens" | "ac_sens" | "tran_sens" | "noise_sens"
    dc: dict                  # keywords of dc_opts, without x0
    tran: dict = None         # keywords of tran_opts without dc and skip_dc, or None
    tspan: tuple = None
    params: tuple = ()        # sensitivity parameters, as Circuit.slot takes them
    rel_step: float = None
    abs_step: object = None
    device_noise: bool = False   # noise, noise_sens: the BSIM4 MOSFETs' own sources too (ch_noise_ex)
    measures: tuple = ()         # tran, tran_sens: waveform measurements (measure.py), taken on the GPU before the result is handed out
    freqs_hz: tuple = ()         # ac_measure, loop_gain: the frequency grid (their measures, of acmeasure.py, are in `measures`)
    probe: object = None         # loop_gain: the name of the voltage source in the loop wire; net_params: the tuple of the ports' names, port 1 first
    z0: tuple = ()               # net_params: the reference impedance of every port

    @property
    def dc_abstol(self):
        """The DC tolerance of this request."""
        return self.dc.get("abstol", 1e-10)

    def dc_opts(self, x0=None):
        return dc_opts(x0=x0, **self.dc)

    def tran_opts(self, x0=None, skip_dc=False):
        return tran_opts(dc=self.dc_opts(x0), skip_dc=skip_dc, **self.tran)


def tran_request(tspan, dc_abstol, tranop, tran_kw, measures=None):
    return Request("tran", dict(abstol=dc_abstol, tran_mode=tranop), tran_kw, tspan, measures=tuple(measures or ()))


def sens_request(kind, params, given):
    return Request(kind, dc_keywords(given), params=tuple(params), rel_step=given["rel_step"], abs_step=given["abs_step"],
                   device_noise=bool(given.get("device_noise", False)))


def ac_measure_request(measures, freqs_hz, params, given):
    return Request("ac_measure", dc_keywords(given), params=tuple(params), rel_step=given["rel_step"], abs_step=given["abs_step"], measures=tuple(measures),
                   freqs_hz=tuple(float(f) for f in np.asarray(freqs_hz, dtype=np.float64).reshape(-1)))


def loop_gain_request(probe, freqs_hz, params, measures, given):
    return ac_measure_request(measures, freqs_hz, params, given)._replace(kind="loop_gain", probe=str(probe).lower())


def net_params_request(ports, freqs_hz, z0, params, measures, given):
    """The ports as a tuple of names and one reference impedance per port (a scalar `z0` serves every port)."""
    ports = (ports,) if isinstance(ports, str) else tuple(ports)
    z = np.asarray(z0, dtype=np.float64).reshape(-1)
    if len(z) == 1:
        z = np.repeat(z, len(ports))
    if len(z) != len(ports):
        raise CedarError("net_params: %d reference impedances for %d ports" % (len(z), len(ports)))
    return ac_measure_request(measures, freqs_hz, params, given)._replace(kind="net_params", probe=tuple(str(p).lower() for p in ports), z0=tuple(float(v) for v in z))


def tran_sens_request(params, tspan, dc_abstol, tranop, tran_kw, rel_step, abs_step, measures=None):
    return Request("tran_sens", dict(abstol=dc_abstol, tran_mode=tranop), tran_kw, tspan, tuple(params), rel_step, abs_step, measures=tuple(measures or ()))


# ---- engine set-up ------------------------------------------------------------------------------------------------------------------
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


class Batch(NamedTuple):
    """An engine circuit with its samples set.  A single circuit is a batch of one without points."""
    ckt: Circuit
    eng: EngineCircuit
    slot_ids: list            # the slots a sweep learned, and
    vals: np.ndarray          # their values[slot][sample]
    views: list               # per sample: the circuit with that sample's device parameters (post-processing such as R.I = V/r reads them)
    ids: list                 # slot ids of the requested sensitivity parameters
    points: list = None       # per sample: the sweep point
    probe: object = None      # loop_gain: the device index of the probe; net_params: the list of the ports' device indices


def _probe_excitation(ckt, probe):
    """(the circuit record with |ac| = 1 on the probe's source and 0 on every other one, the probe's device index).  An AC-driven
    voltage source is the only kind the engine's structural analysis never folds into a known node or merges away, so this is how a
    loop-gain probe reaches it; the user's own `ac=` magnitudes play no part.  The record is a shallow copy: only `source_ac` differs."""
    if isinstance(probe, tuple):   # net_params: every port is excited; the engine solves one column per port
        for p in probe:
            if p not in ckt.dev_names:
                raise CedarError("net_params: unknown port '%s'" % p)
        devs = [ckt.dev_names.index(p) for p in probe]
    else:
        if probe not in ckt.dev_names:
            raise CedarError("loop_gain: unknown probe '%s'" % probe)
        devs = [ckt.dev_names.index(probe)]
    view = copy.copy(ckt)
    view.source_ac = [0.0] * len(ckt.source_ac)
    for i in devs:
        if ckt.dev_kind[i] == DEV_V:   # (anything else is refused by the engine, which names the device)
            view.source_ac[ckt.dev_ipar[i][0]] = 1.0
    return view, devs if isinstance(probe, tuple) else devs[0]


def _engine_of(ckt, ctx, params, small_signal, ac_source, probe=None):
    """(slot ids of `params`, engine circuit, device index of the loop-gain probe or None).  The slots are declared before the engine
    circuit is built from the description."""
    if ac_source:
        need_ac_source(ckt)
    ids = [_slot_of(ckt, p) for p in params]
    if probe is None:
        return ids, EngineCircuit(ckt, ctx, small_signal=small_signal), None
    view, dev = _probe_excitation(ckt, probe)
    return ids, EngineCircuit(view, ctx, small_signal=True), dev


def single(circuit, ctx, observe=None, params=(), small_signal=False, ac_source=False, probe=None):
    ckt = _prepare(circuit, observe)
    ids, eng, dev = _engine_of(ckt, ctx, params, small_signal, ac_source, probe)
    return Batch(ckt, eng, [], None, [ckt], ids, probe=dev)


# ---- solve and wrap: (a batch of S samples, the request) -> S solutions ------------------------------------------------------------------
def _point(b, s):
    return b.points[s] if b.points else None


def solve_dc(b, req, x0=None):
    """A single circuit's Solution carries the call's rc, and its failure warns; a sweep's samples carry their own status."""
    rc, x, status, st = b.eng.dc(req.dc_opts(x0))
    if b.points is None:
        if rc != 0:
            warnings.warn("DC operating point analysis failed. Further failures may follow.")  # src/dcop.jl:141
        return [dc_solution(b.ckt, x[0], rc, st)]
    return [dc_solution(b.views[s], x[s], int(status[s]), st, b.points[s]) for s in range(b.eng.n_samples)]


def _measure_kw(b, req, with_sens=False):
    """The engine call's `measures=` of a request that asks for some (and nothing at all of one that does not: the call is the parent's)."""
    if not req.measures:
        return None, {}
    names, specs = resolve_measures(b.ckt, req.measures, b.views, with_sens)
    return names, {"measures": (len(names), specs)}


def _hand_out_measures(sols, names, st, params=()):
    """`sol.measures[name]`, `sol.measure_status[name]` and, with sensitivities, `sol.measure_sens[name, par]` of every sample."""
    if names is None:
        return sols
    val, status, sens = st.pop("measures")
    cols = _param_columns(params)
    for s, sol in enumerate(sols):
        sol.measures = {n: float(val[k, s]) for k, n in enumerate(names)}
        sol.measure_status = {n: int(status[k, s]) for k, n in enumerate(names)}
        if params:
            sol.measure_sens = MeasureSens(names, cols, sens[:, :, s] if sens is not None else np.full((len(names), len(params)), np.nan))
    return sols


def solve_tran(b, req, x0=None, skip_dc=False):
    """One Solution per sample of a batched transient: observable k of sample s is v[k, :, s]."""
    names, mkw = _measure_kw(b, req)
    rc, t, v, xf, st = b.eng.tran(req.tspan[0], req.tspan[1], req.tran_opts(x0, skip_dc), **mkw)
    return _hand_out_measures([Solution(b.views[s], t, {o: (v[k, :, s] if v.size else np.zeros(0)) for k, o in enumerate(b.ckt.obs)},
                                        xf[s] if xf is not None else None, rc, st, _point(b, s)) for s in range(b.eng.n_samples)], names, st)


def solve_dc_sens(b, req, x0=None):
    rc, x, sens, status, st = b.eng.dc_sens(b.ids, req.dc_opts(x0), rel_step=req.rel_step, abs_step=req.abs_step)
    if _nothing_to_hand_out(rc, status):
        raise _failure("DC sensitivity analysis", rc, b.eng)
    return [SensSolution(b.views[s], req.params, sens[s], dc_solution(b.views[s], x[s], int(status[s]), st, _point(b, s)), int(status[s]))
            for s in range(b.eng.n_samples)]


def solve_tran_sens(b, req, x0=None, skip_dc=False):
    """One TranSensSolution per sample of a batched ch_tran_sens: observable k of sample s is v[k, :, s], its derivatives sens[k, :, :, s].
    A refusal (an unsupported slot, a bad option) leaves nothing to hand out and raises."""
    names, mkw = _measure_kw(b, req, with_sens=True)
    rc, t, v, xf, st, sens = b.eng.tran_sens(req.tspan[0], req.tspan[1], b.ids, req.tran_opts(x0, skip_dc), rel_step=req.rel_step, abs_step=req.abs_step, **mkw)
    if len(t) == 0 and rc != 0:
        raise _failure("transient sensitivity analysis", rc, b.eng)
    return _hand_out_measures([TranSensSolution(b.views[s], t, {o: v[k, :, s] for k, o in enumerate(b.ckt.obs)}, xf[s] if xf is not None else None, rc, st,
                                                _point(b, s), req.params, {o: sens[k, :, :, s] for k, o in enumerate(b.ckt.obs)})
                               for s in range(b.eng.n_samples)], names, st, req.params)


def solve_ac_sens(b, req):
    """Nothing is solved yet: the samples share a run object that solves per frequency list when one of them is asked."""
    run = ACSensRun(b.eng, req.dc, b.ids, req.rel_step, req.abs_step)
    return [ACSensSolution(b.views[s], run, req.params, s, _point(b, s)) for s in range(b.eng.n_samples)]


def solve_ac_measure(b, req):
    """One ACMeasured per sample of one ch_ac_measure: the analysis and its measures stay in HBM; values, statuses and the measures'
    derivatives come back.  The specs are checked against the MNA rows before anything is solved; a sample without an operating
    point has status 5 and NaN while the others are served; a refusal raises."""
    res = resolve_fmeasures(req.measures, mna_rows(b.ckt))
    if not res.names:
        raise CedarError("ac_measure: at least one measure")
    rc, val, status, sens, sample_status, st = b.eng.ac_measure(b.ids, req.freqs_hz, res.specs, len(res.names), req.dc_opts(), rel_step=req.rel_step, abs_step=req.abs_step)
    if _nothing_to_hand_out(rc, sample_status if b.ids else np.full(b.eng.n_samples, rc)):
        raise _failure("AC measurement", rc, b.eng)
    val, sens = res.apply(val, sens)
    return [ACMeasured(b.views[s], res.names, val[:, s], status[:, s], sens[:, :, s] if sens is not None else None, req.params, int(sample_status[s]), st, _point(b, s))
            for s in range(b.eng.n_samples)]


def _loop_gain_rows(sym, name):
    """`row_of` of a loop-gain analysis: its one row is named by the reserved symbol "T"."""
    if isinstance(sym, str) and sym.lower() == "t":
        return 0, -1, 1.0
    raise CedarError("measure '%s': a loop-gain measure reads the row \"T\", not %r" % (name, sym))


def solve_loop_gain(b, req):
    """One LoopGainSolution per sample of one ch_loop_gain: T, dT/dp and the measures of T, taken in HBM.  A sample without an
    operating point has NaN rows, measure status 5 and its status in `rc` while the others are served; a refusal raises."""
    res = resolve_fmeasures(req.measures, _loop_gain_rows) if req.measures else None
    names = res.names if res else []
    rc, T, dT, val, status, sens, sample_status, st = b.eng.loop_gain(b.probe, req.freqs_hz, b.ids, res.specs if res else None, len(names), req.dc_opts(),
                                                                       rel_step=req.rel_step, abs_step=req.abs_step)
    if _nothing_to_hand_out(rc, sample_status):
        raise _failure("loop gain analysis (probe '%s')" % req.probe, rc, b.eng)
    if res:
        val, sens = res.apply(val, sens)
    return [LoopGainSolution(b.views[s], req.probe, req.freqs_hz, T[s], dT[s] if dT is not None else None, req.params, names, val[:, s], status[:, s],
                             sens[:, :, s] if sens is not None else None, int(sample_status[s]), st, _point(b, s)) for s in range(b.eng.n_samples)]


def solve_net_params(b, req):
    """One NetParamsSolution per sample of one ch_net_params: S, Y, Z, their derivatives and the measures of their entries, taken in
    HBM.  A sample without an operating point has NaN rows, measure status 5 and its status in `rc` while the others are served; a
    refusal raises."""
    P = len(req.probe)
    res = resolve_fmeasures(req.measures, net_rows(P)) if req.measures else None
    names = res.names if res else []
    rc, X, dX, val, status, sens, sample_status, st = b.eng.net_params(b.probe, req.z0, req.freqs_hz, b.ids, res.specs if res else None, len(names), req.dc_opts(),
                                                                       rel_step=req.rel_step, abs_step=req.abs_step)
    if _nothing_to_hand_out(rc, sample_status):
        raise _failure("network analysis (ports %s)" % ", ".join("'%s'" % p for p in req.probe), rc, b.eng)
    if res:
        val, sens = res.apply(val, sens)
    return [NetParamsSolution(b.views[s], req.probe, req.z0, req.freqs_hz, {k: v[s] for k, v in X.items()}, {k: v[s] for k, v in dX.items()} if dX else None, req.params, names,
                              val[:, s], status[:, s], sens[:, :, s] if sens is not None else None, int(sample_status[s]), st, _point(b, s)) for s in range(b.eng.n_samples)]


def solve_noise_sens(b, req):
    """Nothing is solved yet: the samples share a run object that solves per (output, frequency list) when one of them is asked."""
    run = NoiseSensRun(b.ckt, b.eng, req.dc, b.ids, req.rel_step, req.abs_step, req.device_noise)
    return [NoiseSensSolution(b.views[s], run, req.params, s, _point(b, s)) for s in range(b.eng.n_samples)]


def solve_noise(b, req):
    """Nothing is solved yet: the samples share a run object that solves per (output, frequency list) when one of them is asked."""
    run = NoiseRun(b.eng, req.dc_opts(), req.device_noise)
    return [NoiseSolution(b.views[s], b.eng, run.opts, req.device_noise, run, s, _point(b, s)) for s in range(b.eng.n_samples)]


class _Kind(NamedTuple):
    solve: object
    warm: bool = False            # a warm start applies (the sensitivity analyses start every sample cold)
    small_signal: bool = False    # the engine circuit keeps the sources' AC magnitudes
    ac_source: bool = False       # ... and there must be one


_KINDS = {"dc": _Kind(solve_dc, warm=True), "tran": _Kind(solve_tran, warm=True), "dc_sens": _Kind(solve_dc_sens),
          "ac_sens": _Kind(solve_ac_sens, small_signal=True, ac_source=True), "ac_measure": _Kind(solve_ac_measure, small_signal=True, ac_source=True), "tran_sens": _Kind(solve_tran_sens),
          "noise": _Kind(solve_noise, small_signal=True), "noise_sens": _Kind(solve_noise_sens, small_signal=True),
          "loop_gain": _Kind(solve_loop_gain, small_signal=True), "net_params": _Kind(solve_net_params, small_signal=True)}


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

    def _engine(self, lo, hi, ctx, params=(), small_signal=False, views=True, ac_source=False, probe=None):
        """Points lo..hi as the samples of one engine circuit.  `views=False` leaves the per-sample circuits out (a caller that hands
        out arrays, not Solutions, has no use for them)."""
        base, slot_ids, vals = self._batch(lo, hi)
        ckt = _prepare(base, None)
        each = [sample_view(ckt, vals, s) for s in range(hi - lo)] if views else None   # before `params` add slots that `vals` has no row for
        ids, eng, dev = _engine_of(ckt, ctx, params, small_signal, ac_source=ac_source, probe=probe)
        eng.set_samples(hi - lo)
        if slot_ids:
            eng.set_params(slot_ids, vals)
        return Batch(ckt, eng, slot_ids, vals, each, ids, self.points[lo:hi], dev)

    def _run(self, req, ctx):
        """This rank's share of the sweep, in sweep order.  u0 and observe of the front functions do not reach a sweep."""
        lo, hi = shard_range(len(self.points), self.rank, self.world)
        if hi <= lo:
            return []
        n = hi - lo
        G = (4 if n >= 4096 else 2 if n >= 2048 else 1) if self.groups == "auto" else min(self.groups, n)
        if G <= 1:
            return self._run_range(req, ctx, lo, hi)
        from concurrent.futures import ThreadPoolExecutor
        first = ctx if ctx is not None else default_context()
        ctxs = [first] + [Context(first.device_id) for _ in range(G - 1)]

        def work(g):
            a, b = shard_range(hi - lo, g, G)
            return self._run_range(req, ctxs[g], lo + a, lo + b)

        with ThreadPoolExecutor(G) as ex:
            parts = list(ex.map(work, range(G)))
        return [sol for part in parts for sol in part]

    def _run_range(self, req, ctx, lo, hi):
        kind = _KINDS[req.kind]
        b = self._engine(lo, hi, ctx, req.params, kind.small_signal, ac_source=kind.ac_source, probe=req.probe)
        if not (kind.warm and self.warm_start and hi - lo > 1):
            return kind.solve(b, req)
        e0 = EngineCircuit(_prepare(self._build(**self.points[lo]), None), ctx)
        rc0, xw, _, _ = e0.dc(dc_opts(abstol=req.dc_abstol))
        return kind.solve(b, req, np.tile(np.nan_to_num(xw[0]), (hi - lo, 1)) if rc0 == 0 else None)

    def dc_sens(self, params, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, tran_mode=False, rel_step=None, abs_step=None, ctx=None):
        """Sensitivities of every sweep point with respect to `params`: one batched ch_dc_sens per sample group (the batching and
        sharding of `_run`); a list of SensSolution in sweep order, each differentiated at its own parameter point."""
        return self._run(sens_request("dc_sens", params, locals()), ctx)

    def ac_sens(self, params, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
        """AC sensitivities of every sweep point with respect to `params`: one batched ch_ac_sens per sample group and frequency list
        (the batching and sharding of `_run`); a list of ACSensSolution in sweep order, each differentiated at its own point."""
        return self._run(sens_request("ac_sens", params, locals()), ctx)

    def ac_measure(self, measures, freqs_hz, params=(), abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
        """Frequency-domain measurements (acmeasure.py) of every sweep point and their derivatives with respect to `params`: one batched
        ch_ac_measure per sample group; a list of ACMeasured in sweep order."""
        return self._run(ac_measure_request(measures, freqs_hz, params, locals()), ctx)

    def loop_gain(self, probe, freqs_hz, params=(), measures=(), abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
        """Loop gain at the probe, its derivatives with respect to `params` and the measures of it (acmeasure.py, on the row "T") for
        every sweep point: one batched ch_loop_gain per sample group; a list of LoopGainSolution in sweep order."""
        return self._run(loop_gain_request(probe, freqs_hz, params, measures, locals()), ctx)

    def net_params(self, ports, freqs_hz, z0=50.0, params=(), measures=(), abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
        """S, Y and Z parameters seen from `ports`, their derivatives with respect to `params` and the measures of their entries
        (acmeasure.py, on the rows "s21", "y11", ...) for every sweep point: one batched ch_net_params per sample group; a list of
        NetParamsSolution in sweep order."""
        return self._run(net_params_request(ports, freqs_hz, z0, params, measures, locals()), ctx)

    def noise_sens(self, params, device_noise=False, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
        """Noise PSD sensitivities of every sweep point with respect to `params`: one batched ch_noise_sens per sample group, output and
        frequency list (the batching and sharding of `_run`); a list of NoiseSensSolution in sweep order, each differentiated at its own point."""
        return self._run(sens_request("noise_sens", params, locals()), ctx)

    def tran_arrays(self, tspan, abstol=1e-6, reltol=1e-3, dc_abstol=1e-10, saveat=None, ctx=None, **kw):
        """This rank's share of the sweep as ONE batched transient, results as arrays instead of per-point Solutions: the shape
        the result gather of a sharded sweep moves (`gather_sharded`).  Returns (rc, t[n_save],
        rows[samples, n_obs, n_save], stats); observables in the order of `builder(...).obs`."""
        req = tran_request(tspan, dc_abstol, False, dict(abstol=abstol, reltol=reltol, saveat=saveat, **kw))
        lo, hi = shard_range(len(self.points), self.rank, self.world)
        eng = self._engine(lo, hi, ctx, views=False).eng
        rc, t, v, xf, st = eng.tran(tspan[0], tspan[1], req.tran_opts())
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
