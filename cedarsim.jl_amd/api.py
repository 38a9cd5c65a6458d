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
    ac_measure(circuit, measures, freqs_hz, params) → ACMeasured.measures[name], .measure_sens[name, par]  ≙ .measure ac cards (ngspice), per sample, in HBM
    ac_sens(circuit, params) → ACSensSolution.freqresp(sym, ωs), .sens(sym, par, ωs)  ≙ d(freqresp(ac, sym, ωs))/dp (ngspice: .sens … ac)
    noise_sens(circuit, params) → NoiseSensSolution.psd(sym, ωs), .sens(sym, par, ωs)  ≙ d(PSD(noise, sym, ωs))/dp
    tran_sens(circuit, params, tspan) → TranSensSolution.sens["node_out", "r1"]  ≙ ODEForwardSensitivityProblem over tspan  test/sensitivity.jl
    loop_gain(circuit, probe, freqs_hz, params, measures) → LoopGainSolution.T, .sens[par], .measures[name]  ≙ a stability (.stb) analysis at a probe, the loop closed
    net_params(circuit, ports, freqs_hz, z0, params, measures) → NetParamsSolution.S, .Y, .Z, .sens_S[par], .measures[name]  ≙ an N-port (.net / S-parameter) analysis at voltage-source ports

The reference loops serially over sweep points, paying a full DC + transient each
(`broadcast(sims) do sim … remake(prob, p=sim)`, src/sweeps.jl:473-480).  Here every point becomes one
*sample* of a single batched GPU solve (`ch_set_params` + one `ch_dc`/`ch_tran`); with several ranks
the points are split into contiguous shards, one per GPU, and results are gathered at the end.
All numerics run in libcedarhip.so; nothing here computes a circuit solution.
"""
import math

import numpy as np

from .batch import (CircuitSweep, Request, ac_measure_request, dc_keywords, gather_sharded, gather_sharded_device, loop_gain_request, net_params_request, sens_request, single, solve_ac_measure,  # noqa: F401
                    solve_ac_sens, solve_loop_gain, solve_net_params, solve_noise_sens, solve_dc, solve_dc_sens, solve_tran, solve_tran_sens, tran_request, tran_sens_request)
from .circuit import CedarError, Circuit
from .solution import ACMeasured, ACSensSolution, ACSolution, LoopGainSolution, NetParamsSolution, NoiseSensSolution, NoiseSolution, SensSolution, Solution, TranSensSolution, mag_phase_sens  # noqa: F401


def dc(circuit, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, tran_mode=False, u0=None, observe=None, ctx=None):
    """DC operating point (CedarDCOp: sources at their .dc value, du = 0; src/dcop.jl:157-200)."""
    req = Request("dc", dc_keywords(locals()))
    if isinstance(circuit, CircuitSweep):
        return circuit._run(req, ctx)
    return solve_dc(single(circuit, ctx, observe), req, u0)[0]


def _netlist_tspan(circuit):
    """(0, tstop) of the `.TRAN` statement of a parsed netlist, or of the netlist a circuit was built from (src/circsummary.jl:109-128)."""
    nl = circuit if hasattr(circuit, "tran") and not isinstance(circuit, Circuit) else getattr(circuit, "_netlist", None)
    if nl is None or nl.tran is None:
        raise CedarError("no tspan given and the netlist has no .TRAN statement")
    return (0.0, nl.tran[1])


def tran(circuit, tspan=None, abstol=1e-6, reltol=1e-3, u0=None, initializealg="dcop", dc_abstol=1e-10, saveat=None,
         max_order=5, observe=None, ctx=None, measures=None, **kw):
    """Transient (solve(prob, IDA(); abstol, reltol, initializealg=CedarDCOp()), src/sweeps.jl:450-465).

    u0: MNA initial state → skips the DC solve (test/common.jl:36-43 `u0=` semantics).
    tspan defaults to the netlist's `.TRAN` (src/circsummary.jl:109-128).
    measures: waveform measurements (measure.py: `when`, `delay`, ..., `parse_measure`), evaluated on the GPU for every sample before
    the rows are handed out: `sol.measures[name]`, `sol.measure_status[name]`."""
    sweep = isinstance(circuit, CircuitSweep)
    if tspan is None and not sweep:
        tspan = _netlist_tspan(circuit)
    req = tran_request(tspan, dc_abstol, initializealg == "tranop", dict(abstol=abstol, reltol=reltol, saveat=saveat, max_order=max_order, **kw), measures)
    if sweep:
        return circuit._run(req, ctx)
    x0 = None if u0 is None else np.asarray(u0, float)[None, :]
    return solve_tran(single(circuit, ctx, observe), req, x0, skip_dc=u0 is not None)[0]


def acdec(nd, fstart, fstop):
    """`.ac dec nd fstart fstop`: log-spaced frequencies in Hz (src/ac.jl:317-322)."""
    a, b = math.log10(fstart), math.log10(fstop)
    points = int(math.ceil((b - a) * nd)) + 1
    return 10.0 ** np.linspace(a, b, points)


def ac(circuit, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, ctx=None):
    """ac!(circ): DC operating point + linearisation; sample it with `.freqresp(sym, ωs)`."""
    req = Request("ac", dc_keywords(locals()))
    b = single(circuit, ctx, small_signal=True, ac_source=True)
    return ACSolution(b.ckt, b.eng, req.dc_opts())


def noise(circuit, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, ctx=None, device_noise=False):
    """noise!(circ): the thermal noise of the resistors and the sources of compiled modules referred to an output with
    `.psd(sym, ωs)`.  device_noise=True adds the BSIM4 MOSFETs' channel thermal and flicker noise (ch_noise_ex); the solution then
    also breaks the PSD down per source (`.contributions`) and per device (`.summary`)."""
    if isinstance(circuit, CircuitSweep):   # a list, one NoiseSolution per point, out of one batched analysis per (output, frequency list)
        return circuit._run(Request("noise", dc_keywords(locals()), device_noise=bool(device_noise)), ctx)
    req = Request("noise", dc_keywords(locals()))
    b = single(circuit, ctx, small_signal=True)
    return NoiseSolution(b.ckt, b.eng, req.dc_opts(), device_noise)


def dc_sens(circuit, params, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, tran_mode=False, u0=None, rel_step=None, abs_step=None, ctx=None):
    """DC operating point and d(solution)/d(parameter) for every name in `params` ("r1", ("m1", "w"), ("nfet_06v0", "vth0"), "temp",
    "gmin": what `Circuit.slot` takes) — the forward sensitivities of test/sensitivity.jl, by the direct method on the GPU."""
    req = sens_request("dc_sens", params, locals())
    if isinstance(circuit, CircuitSweep):
        return circuit._run(req, ctx)
    x0 = None if u0 is None else np.asarray(u0, float)[None, :]
    return solve_dc_sens(single(circuit, ctx, params=params), req, x0)[0]


def ac_sens(circuit, params, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
    """ac!(circ) and d(response)/d(parameter) for every name in `params` (what `Circuit.slot` takes, as for dc_sens): an
    ACSensSolution.  A CircuitSweep gives a list, one per point, out of one batched solve."""
    req = sens_request("ac_sens", params, locals())
    if isinstance(circuit, CircuitSweep):
        return circuit._run(req, ctx)
    return solve_ac_sens(single(circuit, ctx, params=params, small_signal=True, ac_source=True), req)[0]


def ac_measure(circuit, measures, freqs_hz, params=(), abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
    """ac!(circ) on the grid `freqs_hz` (Hz, strictly increasing) and the frequency-domain measurements `measures` (acmeasure.py:
    `bandwidth`, `unity_gain_freq`, `phase_margin`, `gain_margin`, `fwhen`, ..., `parse_ac_measure`) of it, evaluated on the GPU where
    the solve left its result, with their exact derivatives with respect to every name in `params` (what `Circuit.slot` takes): an
    ACMeasured with `.measures[name]`, `.measure_status[name]`, `.measure_sens[name, par]`.  A CircuitSweep gives a list, one per
    point, out of one batched solve."""
    req = ac_measure_request(measures, freqs_hz, params, locals())
    if isinstance(circuit, CircuitSweep):
        return circuit._run(req, ctx)
    return solve_ac_measure(single(circuit, ctx, params=params, small_signal=True, ac_source=True), req)[0]


def loop_gain(circuit, probe, freqs_hz, params=(), measures=(), abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
    """Stability analysis: the loop gain T(f) of the CLOSED loop on the grid `freqs_hz` (Hz), measured at `probe`, with the bias kept.
    `probe` names an independent voltage source `vprobe x y` (DC value normally 0) inserted in the loop wire: terminal x (+) faces the
    side the loop signal arrives from, y (-) the side it goes into.  The direction matters: the reversed probe measures the reverse
    loop gain.  T is Tian's loop gain, T = u / (1 - u) with u = V2 - I1 out of two excitations of the linearised circuit (the probe
    at 1 V: V2 = v_x; a unit current into x: I1 = the probe's current), both solved on one factorisation per frequency.
    Every AC excitation but the probe's is off: the circuit reaches the engine with |ac| = 1 on the probe and 0 on every other
    source, so a `vin ... ac=1` of the user's is ignored for this analysis.
    params: names as `Circuit.slot` takes them; `sol.sens[par]` is dT/d(parameter) [n_freq], bias shift included, from two adjoint
    vectors (no solve per parameter).  measures: frequency-domain measures (acmeasure.py) of the reserved symbol "T", e.g.
    `phase_margin("pm", "T")`, `gain_margin("gm", "T")`, `unity_gain_freq("fug", "T")` (the grid then has to be strictly increasing),
    evaluated on the GPU where the rows lie, with their exact derivatives: `sol.measures[name]`, `sol.measure_status[name]`,
    `sol.measure_sens[name, par]`.  Returns a LoopGainSolution; a CircuitSweep gives a list, one per point, out of one batched
    analysis."""
    req = loop_gain_request(probe, freqs_hz, params, measures, locals())
    if isinstance(circuit, CircuitSweep):
        return circuit._run(req, ctx)
    return solve_loop_gain(single(circuit, ctx, params=params, probe=req.probe), req)[0]


def net_params(circuit, ports, freqs_hz, z0=50.0, params=(), measures=(), abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
    """N-port network analysis: the S, Y and Z parameters of the circuit seen from `ports` on the grid `freqs_hz` (Hz), with the bias
    kept.  `ports` names independent voltage sources `vpJ a b` in port order (port 1 first, at most 8); a port's DC value stays, so a
    port may bias a gate.  Run k puts 1 V AC on port k and 0 V on the others, which stay ideal sources (AC shorts); the current
    ENTERING the network at a port's + terminal counts positive, so a resistor R across one port gives Y11 = +1/R.  `z0`: the real,
    positive reference impedance, a scalar or one per port; S = (I - y)(I + y)^-1 with y = sqrt(z0) Y sqrt(z0), Z = Y^-1 (NaN where
    Y is singular, as for a series-only network).  All ports are solved on one factorisation per frequency.
    Every AC excitation but the ports' is off: the circuit reaches the engine with |ac| = 1 on the ports and 0 on every other source.
    params: names as `Circuit.slot` takes them; `sol.sens_S[par]`, `sol.sens_Y[par]`, `sol.sens_Z[par]` are the derivatives
    [n_freq][P][P], bias shift included, from P adjoint vectors (no solve per parameter).  measures: frequency-domain measures
    (acmeasure.py) of the reserved symbols "s21", "y11", "z12" (kind, response port, driven port; case-insensitive), e.g.
    `bandwidth("bw", "s21", ref_at=1e3)`, `db("s11")`, evaluated on the GPU where the rows lie, with their exact derivatives:
    `sol.measures[name]`, `sol.measure_status[name]`, `sol.measure_sens[name, par]`.  Returns a NetParamsSolution
    (`.write_touchstone(path)` saves S); a CircuitSweep gives a list, one per point, out of one batched analysis."""
    req = net_params_request(ports, freqs_hz, z0, params, measures, locals())
    if isinstance(circuit, CircuitSweep):
        return circuit._run(req, ctx)
    return solve_net_params(single(circuit, ctx, params=params, probe=req.probe), req)[0]


def noise_sens(circuit, params, device_noise=False, abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None, ctx=None):
    """noise!(circ) and d(PSD)/d(parameter) for every name in `params` (what `Circuit.slot` takes, as for dc_sens), by the direct
    method on the adjoint system: a NoiseSensSolution (`.psd`, `.sens`, `.log_sens`, `.integrated`, `.integrated_sens`).  device_noise
    as for `noise`.  A CircuitSweep gives a list, one per point, out of one batched solve per (output, frequency list)."""
    req = sens_request("noise_sens", params, locals())
    if isinstance(circuit, CircuitSweep):
        return circuit._run(req, ctx)
    return solve_noise_sens(single(circuit, ctx, params=params, small_signal=True), req)[0]


def tran_sens(circuit, params, tspan=None, abstol=1e-6, reltol=1e-3, u0=None, initializealg="dcop", dc_abstol=1e-10, saveat=None, max_order=5,
              rel_step=None, abs_step=None, observe=None, ctx=None, measures=None, **kw):
    """tran!(circ, tspan) and d(observable)(t)/d(parameter) along the waveform for every name in `params` (what `Circuit.slot` takes,
    as for dc_sens) — the ODEForwardSensitivityProblem of test/sensitivity.jl, by the direct method at every accepted step of the host
    stepper: a TranSensSolution (`sol.sens["node_out", ("m1", "w")]`, `sol.sens(t, idxs=…, par=…)`).  The step sequence is held fixed,
    so this is the derivative of the discrete solution the run computed.  A CircuitSweep gives a list out of one batched solve.
    measures: as for `tran`; every measure also gets its exact derivatives with respect to `params`: `sol.measure_sens[name, par]`."""
    sweep = isinstance(circuit, CircuitSweep)
    if tspan is None and not sweep:
        tspan = _netlist_tspan(circuit)
    req = tran_sens_request(params, tspan, dc_abstol, initializealg == "tranop", dict(abstol=abstol, reltol=reltol, saveat=saveat, max_order=max_order, **kw),
                            rel_step, abs_step, measures)
    if sweep:
        return circuit._run(req, ctx)
    x0 = None if u0 is None else np.asarray(u0, float)[None, :]
    return solve_tran_sens(single(circuit, ctx, observe, params=params), req, x0, skip_dc=u0 is not None)[0]
