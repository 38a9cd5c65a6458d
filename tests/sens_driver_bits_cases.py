"""Cases and the one runner shared by tests/test_gpu_sens_driver_bits.py and tests/golden/make_sens_driver_bits.py: the host drivers of the
sensitivity family (csrc/ch_engine_sens.hpp, ch_engine_noisesens.hpp, ch_engine_transens.hpp, ch_engine_ac.hpp, ch_engine_fmeasure.hpp,
ch_engine_loopgain.hpp), every one on its path up to 96 unknowns and on its global-workspace path above.  The circuits are those of the drivers' own GPU tests.

  dc_amp3            amplifier x 3 samples at their own rd, m1.w; slots: device parameter, source DC value, gmin, multiplier
  dc_chunks          resistor ladder of 80 unknowns, 160 slots: more right-hand sides than one LDS chunk
  dc_ladder97        resistor ladder of 97 unknowns: global workspace
  dc_failed          3 samples, the middle one without an operating point
  ac_amp, _sparse    amplifier (state term active), fused and with CEDARHIP_FORCE_SPARSE=1
  ac_ladder96, 97    R-L-C ladders either side of the LDS limit
  ac_chunks          chunk_ladder: 302 unknowns x 2 samples x 400 frequencies, two launches of the complex solve
  ac_rlc             series R-L-C: G and C do not depend on x, the state term is skipped
  ac_failed          2 samples, the second without an operating point
  ac_plain_*         ch_ac itself on the amplifier and the ladder of 97
  noise_plain_*      ch_noise itself on the amplifier and the ladder of 97; noise_ex_amp: ch_noise_ex with MOSFET noise and contributions
  noise_amp_mos      amplifier at the drain with the MOSFETs' own noise
  noise_shared       two MOSFETs of one class, slot ma.w: the extra row of the noise-parameter table
  noise_held         an output held by a source: zeros, dc_sens served
  noise_ladder97     global workspace
  noise_chunks       chunk_ladder at n40: two launches
  noise_failed       2 samples, the second without an operating point; noise_failed_held: the same at ground
  tran_rc2, rc97     RC ladders from a zero state (skip_dc), a few steps
  tran_amp           amplifier driven by a PULSE: rd (central), rb1.m (forward), the PULSE's v2 (moves no break point), vdd (central)
  tran_chunks        RC ladder of 96 unknowns, 100 multiplier slots: two column chunks
  tran_skip_dc       RC low-pass behind a SIN from a given state
  acm_amp, _noslots  ch_ac_measure on the amplifier with 3 slots and with none
  acm_ladder97, _noslots  the same above 96 unknowns
  lg_loop4, 96, 97   ch_loop_gain on loopgain_reference.loop(n - 4), the circuit of shape_case(n), with the slots of test_gpu_loop_gain:
                     the adjoint pass, the LDS and the global-workspace solve (97 on the forced sparse path, as in that test), the
                     bilinear kernel
  lg_loop64_noslots, lg_loop97_noslots  T alone: one pass
  lg_amp_measures    the BSIM4 feedback amplifier with its three slots and the three measures on T
  lg_failed          the sweep of test_gpu_loop_gain: 3 samples, the middle one without an operating point, one measure

The lg_ cases are recorded in tests/golden/loopgain_bits.npz (GOLDEN_FILES), every other one in sens_driver_bits.npz.

The record of a case: every output array, every status, `meta` = (return code, unknowns of the circuit, path) and `stats`, the integer
counters of ch_stats in the order of `stats_names` (the timing fields are left out).  An array of more than LIMIT elements is
recorded as the SHA-256 of its bytes (which pins every bit), its shape and every n-th element."""
import hashlib
import math
import os

import numpy as np

from cedarsim_jl_amd import PULSE, Circuit, db, dc_opts, ffind_at, tran_opts

LIMIT = 256
SAMPLES = 32


def _put(rec, key, a):
    a = np.ascontiguousarray(a)
    if a.size <= LIMIT:
        rec[key] = a
        return
    rec[key + "#sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
    rec[key + "#shape"] = np.array(a.shape, np.int64)
    rec[key + "#every"] = a.reshape(-1)[::-(-a.size // SAMPLES)].copy()


def _record(e, rc, st, **arrays):
    rec = {}
    for k, a in arrays.items():
        if a is not None:
            _put(rec, k, a)
    info = e.info()
    rec["meta"] = np.array([rc, info["n_unknowns"], info["path"]], np.int64)
    names = sorted(k for k, v in st.items() if isinstance(v, (int, np.integer)) and not isinstance(v, bool))
    rec["stats"] = np.array([int(st[k]) for k in names], np.int64)
    rec["stats_names"] = np.array(",".join(names))
    if st.get("dense_points") is not None:
        _put(rec, "dense_points", np.asarray(st["dense_points"]))
    return rec


def _small(E):
    return lambda c: E(c, small_signal=True)


def _ids(c, names):
    return [c.slot(*nm) if isinstance(nm, tuple) else c.slot(nm) for nm in names]


def _sparse(fn):
    os.environ["CEDARHIP_FORCE_SPARSE"] = "1"
    try:
        return fn()
    finally:
        del os.environ["CEDARHIP_FORCE_SPARSE"]


def _zero(c, S=1):
    return dc_opts(abstol=1e-12, x0=np.zeros((S, c.n_mna)))


FEW = dict(abstol=1e-12, n_restarts=2, maxiters=5)


def _no_point_cell():
    """rc_cell beside a current source into a resistor that is infinite in one sample"""
    from test_gpu_ac_sens import rc_cell
    c = rc_cell()
    c.I("i1", "n", 0, dc=1e-3)
    c.R("rn", "n", 0, 1e3)
    return c, _ids(c, ["rn", "r1", "c1"])


# ---- ch_dc_sens ----------------------------------------------------------------------------------------------------------------------
def _dc(e, ids, o):
    rc, x, s, status, st = e.dc_sens(ids, o)
    return _record(e, rc, st, x=x, sens=s, status=status)


def dc_amp3(E):
    from test_gpu_ac_noise import amp_circuit
    c = amp_circuit()
    ids = _ids(c, ["rd", ("m1", "w"), "vdd", "gmin", ("rb1", "m")])
    e = E(c)
    e.set_samples(3)
    e.set_params(ids[:2], [[18e3, 20e3, 25e3], [1.8e-6, 2e-6, 2.4e-6]])
    return _dc(e, ids, dc_opts(abstol=1e-12))


def dc_chunks(E):
    from test_gpu_dc_sens import LADDER_ENG, ladder
    c, _, _ = ladder(80)
    ids = _ids(c, ["rs%d" % i for i in range(1, 81)] + ["rp%d" % i for i in range(1, 81)])
    return _dc(E(c), ids, LADDER_ENG(c))


def dc_ladder97(E):
    from test_gpu_dc_sens import LADDER_ENG, ladder
    c, _, _ = ladder(97)
    ids = _ids(c, ["v", "rs1", "rs49", "rs97", "rp1", "rp49", "rp97"])
    return _dc(E(c), ids, LADDER_ENG(c))


def dc_failed(E):
    from test_gpu_dc_sens import divider
    c = divider(observe_branch=False)
    c.I("i1", "a", 0, dc=1e-3)
    c.R("ra", "a", 0, 1e3)
    ids = _ids(c, ["ra", "r1", "v"])
    e = E(c)
    e.set_samples(3)
    e.set_params(ids[:1], [[1e3, math.inf, 2e3]])
    return _dc(e, ids, dc_opts(**FEW))


# ---- ch_ac_sens, ch_ac ----------------------------------------------------------------------------------------------------------------
def _ac(e, ids, f, o):
    rc, x, ds, s, status, st = e.ac_sens(ids, f, o)
    return _record(e, rc, st, x=x, dc_sens=ds, sens=s, status=status)


def ac_amp(E):
    from test_gpu_ac_noise import amp_circuit
    from test_gpu_ac_sens import AMP_FREQS, AMP_SLOTS
    c = amp_circuit()
    ids = _ids(c, AMP_SLOTS)
    return _ac(_small(E)(c), ids, AMP_FREQS, dc_opts(abstol=1e-12))


def ac_ladder(E, n):
    import smallsignal_cases as cases
    from test_gpu_ac_sens import FL, element_names, spread
    c = cases.ladder(n)
    ids = _ids(c, spread(element_names(c), 6))
    return _ac(_small(E)(c), ids, FL, _zero(c))


def _chunk_engine(E):
    import smallsignal_cases as cases
    c = cases.chunk_ladder()
    ids = _ids(c, ["r8", "c150", "r299"])
    e = _small(E)(c)
    e.set_samples(cases.CHUNK_SAMPLES)
    e.set_params([c.sweep[0]], [c.sweep[1]])
    return c, ids, e


def ac_chunks(E):
    c, ids, e = _chunk_engine(E)
    return _ac(e, ids, c.freqs, _zero(c, e.n_samples))


def ac_rlc(E):
    from api_bits_cases import rlc
    c = rlc()
    ids = _ids(c, ["l1", "c1", "r1"])
    return _ac(_small(E)(c), ids, np.array([0.0, 1e4, 5e6, 1e8]), _zero(c))


def ac_failed(E):
    c, ids = _no_point_cell()
    e = _small(E)(c)
    e.set_samples(2)
    e.set_params(ids[:1], [[1e3, math.inf]])
    return _ac(e, ids, np.array([0.0, 1e5]), dc_opts(**FEW))


def _plain(e, f, o):
    rc, x, st = e.ac(f, o)
    return _record(e, rc, st, x=x)


def ac_plain_amp(E):
    from test_gpu_ac_noise import amp_circuit
    from test_gpu_ac_sens import AMP_FREQS
    return _plain(_small(E)(amp_circuit()), AMP_FREQS, dc_opts(abstol=1e-12))


def ac_plain_ladder97(E):
    import smallsignal_cases as cases
    from test_gpu_ac_sens import FL
    c = cases.ladder(97)
    return _plain(_small(E)(c), FL, _zero(c))


# ---- ch_noise, ch_noise_ex ----------------------------------------------------------------------------------------------------------
def noise_plain_amp(E):
    from test_gpu_ac_noise import amp_circuit
    from test_gpu_noise_sens import AMP_FREQS
    c = amp_circuit()
    e = _small(E)(c)
    rc, psd, st = e.noise(0, c._n("d"), AMP_FREQS, dc_opts(abstol=1e-12))
    return _record(e, rc, st, psd=psd)


def noise_plain_ladder97(E):
    import smallsignal_cases as cases
    from test_gpu_noise_sens import F3
    c = cases.ladder(97)
    e = _small(E)(c)
    rc, psd, st = e.noise(0, c._n(c.far), F3, _zero(c))
    return _record(e, rc, st, psd=psd)


def noise_ex_amp(E):
    from test_gpu_ac_noise import amp_circuit
    from test_gpu_noise_sens import AMP_FREQS
    c = amp_circuit()
    e = _small(E)(c)
    rc, psd, contrib, st = e.noise_ex(0, c._n("d"), AMP_FREQS, dc_opts(abstol=1e-12), mos_noise=True, contributions=True)
    return _record(e, rc, st, psd=psd, contrib=contrib)


# ---- ch_noise_sens --------------------------------------------------------------------------------------------------------------------
def _noise(e, out, ids, f, o, **kw):
    rc, psd, dpsd, ds, status, st = e.noise_sens(0, out, ids, f, o, **kw)
    return _record(e, rc, st, psd=psd, dpsd=dpsd, dc_sens=ds, status=status)


def noise_amp_mos(E):
    from test_gpu_ac_noise import amp_circuit
    from test_gpu_noise_sens import AMP_FREQS
    c = amp_circuit()
    ids = _ids(c, ["rd", ("m1", "w"), "temp", ("rb1", "m"), "vdd"])
    return _noise(_small(E)(c), c._n("d"), ids, AMP_FREQS, dc_opts(abstol=1e-12), mos_noise=True)


def noise_shared(E):
    from test_gpu_b4_noise import card
    from test_gpu_noise_sens import FET_FREQS
    c = Circuit(gmin=1e-12)
    mi = c.add_model(*card("nfet_06v0"))
    c.V("vdd", "vdd", 0, dc=5.0)
    c.V("vg", "g", 0, dc=1.6)
    c.R("rd", "vdd", "d", 10e3)
    c.M("ma", "d", "g", 0, 0, mi, 2e-6, 6e-7)
    c.M("mb", "d", "g", 0, 0, mi, 2e-6, 6e-7)
    c.C("cl", "d", 0, 1e-12)
    ids = _ids(c, [("ma", "w"), "rd"])
    return _noise(_small(E)(c), c._n("d"), ids, FET_FREQS, dc_opts(abstol=1e-12), mos_noise=True)


def noise_held(E):
    c = Circuit()
    c.V("vb", "k", 0, dc=1.0)
    c.R("r1", "k", "a", 1e3)
    c.R("r2", "a", 0, 2e3)
    ids = _ids(c, ["r1", "r2", "vb"])
    return _noise(_small(E)(c), c._n("k"), ids, np.array([0.0, 1e3, 1e6]), _zero(c))


def noise_ladder97(E):
    import smallsignal_cases as cases
    from test_gpu_noise_sens import F3, case_names
    c = cases.ladder(97)
    ids = _ids(c, case_names(c, 6))
    return _noise(_small(E)(c), c._n(c.far), ids, F3, _zero(c))


def noise_chunks(E):
    c, ids, e = _chunk_engine(E)
    return _noise(e, c._n("n%d" % c.out), ids, c.freqs, _zero(c, e.n_samples))


def noise_failed(E, out="b"):
    c, ids = _no_point_cell()
    e = _small(E)(c)
    e.set_samples(2)
    e.set_params(ids[:1], [[1e3, math.inf]])
    return _noise(e, c._n(out) if out else 0, ids, np.array([0.0, 1e5]), dc_opts(**FEW))


# ---- ch_tran_sens ---------------------------------------------------------------------------------------------------------------------
def _tran(e, span, ids, o):
    rc, t, v, xf, st, sens = e.tran_sens(span[0], span[1], ids, o)
    return _record(e, rc, st, t=t, v=v, xf=xf, sens=sens)


def _from_zero(c, **kw):
    return tran_opts(stepper="host", dc=dc_opts(abstol=1e-12, x0=np.zeros((1, c.n_mna))), skip_dc=True, **kw)


def tran_rc(E, n, span):
    from test_gpu_tran_sens import rc_ladder
    c = rc_ladder(n)
    ids = _ids(c, sorted({"rs1", "rs%d" % ((n + 1) // 2), "rs%d" % n}, key=lambda s: int(s[2:])))
    return _tran(E(c), (0.0, span), ids, _from_zero(c, abstol=1e-8, reltol=1e-3))


def tran_amp(E):
    from test_gpu_ac_noise import amp_circuit
    c = amp_circuit()
    i = c.dev_ipar[c.dev_names.index("vin")][0]
    c.sources[i] = (0.0, PULSE(0.0, 0.05, 2e-9, 1e-9, 1e-9, 4e-9, 2e-8))
    c.C("cload", "o", 0, 2e-12)
    c.observe_all_nodes()
    ids = _ids(c, ["rd", ("rb1", "m"), ("vin", 1), "vdd"])
    return _tran(E(c), (0.0, 1.2e-8), ids, tran_opts(stepper="host", dc=dc_opts(abstol=1e-12), abstol=1e-9, reltol=1e-6))


def tran_chunks(E):
    from test_gpu_tran_sens import rc_ladder
    c = rc_ladder(96)
    ids = [c.slot("rs%d" % i, "m") for i in range(1, 97)] + [c.slot("cp%d" % i, "m") for i in range(1, 5)]
    return _tran(E(c), (0.0, 5e-8), ids, _from_zero(c, abstol=1e-8, reltol=1e-3))


def tran_skip_dc(E):
    from test_gpu_tran_sens import rc_circuit
    c = rc_circuit()
    ids = _ids(c, ["r1", "c1", ("v", 1)])
    x0 = np.array([[0.2, 0.1] + [0.0] * (c.n_mna - 2)])
    o = tran_opts(stepper="host", dc=dc_opts(abstol=1e-12, x0=x0), skip_dc=True, abstol=1e-9, reltol=1e-6)
    return _tran(E(c), (0.0, 5e-8), ids, o)


# ---- ch_ac_measure --------------------------------------------------------------------------------------------------------------------
def _acm(e, c, ids, f, measures, o):
    from cedarsim_jl_amd.acmeasure import mna_rows, resolve_fmeasures
    res = resolve_fmeasures(measures, mna_rows(c))
    rc, val, status, ds, sample_status, st = e.ac_measure(ids, f, res.specs, len(res.names), o)
    return _record(e, rc, st, value=val, status=status, sens=ds, sample_status=sample_status)


def acm_amp(E, slots=True):
    from test_gpu_ac_measure import AMP_F, AMP_PARAMS, amp_measures
    from test_gpu_ac_noise import amp_circuit
    c = amp_circuit()
    ids = _ids(c, AMP_PARAMS)
    return _acm(_small(E)(c), c, ids if slots else [], AMP_F, amp_measures(), dc_opts(abstol=1e-12))


def acm_ladder97(E, slots=True):
    import smallsignal_cases as cases
    from test_gpu_ac_sens import element_names, spread
    c = cases.ladder(97)
    ids = _ids(c, spread(element_names(c), 3))
    measures = [ffind_at("g", db(c.far), 2e4), ffind_at("g0", db("n0"), 2e4)]
    return _acm(_small(E)(c), c, ids if slots else [], 10.0 ** np.linspace(3.0, 6.0, 7), measures, _zero(c))


# ---- ch_loop_gain ---------------------------------------------------------------------------------------------------------------------
LG_FREQS = np.array([0.0, 1e3, 1e6, 3.3e8, 1e10])


def _lg(e, c, ids, f, o, measures=(), expect=0):
    from cedarsim_jl_amd.acmeasure import resolve_fmeasures
    from cedarsim_jl_amd.batch import _loop_gain_rows
    from loopgain_reference import PROBE
    res = resolve_fmeasures(list(measures), _loop_gain_rows) if measures else None
    rc, T, dT, val, status, ds, sample_status, st = e.loop_gain(c.dev_names.index(PROBE), f, ids, res.specs if res else None, len(res.names) if res else 0, o)
    assert rc == expect, (rc, e.ctx.last_error())      # a case that pins a refusal pins no kernel
    return _record(e, rc, st, T=T, dT=dT, value=val, status=status, sens=ds, sample_status=sample_status)


def lg_loop(E, n, slots=True):
    from loopgain_reference import loop
    from test_gpu_loop_gain import sens_names
    c = loop(n - 4)
    ids = _ids(c, sens_names(c, n)) if slots else []
    run = lambda: _lg(_small(E)(c), c, ids, LG_FREQS, _zero(c))
    return _sparse(run) if n == 97 else run()


def lg_amp_measures(E):
    from test_gpu_loop_gain import AMP_FREQS, AMP_PARAMS, feedback_amp, loop_measures
    c = feedback_amp()
    ids = _ids(c, AMP_PARAMS)       # (slots are declared on the circuit before its engine is built)
    return _lg(_small(E)(c), c, ids, AMP_FREQS, dc_opts(abstol=1e-13), loop_measures())


def lg_failed(E):
    import smallsignal_cases as cases
    from cedarsim_jl_amd import unity_gain_freq
    from loopgain_reference import loop
    c = loop()
    c.I("i1", "n", 0, dc=1e-3)
    c.R("rn", "n", 0, 1e3)
    ids = _ids(c, ["rn", "r2"])
    e = _small(E)(c)
    e.set_samples(3)
    e.set_params(ids[:1], [[1e3, math.inf, 2e3]])
    return _lg(e, c, ids, cases.FREQS[2:6], dc_opts(**FEW), [unity_gain_freq("fug", "T", xscale="lin")], expect=-3)


# name -> (runner(EngineCircuit), the case runs above 96 unknowns)
CASES = {
    "dc_amp3": (dc_amp3, False),
    "dc_chunks": (dc_chunks, False),
    "dc_ladder97": (dc_ladder97, True),
    "dc_failed": (dc_failed, False),
    "ac_amp": (ac_amp, False),
    "ac_amp_sparse": (lambda E: _sparse(lambda: ac_amp(E)), False),
    "ac_ladder96": (lambda E: ac_ladder(E, 96), False),
    "ac_ladder97": (lambda E: ac_ladder(E, 97), True),
    "ac_chunks": (ac_chunks, True),
    "ac_rlc": (ac_rlc, False),
    "ac_failed": (ac_failed, False),
    "ac_plain_amp": (ac_plain_amp, False),
    "ac_plain_ladder97": (ac_plain_ladder97, True),
    "noise_plain_amp": (noise_plain_amp, False),
    "noise_plain_ladder97": (noise_plain_ladder97, True),
    "noise_ex_amp": (noise_ex_amp, False),
    "noise_amp_mos": (noise_amp_mos, False),
    "noise_shared": (noise_shared, False),
    "noise_held": (noise_held, False),
    "noise_ladder97": (noise_ladder97, True),
    "noise_chunks": (noise_chunks, True),
    "noise_failed": (noise_failed, False),
    "noise_failed_held": (lambda E: noise_failed(E, out=None), False),
    "tran_rc2": (lambda E: tran_rc(E, 2, 2e-9), False),
    "tran_rc97": (lambda E: tran_rc(E, 97, 2e-8), True),
    "tran_amp": (tran_amp, False),
    "tran_chunks": (tran_chunks, False),
    "tran_skip_dc": (tran_skip_dc, False),
    "acm_amp": (acm_amp, False),
    "acm_amp_noslots": (lambda E: acm_amp(E, slots=False), False),
    "acm_ladder97": (acm_ladder97, True),
    "acm_ladder97_noslots": (lambda E: acm_ladder97(E, slots=False), True),
    "lg_loop4": (lambda E: lg_loop(E, 4), False),
    "lg_loop96": (lambda E: lg_loop(E, 96), False),
    "lg_loop97": (lambda E: lg_loop(E, 97), True),
    "lg_loop64_noslots": (lambda E: lg_loop(E, 64, slots=False), False),
    "lg_loop97_noslots": (lambda E: lg_loop(E, 97, slots=False), True),
    "lg_amp_measures": (lg_amp_measures, False),
    "lg_failed": (lg_failed, False),
}

# golden file under tests/golden/ -> the prefixes of the cases it holds (a case belongs to the first file that claims it)
GOLDEN_FILES = {"loopgain_bits.npz": ("lg_",), "sens_driver_bits.npz": ("",)}


def golden_file(name):
    return next(f for f, prefixes in GOLDEN_FILES.items() if name.startswith(prefixes))


def run_case(EngineCircuit, name):
    return CASES[name][0](EngineCircuit)
