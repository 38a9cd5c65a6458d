"""The BSIM4 card space on the device (run with `-m gpu` on an MI355X): every card variant of tests/bsim4_cards.py through
the existing entry points — ch_mos_eval (one lane per instance), ch_mos_eval_quad (four lanes), ch_eval (the assembled
residual and Jacobian, on the default and on the sparse path), ch_dc and ch_tran (the device stepper with and without the
wave-pair split, and the sparse path) — against the CPU oracle.

The stamps are judged PER ROW (bsim4_cards.row_scales): a leakage current is measured against its own row, not against the
on-current of another.  The bound is the project's stamp tolerance, 1e-10; test_bsim4_oracle.test_bias_set_is_well_conditioned
shows that rounding of the inputs alone moves the reference by at most 2e-11 on these rows."""
import ctypes

import numpy as np
import pytest

import bsim4_cards as BC
from cedarsim_jl_amd import dc_opts, tran_opts
from cedarsim_jl_amd.circuit import ERR_UNSUPPORTED, CedarError

pytestmark = pytest.mark.gpu

ROWS = BC.bias_rows()
VBANK = BC.bank_voltages(ROWS)
TEMPS = (-40.0, 27.0, 125.0)
STAMP_TOL = 1e-10


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()  # fails loudly if the HIP extension is missing
    return EngineCircuit


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


# ------------------------------------------------------------------------------------------------
# device level
@pytest.mark.parametrize("name", BC.NAMES)
def test_stamps_match_oracle_row_by_row(E, O, name):
    c = BC.fet_bank(name, rows=len(ROWS))
    e, o = E(c), O(c)
    st = c.slot("temp")
    bad = []
    for temp in TEMPS:
        e.set_params([st], [[temp]])
        o.set_param(st, temp)
        b = o.mos_eval(VBANK)
        for label, a in (("plain", e.mos_eval(VBANK)), ("quad", e.mos_eval(VBANK, quad=True))):
            err, r, s = BC.worst(a, b)
            print("variant %-9s %6.1f C %-5s worst row-scaled error %.3e (%s row %d %s, slot %s: %.17g vs %.17g)" % (
                name, temp, label, err, "nmos" if r % 2 == 0 else "pmos", r // 2, ROWS[r // 2].tolist(), BC.SLOT_NAMES[s], a[r, s], b[r, s]))
            if not err < STAMP_TOL:
                bad.append((name, temp, label, err, "row %d" % (r // 2), "nmos" if r % 2 == 0 else "pmos", ROWS[r // 2].tolist(), BC.SLOT_NAMES[s], a[r, s], b[r, s]))
    assert not bad, bad


FAR_ROWS = BC.far_admitted_rows()
FAR_VBANK = BC.bank_voltages(FAR_ROWS)


@pytest.mark.parametrize("name", BC.NAMES)
def test_far_bias_stamps_are_finite_and_match_oracle(E, O, name):
    """The rows a cold-start Newton iterate reaches and the bias set does not (20 V and 40 V, BC.far_bias_rows without the rows
    test_bsim4_oracle finds ill-conditioned): finite everywhere, and within STAMP_TOL per row, as above.  frcp and fsqrt have no
    guard (frcp(+-0), frcp(+-inf) are NaN by construction, tests/test_gpu_device_math.py): a model path that reached such an
    argument on these rows would show here as a NaN the oracle, which divides, does not have."""
    c = BC.fet_bank(name, rows=len(FAR_ROWS))
    e, o = E(c), O(c)
    st = c.slot("temp")
    bad = []
    for temp in TEMPS:
        e.set_params([st], [[temp]])
        o.set_param(st, temp)
        b = o.mos_eval(FAR_VBANK)
        assert np.all(np.isfinite(b)), (name, temp)
        for label, a in (("plain", e.mos_eval(FAR_VBANK)), ("quad", e.mos_eval(FAR_VBANK, quad=True))):
            nf = np.nonzero(~np.isfinite(a).all(axis=1))[0]
            err, r, s = BC.worst(a, b)
            print("variant %-9s %6.1f C %-5s far rows: worst row-scaled error %.3e (%s row %s, slot %s: %.17g vs %.17g)" % (
                name, temp, label, err, "nmos" if r % 2 == 0 else "pmos", FAR_ROWS[r // 2].tolist(), BC.SLOT_NAMES[s], a[r, s], b[r, s]))
            if nf.size or not err < STAMP_TOL:
                bad.append((name, temp, label, err, "nmos" if r % 2 == 0 else "pmos", FAR_ROWS[r // 2].tolist(), BC.SLOT_NAMES[s], a[r, s], b[r, s],
                            "not finite: %s" % [FAR_ROWS[i // 2].tolist() for i in nf[:4]]))
    assert not bad, bad


@pytest.mark.parametrize("sel,val", BC.UNSUPPORTED_SELECTORS)
def test_unimplemented_sub_models_are_refused_like_the_oracle_does(E, O, sel, val):
    c = BC.fet_bank({sel: float(val)}, rows=1)
    o = O(c)
    pf = ctypes.POINTER(ctypes.c_double)
    v, out = np.ascontiguousarray(VBANK[:2]), np.zeros((2, 40))
    rc_o = o.L.oracle_mos_eval(o.h, v.ctypes.data_as(pf), out.ctypes.data_as(pf))
    assert rc_o == ERR_UNSUPPORTED
    try:
        e = E(c)
    except CedarError as ex:   # refused at construction: the message names the cause
        assert "sub-model" in str(ex), ex
        return
    for fn in (e.L.ch_mos_eval, e.L.ch_mos_eval_quad):   # or at the first call, with the oracle's code
        assert fn(e.h, 0, v.ctypes.data_as(pf), out.ctypes.data_as(pf)) == rc_o, (sel, val)
    assert e.dc()[0] == rc_o and "sub-model" in e.ctx.last_error()


# ------------------------------------------------------------------------------------------------
# the assembled residual and Jacobian: the default path, and the sparse path's two device halves
def _eval_errors(e, o, c):
    nu = e.maps()[0]
    rc, xo, _ = o.dc(dc_opts(abstol=1e-14))
    assert rc == 0
    rng = np.random.default_rng(3)
    x = xo + 0.05 * rng.standard_normal(xo.shape)
    for n in range(1, c.n_nodes + 1):
        if nu[n] < 0:
            x[n - 1] = xo[n - 1]   # eliminated nodes hold their source-defined values
    reps = [n - 1 for n in range(1, c.n_nodes + 1) if nu[n] >= 0]
    assert len(reps) == e.info()["n_unknowns"] == 2 and e.info()["n_alias"] == 0
    worst = 0.0
    for alpha0 in (0.0, 3e9):
        Fe, Qe, Je = e.eval(x, t=0.0, alpha0=alpha0, mode=1)
        Fo, Qo, Jo = o.eval(x, t=0.0, alpha0=alpha0, mode=1)
        Jo_r = Jo[np.ix_(reps, reps)]
        for got, want in ((Fe[reps], Fo[reps]), (Qe[reps], Qo[reps]), (Je[np.ix_(reps, reps)], Jo_r)):
            assert np.max(np.abs(want)) > 0.0
            worst = max(worst, np.max(np.abs(got - want)) / np.max(np.abs(want)))
    return worst


@pytest.mark.parametrize("name", BC.CIRCUIT_NAMES)
def test_assembled_residual_and_jacobian_match_oracle(E, O, monkeypatch, name):
    c = BC.inverter_chain(name)
    o = O(c)
    bad = []
    for label, path in (("default", 1), ("sparse", 2)):
        if path == 2:
            monkeypatch.setenv("CEDARHIP_FORCE_SPARSE", "1")
        e = E(c)
        err = _eval_errors(e, o, c)
        monkeypatch.delenv("CEDARHIP_FORCE_SPARSE", raising=False)
        assert e.info()["path"] == path, (label, e.info()["path"])   # the run took the path it names
        print("variant %-5s ch_eval %-7s worst error %.3e of the oracle's maximum" % (name, label, err))
        if not err <= 1e-10:
            bad.append((name, label, err))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# inside the steppers
@pytest.mark.parametrize("name", BC.CIRCUIT_NAMES)
def test_operating_point_and_transient_match_oracle_on_every_stepper(E, O, monkeypatch, name):
    c = BC.inverter_chain(name)
    o = O(c)
    rc, xo, _ = o.dc(dc_opts(abstol=1e-14))
    assert rc == 0
    tol = 1e-7
    t0, t1 = BC.CHAIN_TSPAN
    rco, to, vo, _, _ = o.tran(t0, t1, tran_opts(abstol=tol, reltol=tol, saveat=BC.CHAIN_SAVEAT, skip_dc=True, dc=dc_opts(x0=xo)))
    assert rco == 0 and len(to) == len(BC.CHAIN_SAVEAT)
    assert vo.max() > 4.9 and vo.min() < 0.1                      # both outputs really switch inside the window
    scale = max(1.0, np.abs(vo).max())
    steps = {}
    for label, env in (("device", None), ("device_nopair", "CEDARHIP_PERSIST_NOPAIR"), ("sparse", "CEDARHIP_FORCE_SPARSE")):
        if env:
            monkeypatch.setenv(env, "1")
        try:
            e = E(c)
            rc, x, status, _ = e.dc(dc_opts(abstol=1e-14, x0=xo[None, :]))
            assert rc == 0 and status[0] == 0, (label, rc, e.ctx.last_error())
            ok = ~np.isnan(x[0])
            assert np.allclose(x[0][ok], xo[ok], rtol=1e-6, atol=1e-9), (label, np.max(np.abs(x[0][ok] - xo[ok])))
            rc, t, v, _, st = e.tran(t0, t1, tran_opts(abstol=tol, reltol=tol, saveat=BC.CHAIN_SAVEAT, skip_dc=True, dc=dc_opts(x0=xo[None, :])))
            assert rc == 0, (label, rc, e.ctx.last_error())
            path = e.info()["path"]
        finally:
            if env:
                monkeypatch.delenv(env, raising=False)
        # the run took the path it names: the device-resident controller in lock-step form on the dense path, or the sparse path
        if label == "sparse":
            assert path == 2, (label, path)
        else:
            assert path == 1 and st["stepper"] == 2 and st["stepper_mode"] == 1, (label, path, st["stepper"], st["stepper_mode"])
        assert np.array_equal(t, BC.CHAIN_SAVEAT)
        err = np.max(np.abs(v[:, :, 0] - vo))
        print("variant %-5s %-13s waveform error %.3e V, %d accepted / %d rejected steps" % (name, label, err, st["naccept"], st["nreject"]))
        assert err < 1e-4 * scale, (name, label, err)
        steps[label] = (st["naccept"], st["nreject"])
    assert steps["device"] == steps["device_nopair"], steps    # one policy, one arithmetic: the split must not change a step
