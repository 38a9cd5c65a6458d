"""The numpy yardstick of the BSIM4 MOSFET noise (tests/bsim4_noise_reference.py) against closed forms: hand numbers for the thermal
record and fnoimod 0, the unified model's limit noib = noic = 0, vds -> 0 against its first-order expansion, the harmonic mean
against its two asymptotes, and psd_from_transfers on a two-source case."""
import numpy as np

import bsim4_noise_reference as R


def _op(**kw):
    op = dict(ids=1e-4, ueff=0.05, vgsteff=1.0, abulk=1.2, vdseff=0.3, vds=0.5, rds=0.0, esat=4e6, litl=5e-8, leff=1e-6, weffnf=2e-6,
              coxe=2e-3, cdep0=5e-4, cit=0.0, vtm=0.025, qinv=-1e-14)
    op.update(kw)
    return op


def test_hand_numbers_thermal_and_simple_flicker():
    par = dict(R.defaults("n"), fnoimod=0, kf=1e-25, af=2.0, ef=1.1)
    # 4 k 300 * (0.05 * 1e-14) / 1e-12
    assert np.isclose(R.thermal(_op(), par, 300.0), 4 * 1.380649e-23 * 300.0 * 5e-4, rtol=1e-14)
    assert np.isclose(R.thermal(_op(rds=100.0), par, 300.0), 4 * 1.380649e-23 * 300.0 * 5e-16 / 1.05e-12, rtol=1e-14)
    assert np.isclose(R.thermal(_op(qinv=+1e-14), dict(par, ntnoi=2.0), 300.0), 8 * 1.380649e-23 * 300.0 * 5e-4, rtol=1e-14)   # |qinv|, ntnoi
    # 1e-25 * (1e-4)^2 / (2e-3 * 1e-12) = 5e-19
    assert np.isclose(R.flicker_simple(_op(), par), 5e-19, rtol=1e-14)
    assert np.isclose(R.flicker_simple(_op(ids=-1e-4), par), 5e-19, rtol=1e-14)
    assert R.flicker_simple(_op(), dict(par, kf=0.0)) == 0.0
    rec = R.records(_op(), par, 300.0, m=3.0)
    assert rec[0][1] == 0.0 and rec[1][1] == 1.1 and np.isclose(rec[1][0], 1.5e-18, rtol=1e-14)
    assert R.defaults("p")["noia"] == 6.188e40 and R.defaults("n")["noib"] == 3.125e26 and R.defaults("p")["fnoimod"] == 1


def test_unified_model_first_order_limit_at_small_vds():
    """noib = noic = 0, vds = vdseff -> 0 with em < esat (no channel-length modulation term):
    S_inv -> kT q^2 ueff ids noia / (coxe leff^2 abulk 1e10) * (N0 - Nl)/(N0 + N*),  N0 - Nl = N0 abulk vdseff / (vgsteff + 2 vtm)."""
    T = 300.0
    par = dict(R.defaults("n"), noib=0.0, noic=0.0, em=1e6)
    for vde in (1e-5, 1e-6):
        op = _op(vdseff=vde, vds=vde, ids=3e-7)
        s_inv, _ = R.unified_parts(op, par, T)
        N0 = op["coxe"] * op["vgsteff"] / R.Q
        Ns = op["vtm"] * (op["coxe"] + op["cdep0"]) / R.Q
        x = op["abulk"] * vde / (op["vgsteff"] + 2 * op["vtm"])
        first = R.KB * T * R.Q ** 2 * op["ueff"] * op["ids"] * par["noia"] / (op["coxe"] * op["leff"] ** 2 * op["abulk"] * 1e10) * N0 * x / (N0 + Ns)
        assert abs(float(s_inv) / first - 1.0) < 2.0 * x, (vde, float(s_inv), first)   # the next term of the expansion is of relative size x/2


def test_harmonic_mean_against_both_asymptotes():
    T = 300.0
    # S_wi << S_inv: a large noib raises S_inv alone;  S_inv << S_wi: a small vdseff lowers S_inv alone
    lo_wi = (_op(), dict(R.defaults("n"), noib=1e34))
    lo_inv = (_op(vdseff=1e-7, vds=1e-7), dict(R.defaults("n"), em=1e6))
    for (op, par), which in ((lo_wi, 1), (lo_inv, 0)):
        parts = [float(v) for v in R.unified_parts(op, par, T)]
        small, big = parts[which], parts[1 - which]
        assert small < 1e-4 * big
        h = R.flicker_unified(op, par, T)
        assert h < small and np.isclose(h, small, rtol=2.0 * small / big)
        assert np.isclose(h * (1.0 + small / big), small, rtol=1e-12)
    assert R.flicker_unified(_op(ids=0.0), R.defaults("n"), T) == 0.0


def test_psd_from_transfers():
    f = np.array([1.0, 10.0, 100.0])
    H = [np.array([2.0, 2.0j, 1.0 + 1.0j]), np.array([0.5, 0.5, 0.5])]
    got = R.psd_from_transfers(H, [(3.0, 0.0), (8.0, 1.0)], f)
    assert np.allclose(got, [4 * 3.0 + 0.25 * 8.0, 4 * 3.0 + 0.25 * 0.8, 2 * 3.0 + 0.25 * 0.08], rtol=1e-15)
