"""The CPU yardstick of the network-parameter tests (netparams_reference.py) against closed forms, to 1e-12: the series resistor
(which pins the sign of the port current), the matched three-way splitter, the unilateral VCCS stage with unequal reference
impedances, the third-order Butterworth low-pass, and its analytic dS/dp, dY/dp, dZ/dp against its own Richardson differences."""
import copy

import numpy as np

import netparams_reference as NP

TOL = 1e-12


def test_series_resistor_pins_the_current_sign():
    c, ports = NP.series_r(50.0)
    r = NP.net_params(c, ports, 50.0, [0.0, 1e6, 1e9], want_z=False)
    for f in range(3):
        assert np.max(np.abs(r["S"][f] - np.array([[1, 2], [2, 1]]) / 3.0)) <= TOL
        assert np.max(np.abs(r["Y"][f] - np.array([[0.02, -0.02], [-0.02, 0.02]]))) <= TOL   # Y11 = +1/R: the current ENTERING counts
        assert np.max(np.abs(r["S_l"][f] - r["S"][f])) <= TOL


def test_three_way_star_is_matched():
    c, ports = NP.star3()
    r = NP.net_params(c, ports, 50.0, [0.0, 1e8], want_z=False)    # (nothing goes to ground: Yp is singular, Z does not exist)
    want = 0.5 * (np.ones((3, 3)) - np.eye(3))
    assert np.max(np.abs(r["S"] - want[None])) <= TOL
    assert np.max(np.abs(r["Y"].sum(axis=2))) <= TOL


def test_unilateral_stage_with_unequal_reference_impedances():
    c, ports = NP.unilateral()
    z1, z2 = 50.0, 75.0
    r = NP.net_params(c, ports, (z1, z2), [0.0, 1e7])
    for f in range(2):
        assert np.max(np.abs(r["Y"][f] - np.array([[1.0 / NP.RIN, 0.0], [NP.GM, 1.0 / NP.RO]]))) <= TOL
        S = r["S"][f]
        assert S[0, 1] == 0.0
        s21 = -2.0 * NP.GM * np.sqrt(z1 * z2) / ((1.0 + z1 / NP.RIN) * (1.0 + z2 / NP.RO))
        assert abs(S[1, 0] - s21) <= TOL * abs(s21)
        assert np.max(np.abs(r["Z"][f] @ r["Y"][f] - np.eye(2))) <= TOL
        assert abs(S[0, 0] - (1.0 - z1 / NP.RIN) / (1.0 + z1 / NP.RIN)) <= TOL and abs(S[1, 1] - (1.0 - z2 / NP.RO) / (1.0 + z2 / NP.RO)) <= TOL


def test_butterworth_low_pass():
    fc = 1e8
    c, ports = NP.butterworth(50.0, fc)
    f = np.array([1e3, 1e7, 5e7, 1e8, 2e8, 1e9])
    r = NP.net_params(c, ports, 50.0, f, want_z=False)    # (det Yp = 2C/L - (wC)^2 vanishes at fc: Z does not exist there)
    S = r["S"]
    assert np.max(np.abs(np.abs(S[:, 1, 0]) ** 2 - 1.0 / (1.0 + (f / fc) ** 6))) <= TOL
    for k in range(len(f)):
        assert np.max(np.abs(S[k].conj().T @ S[k] - np.eye(2))) <= TOL       # lossless
        assert np.max(np.abs(S[k] - S[k].T)) <= TOL                          # reciprocal
    assert abs(abs(S[3, 1, 0]) ** 2 - 0.5) <= TOL                            # -3 dB at fc


def _moved(c, slot, value):
    d = copy.deepcopy(c)
    d.dev_par[slot[1]][slot[2]] = value
    return d


def test_analytic_derivatives_against_richardson_differences():
    """dS, dY, dZ of the bilateral stage (z0 = 50, 75) in rg, cf, gm and ro: central differences of the yardstick's own values at
    relative steps 2e-4 and 1e-4, extrapolated; the finer difference lies within 1e-7 of the extrapolation (its h^2 term), the analytic values agree
    with the extrapolation to 1e-8 of the kind's largest entry."""
    c, ports = NP.stage(5)
    f = np.array([0.0, 1e6, 1e9])
    names = ["rg", "cf", "gm", "ro"]
    slots = [c.slots[c.slot(nm)] for nm in names]
    r = NP.net_params(c, ports, NP.Z0_STAGE, f, slots=slots)
    for k, slot in enumerate(slots):
        p = c.dev_par[slot[1]][slot[2]]
        y = []
        for rel in (2e-4, 1e-4):
            h = rel * abs(p)
            plus, minus = (NP.net_params(_moved(c, slot, p + s * h), ports, NP.Z0_STAGE, f) for s in (1, -1))
            y.append({kd: (plus[kd] - minus[kd]) / (2.0 * h) for kd in NP.KINDS})
        for kd in NP.KINDS:
            rich = (4.0 * y[1][kd] - y[0][kd]) / 3.0
            top = np.max(np.abs(rich))
            assert np.max(np.abs(y[1][kd] - rich)) <= 1e-7 * top
            assert np.max(np.abs(r["d" + kd][:, k] - rich)) <= 1e-8 * top, (names[k], kd)


def test_the_method_of_the_engine_in_numpy_agrees():
    c, ports = NP.stage(5)
    f = np.array([0.0, 1e6, 1e10])
    slots = [c.slots[c.slot(nm)] for nm in ("rg", "cf", "gm", "ro")]
    r = NP.net_params(c, ports, NP.Z0_STAGE, f, slots=slots)
    fd = NP.fd_net_sens(c, ports, NP.Z0_STAGE, f, slots)
    for kd in NP.KINDS:
        assert NP.sens_errors(fd["d" + kd], r["d" + kd]).max() <= 1e-9
