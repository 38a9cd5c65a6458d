"""Pins the analytic AC-sensitivity yardstick (acsens_reference.py) against closed forms, and the numpy version of the engine's
method against the yardstick, on the CPU."""
import numpy as np
import pytest

import acsens_reference as AR
import smallsignal_cases as cases
import smallsignal_reference as SR
from cedarsim_jl_amd import Circuit


def rc_lowpass(r=1.3e3, c=2.2e-9):
    ck = Circuit()
    ck.V("vin", "a", 0, dc=0.0, ac=1.0)
    ck.R("r1", "a", "b", r)
    ck.C("c1", "b", 0, c)
    return ck


def test_rc_lowpass_closed_forms():
    """H = 1 / (1 + jwRC) at node b:  dH/dR = -jwC H^2,  dH/dC = -jwR H^2; the source's DC value and the source node give 0."""
    r, c = 1.3e3, 2.2e-9
    ck = rc_lowpass(r, c)
    slots = [ck.slots[ck.slot(nm)] for nm in ("r1", "c1", "vin")]
    b = ck.mna_index("v", "b")
    for f in (0.0, 1e3, 1.0 / (2 * np.pi * r * c), 1e7):
        w = 2 * np.pi * f
        x, s = AR.ac_sens(ck, slots, w)
        h = 1.0 / (1.0 + 1j * w * r * c)
        assert abs(x[b] - h) <= 1e-15
        assert abs(s[0][b] - (-1j * w * c * h * h)) <= 1e-15 * max(abs(w * c), 1e-300)
        assert abs(s[1][b] - (-1j * w * r * h * h)) <= 1e-15 * max(abs(w * r), 1e-300)
        assert not s[2].any() and s[0][ck.mna_index("v", "a")] == 0.0
        if f == 0.0:
            assert not s[0].any() and not s[1].any()


def test_series_rlc_closed_forms():
    """vin - R - L - (C to ground): H = 1 / D at the capacitor, D = 1 - w^2 LC + jwRC;  dH/dR = -jwC H^2, dH/dL = w^2 C H^2,
    dH/dC = -(jwR - w^2 L) H^2; the source current is I = -jwC H (from net+ through the source)."""
    r, l, c = 47.0, 3.3e-6, 1.5e-9
    ck = Circuit()
    ck.V("vin", "a", 0, dc=0.0, ac=1.0)
    ck.R("r1", "a", "m", r)
    ck.L("l1", "m", "o", l)
    ck.C("c1", "o", 0, c)
    slots = [ck.slots[ck.slot(nm)] for nm in ("r1", "l1", "c1")]
    o, iv = ck.mna_index("v", "o"), ck.mna_index("i", "vin")
    f0 = 1.0 / (2 * np.pi * np.sqrt(l * c))
    for f in (1e4, 0.5 * f0, f0, 3.0 * f0):
        w = 2 * np.pi * f
        x, s = AR.ac_sens(ck, slots, w)
        h = 1.0 / (1.0 - w * w * l * c + 1j * w * r * c)
        want = [-1j * w * c * h * h, w * w * c * h * h, -(1j * w * r - w * w * l) * h * h]
        assert abs(x[o] - h) <= 1e-14 * abs(h) and abs(x[iv] - (-1j * w * c * h)) <= 1e-14 * abs(w * c * h)
        for k in range(3):
            assert abs(s[k][o] - want[k]) <= 1e-13 * abs(want[k]), (f, k)
        # d(source current)/dp = -jwC dH/dp for R and L; for C the product rule adds -jw H
        assert abs(s[0][iv] - (-1j * w * c * want[0])) <= 1e-13 * abs(w * c * want[0])
        assert abs(s[2][iv] - (-1j * w * h - 1j * w * c * want[2])) <= 1e-13 * abs(w * h)


def test_multiplier_and_gain_stamps_against_a_difference_of_the_reference():
    """The multiplier and controlled-source stamps against central differences of refined solves (step 1e-4 relative:
    truncation 1e-8, far above the refined solves' error)."""
    ck = cases.pivot_torture()
    names = [("r1", "m"), ("cc", "m"), ("la", "m"), "e1", "gy1", ("gy2", "m"), ("e2", "m")]
    slots = [ck.slots[ck.slot(*nm) if isinstance(nm, tuple) else ck.slot(nm)] for nm in names]
    w = 2 * np.pi * 1e6
    _, s = AR.ac_sens(ck, slots, w)
    for k, slot in enumerate(slots):
        p = ck.dev_mult[slot[1]] if slot[0] == AR.SLOT_DEV_MULT else ck.dev_par[slot[1]][slot[2]]
        h = 1e-4 * abs(p)
        xp = SR.solve(*SR.mna(AR._moved(ck, slot, h), w))[0]
        xm = SR.solve(*SR.mna(AR._moved(ck, slot, -h), w))[0]
        fd = (xp - xm) / (2 * h)
        assert np.max(np.abs(fd - s[k])) <= 1e-6 * np.max(np.abs(s[k])), names[k]


def test_mag_phase_sens_against_a_finite_difference():
    """d|H|/dR and d(arg H)/dR of the RC low-pass from H and dH/dR = -jwC H^2, against central differences of |H| and arg H."""
    from cedarsim_jl_amd import mag_phase_sens
    r, c = 1.3e3, 2.2e-9
    w = 2 * np.pi * np.array([1e3, 5e4, 2e6])

    def resp(rr):
        return 1.0 / (1.0 + 1j * w * rr * c)
    h = resp(r)
    dmag, dph = mag_phase_sens(h, -1j * w * c * h * h)
    d = 1e-5 * r
    assert np.allclose(dmag, (np.abs(resp(r + d)) - np.abs(resp(r - d))) / (2 * d), rtol=1e-7, atol=0.0)
    assert np.allclose(dph, (np.angle(resp(r + d)) - np.angle(resp(r - d))) / (2 * d), rtol=1e-7, atol=0.0)
    assert np.all(dmag < 0.0) and np.all(dph < 0.0)


@pytest.mark.parametrize("n", [1, 2, 63, 96])
def test_the_method_in_numpy_meets_the_yardstick(n):
    """fd_ac_sens (the engine's method in numpy) against the yardstick on a ladder: the e_cpu of the GPU tests, which must stay
    below 1e-7 for a case to be admissible."""
    ck = cases.ladder(n)
    names = [nm for nm, k in zip(ck.dev_names, ck.dev_kind) if k in (AR.DEV_R, AR.DEV_C, AR.DEV_L, AR.DEV_VCCS)][:6]
    slots = [ck.slots[ck.slot(nm)] for nm in names]
    groups = SR.unit_groups(ck)
    for f in (0.0, 1e6, 3.3e8):
        w = 2 * np.pi * f
        _, want = AR.ac_sens(ck, slots, w)
        _, got = AR.fd_ac_sens(ck, slots, w)
        e = AR.scaled_errors(got, want, groups)
        assert AR.tolerance(float(e.max())) <= 32 * AR.E_CPU_MAX
        if f == 0.0:
            caps = [k for k, s in enumerate(slots) if ck.dev_kind[s[1]] in (AR.DEV_C, AR.DEV_L)]
            assert all(not want[k].any() and not got[k].any() for k in caps)
