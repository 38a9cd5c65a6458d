"""Pins the yardstick of the noise sensitivity tests (noisesens_reference.py) without a GPU: closed forms for R || C at a node, and
Richardson-extrapolated central differences of smallsignal_reference.noise_psd (40-digit adjoint solves) for ladder(2) and
pivot_torture; the same-method error e_cpu of fd_noise_sens is printed and held to the bound the GPU tests rely on."""
import copy
import math

import numpy as np
import pytest

import acsens_reference as AR
import noisesens_reference as NR
import smallsignal_cases as cases
import smallsignal_reference as SR
from cedarsim_jl_amd import Circuit
from cedarsim_jl_amd.circuit import DEV_C, DEV_L, DEV_R

K = SR.K_BOLTZMANN


def slots_of(c, names):
    return [c.slots[c.slot(*nm) if isinstance(nm, tuple) else c.slot(nm)] for nm in names]


def test_closed_forms_of_the_rc_cell():
    """R || C at a node driven by nothing: S = 4kTR/(1+x^2), x = wRC; dS/dR = 4kT(1-x^2)/(1+x^2)^2; dS/dC = -8kTR x^2/(C(1+x^2)^2);
    dS/dT = S/T; dS/dm of the resistor (m = 1: R/m in parallel) = -R dS/dR."""
    r, cap, t = 1.3e3, 2.2e-9, 27.0 + 273.15
    c = Circuit()
    c.R("r1", "a", 0, r)
    c.C("c1", "a", 0, cap)
    slots = slots_of(c, ["r1", "c1", "temp", ("r1", "m")])
    out = c.mna_index("v", "a")
    for f in (0.0, 1e3, 1.0 / (2.0 * math.pi * r * cap), 1e6, 1e9):
        w = 2.0 * math.pi * f
        x = w * r * cap
        S, dS, D = NR.noise_sens(c, slots, out, w)
        want_S = 4 * K * t * r / (1 + x * x)
        want = [4 * K * t * (1 - x * x) / (1 + x * x) ** 2, -8 * K * t * r * x * x / (cap * (1 + x * x) ** 2), want_S / t,
                -r * 4 * K * t * (1 - x * x) / (1 + x * x) ** 2]
        assert abs(S - want_S) <= 1e-14 * want_S
        for k in range(4):
            assert abs(dS[k] - want[k]) <= 1e-13 * D[k] or (D[k] == 0.0 and dS[k] == 0.0 and want[k] == 0.0), (f, k, dS[k], want[k], D[k])
        assert D[2] == pytest.approx(abs(want[2]), rel=1e-14)      # temp: a single positive term, nothing cancels
        _, g = NR.fd_noise_sens(c, slots, out, w)
        assert np.max(NR.scaled_error(g, dS, D)) <= 1e-10


def richardson(c, slot, out, w):
    """dS/dp by central differences of SR.noise_psd at relative steps 1e-3 and 5e-4, extrapolated; its own error estimate; and what
    the rounding of the PSDs to double precision (noise_psd returns a float) can add to a difference: 4 * 2^-52 S / h."""
    kind, sa, sb = slot
    p0 = c.temp if kind == NR.SLOT_TEMP else (c.dev_mult[sa] if kind == NR.SLOT_DEV_MULT else c.dev_par[sa][sb])

    def at(dp):
        return SR.noise_psd(NR._moved(c, slot, dp), out, w)
    d = []
    for rel in (1e-3, 5e-4):
        h = rel * abs(p0)
        d.append((at(h) - at(-h)) / (2.0 * h))
    r = (4.0 * d[1] - d[0]) / 3.0
    return r, abs(d[1] - r), 4.0 * 2.0 ** -52 * at(0.0) / (5e-4 * abs(p0))


@pytest.mark.parametrize("name", ["ladder2", "pivot"])
def test_yardstick_against_richardson_differences_of_the_refined_psd(name):
    if name == "ladder2":
        c = cases.ladder(2)
        names = [nm for nm, k in zip(c.dev_names, c.dev_kind) if k in (DEV_R, DEV_C)] + ["temp", ("rs1", "m")]
        out, freqs = c.mna_index("v", c.far), [0.0, 1e3, 1e6, 1e10]
    else:
        c = cases.pivot_torture()
        names = [nm for nm, k in zip(c.dev_names, c.dev_kind) if k in (DEV_R, DEV_C, DEV_L)] + ["temp"]
        out, freqs = c.mna_index("v", "p"), [1e3, 1e6, 3.3e8]
    slots = slots_of(c, names)
    worst_cpu = 0.0
    for f in freqs:
        w = 2.0 * math.pi * f
        S, dS, D = NR.noise_sens(c, slots, out, w)
        assert S == pytest.approx(SR.noise_psd(c, out, w), rel=1e-13)
        _, g = NR.fd_noise_sens(c, slots, out, w)
        worst_cpu = max(worst_cpu, float(np.max(NR.scaled_error(g, dS, D))))
        for k, slot in enumerate(slots):
            r, est, rnd = richardson(c, slot, out, w)
            # the extrapolated difference is good to its own estimate, the rounding of the PSDs and h^4 terms (1e-12 relative)
            assert abs(dS[k] - r) <= 4.0 * est + rnd + 1e-9 * D[k], (name, f, names[k], dS[k], r, est, rnd, D[k])
            assert est <= 1e-5 * max(D[k], abs(r)) + rnd, (name, f, names[k], est, rnd)
    print("%s: e_cpu of fd_noise_sens %.2e" % (name, worst_cpu))
    assert worst_cpu <= AR.E_CPU_MAX
