"""Pins the CPU yardstick of the loop-gain analysis (loopgain_reference.py) on the test loop — a VCCS gm = 2e-3 from y pulling current out
of o, Ro = 5e3 || Co = 1e-12 at o, R1 = 7e3 from o to x, the probe x -> y, R2 = 3e3 || Cg = 2e-13 at y; DC loop gain 2 exactly — against
definitions that do not go through u = V2 - I1: the return ratio of the VCCS on the closed wire, the two-port expression, closed forms.
No GPU."""
import numpy as np

import acsens_reference as AR
import loopgain_reference as LG
import smallsignal_cases as cases

FREQS = np.array([0.0, 1e6, 1e8, 1e9, 1e10])


def test_T_is_the_return_ratio_of_the_vccs_on_the_closed_wire():
    c = LG.loop()
    T, _, _ = LG.loop_gain(c, FREQS)
    rr = LG.return_ratio(c, FREQS)
    assert np.max(np.abs(T - rr)) <= 1e-10, np.abs(T - rr)
    assert abs(T[2] - (0.1505855491 - 0.8066162109j)) <= 1e-9      # at 1e8 Hz, the figure the definition was checked with


def test_T_is_the_two_port_expression():
    c = LG.loop()
    T, _, _ = LG.loop_gain(c, FREQS)
    assert np.max(np.abs(T - LG.two_port(c, FREQS))) <= 1e-10
    for f in FREQS[1:]:   # injecting the current at y instead of x gives the same two-port
        a, b = LG.two_port_matrix(c, f), LG.two_port_matrix(c, f, inject_at_y=True)
        assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(a))


def test_dc_loop_gain_is_two_and_the_reversed_probe_gives_the_reverse_loop_gain():
    T, _, _ = LG.loop_gain(LG.loop(), [0.0])
    assert abs(T[0] - 2.0) <= 1e-13
    c = LG.loop(reverse=True)
    Tr, _, _ = LG.loop_gain(c, FREQS)
    assert abs(Tr[0] - (-0.4)) <= 1e-13
    # (y21 - y12) / (y11 + y22 + 2 y12) of the forward two-port: the direction matters
    fwd = LG.loop()
    for k, f in enumerate(FREQS):
        yp = LG.two_port_matrix(fwd, f)
        assert abs(Tr[k] - (yp[1, 0] - yp[0, 1]) / (yp[0, 0] + yp[1, 1] + 2.0 * yp[0, 1])) <= 1e-10


def test_ideal_unilateral_loop_gives_its_gain():
    for gain in (0.5, 3.0, 1e4):
        T, _, Tl = LG.loop_gain(LG.unilateral(gain), [0.0, 1e9])
        assert np.max(np.abs(T - gain)) <= 1e-12 * gain and np.max(np.abs(Tl - gain)) <= 1e-9 * gain


def test_derivatives_match_richardson_differences_of_the_reference_itself():
    c = LG.loop()
    names = ["r2", "cg", "gm", "r1"]
    slots = [c.slots[c.slot(nm)] for nm in names]
    f = FREQS[[0, 2, 3]]
    _, dT, _ = LG.loop_gain(c, f, slots=slots)
    for k, slot in enumerate(slots):
        p = c.dev_par[slot[1]][slot[2]]
        y = []
        for rel in (1e-3, 5e-4):
            Tp, _, _ = LG.loop_gain(cases.at_params(c, {c.slot(names[k]): p * (1 + rel)}), f)
            Tm, _, _ = LG.loop_gain(cases.at_params(c, {c.slot(names[k]): p * (1 - rel)}), f)
            y.append((Tp - Tm) / (2 * rel * p))
        r = (4.0 * y[1] - y[0]) / 3.0
        assert np.max(np.abs(dT[:, k] - r)) <= 1e-9 * np.max(np.abs(r)), (names[k], dT[:, k], r)
    # gm enters T linearly: dT/dgm = T / gm
    T, _, _ = LG.loop_gain(c, f)
    assert np.max(np.abs(dT[:, 2] - T / LG.GM)) <= 1e-12 * np.max(np.abs(T / LG.GM))


def test_shape_cases_have_the_sizes_and_pass_the_e_cpu_cap():
    """4, 64, 96 and 97 unknowns: the probe is AC-driven, so no node or branch is folded and the engine's count is the MNA size."""
    for n in (4, 64, 96, 97):
        c, T, e_cpu, tol = LG.shape_case(n)
        assert c.n_mna == n
        print("loop(%d): e_cpu %.2e, tolerance %.2e" % (n, e_cpu, tol))
        assert e_cpu <= cases.E_CPU_MAX and tol <= cases.TOL_CEILING
