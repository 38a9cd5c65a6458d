"""The yardstick of the transient sensitivities (tests/transens_reference.py) against closed forms, on the CPU oracle alone: a series
R into a grounded C driven by a DC source, from x0 = 0.  At order 1 on a uniform grid h the discrete solution is
v_n = V (1 - (1 + h/RC)^-n), and the replay's dv_n/dR, dv_n/dC, dv_n/dV must be the derivatives of THAT formula (1e-10 relative: the
frozen-step meaning of the derivative).  At orders up to 5 on a fine grid they converge to the derivatives of V (1 - exp(-t/RC));
halving h at order 2 cuts the error fourfold."""
import numpy as np
import pytest

from cedarsim_jl_amd import Circuit

from transens_reference import Replay, bdf_alpha, lagrange_rows

V, R, Cc = 2.0, 1e3, 1e-9
TAU = R * Cc


@pytest.fixture(scope="module")
def rc(oracle_lib):
    from oracle_binding import Oracle
    c = Circuit()
    c.V("v", "in", 0, dc=V)
    c.R("r", "in", "out", R)
    c.C("c", "out", 0, Cc)
    ids = [c.slot("r"), c.slot("c"), c.slot("v")]
    return c, ids, Replay(Oracle(c), c, ids), c.mna_index("v", "out")


def replay_uniform(rp, n_steps, h, order):
    t = h * np.arange(n_steps + 1)
    orders = [0] + [min(i, order) for i in range(1, n_steps + 1)]
    return t, rp.run(t, orders, np.zeros(rp.n))


def continuous(t):
    e = np.exp(-t / TAU)
    return np.array([-V * e * t / (R * TAU), -V * e * t / (Cc * TAU), 1.0 - e])   # d/dR, d/dC, d/dV of V (1 - exp(-t/RC))


def test_bdf_coefficients_and_lagrange_rows():
    assert bdf_alpha(1.0, [0.5]) == pytest.approx([2.0, -2.0])
    assert bdf_alpha(2.0, [1.0, 0.0]) == pytest.approx([1.5, -2.0, 0.5])        # uniform BDF2
    a = bdf_alpha(1.0, [0.6, 0.1, -0.5])
    assert sum(a) == pytest.approx(0.0, abs=1e-12)                               # a constant has derivative 0
    assert sum(x * y for x, y in zip(a, [1.0, 0.6, 0.1, -0.5])) == pytest.approx(1.0)   # d/dt of t is 1
    t = np.array([0.0, 1.0, 2.0, 4.0])
    y = np.stack([t ** 2, 3.0 * t], axis=1)
    out = lagrange_rows(t, [0, 2, 3, 3], y, [0.0, 0.5, 1.5, 3.0, 4.0])
    assert out[:, 1] == pytest.approx([0.0, 1.5, 4.5, 9.0, 12.0])
    assert out[:, 0] == pytest.approx([0.0, 0.5, 2.25, 9.0, 16.0])              # linear inside the first step, exact parabola behind it


def test_order_one_is_the_derivative_of_the_discrete_solution(rc):
    c, ids, rp, out = rc
    n, h = 12, 0.3 * TAU
    t, (x, s) = replay_uniform(rp, n, h, 1)
    k = np.arange(n + 1)
    a = 1.0 + h / TAU
    assert x[:, out] == pytest.approx(V * (1.0 - a ** -k), rel=1e-12, abs=1e-15)
    exact = np.array([V * k * a ** (-k - 1.0) * (-h / (R * TAU)), V * k * a ** (-k - 1.0) * (-h / (Cc * TAU)), 1.0 - a ** -k])
    for j, name in enumerate(("r", "c", "v")):
        err = np.max(np.abs(s[:, j, out] - exact[j])) / np.max(np.abs(exact[j]))
        print("order 1, d/d%s: max relative error %.3e" % (name, err))
        assert err <= 1e-10, (name, err)
    # and NOT the continuous derivative: at this step the two differ by far more than the bound above
    assert np.max(np.abs(exact[0] - continuous(t)[0])) / np.max(np.abs(exact[0])) > 1e-2


def test_higher_orders_converge_to_the_continuous_sensitivity(rc):
    c, ids, rp, out = rc
    T = 2.0 * TAU

    cache = {}

    def err(order, n):
        if (order, n) not in cache:
            t, (x, s) = replay_uniform(rp, n, T / n, order)
            ref = continuous(t)
            cache[order, n] = np.array([np.max(np.abs(s[:, j, out] - ref[j])) / np.max(np.abs(ref[j])) for j in range(3)])
        return cache[order, n]

    # (the start-up steps run at orders 1, 2, ... and their O(h^2) error is what remains at orders 3 to 5)
    for order in (1, 2, 3, 4, 5):
        e1, e2 = err(order, 100), err(order, 200)
        print("order %d: errors %s -> %s" % (order, e1, e2))
        assert np.all(e2 < e1) and np.all(e2 < (2e-2 if order == 1 else 1e-3))
    ratio = err(2, 100) / err(2, 200)
    print("order 2, halving h: error ratios %s" % ratio)
    assert np.all(ratio >= 3.5) and np.all(ratio <= 4.5), ratio
