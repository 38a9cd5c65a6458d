"""CPU tests of tests/step_defect.py, the yardstick of tests/test_gpu_step_defect.py: the helper against a float64 variable-step,
variable-order BDF written here (it must call a correct solve correct, and see a matrix entry wrong by 1e-10), and the conditions
the GPU tests rest on, checked on the oracle before anything reaches a GPU: every transient case is excited (the median step moves
the state by >= 1e-2 of its size, every unknown covers >= 1e-3 of the largest magnitude of its kind), and the Newton iteration
counts the nonlinear operating points are held to do not sit on a rounding boundary."""
import numpy as np
import pytest

from cedarsim_jl_amd import dc_opts, tran_opts

import step_defect as sd
import step_defect_cases as sc

RATIOS = (2.0, 0.5, 1.5, 2.0, 0.25, 2.0, 1.0 / 1.5, 1.0)      # product 1: the step neither grows nor dies over a cycle
ORDERS = (1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 3, 5)


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def solve(A, b):
    """LAPACK's solve and one step of iterative refinement, all in float64.  Partial pivoting alone is backward stable in the norm,
    not row by row: on the mixed circuit (rows of 1's beside rows of 5e-4 S) it leaves w = 3.7e-15 in the KCL row of a node between a
    floating source and a resistor.  One refinement step with the residual in working precision makes it componentwise stable
    (Skeel 1980), which is the sense `step_defects` measures in."""
    x = np.linalg.solve(A, b)
    return x + np.linalg.solve(A, b - A @ x)


def float64_bdf(G, C, s, h0, n_steps, spoil=None):
    """Variable-step, variable-order BDF in float64 from the operating point at t = 0: (t, orders, X).  spoil = (row, column,
    factor): that entry of G + a0 C is scaled in the solve alone."""
    t, orders, X = [0.0], [0], [solve(G, s(0.0))]
    h = h0
    for i in range(1, n_steps + 1):
        k = min(i, ORDERS[(i - 1) % len(ORDERS)])
        tn = t[-1] + h
        a = [float(v) for v in sd.bdf_alpha(tn, t[::-1][:k])]
        rhs = s(tn)
        for j in range(1, k + 1):
            rhs = rhs - a[j] * (C @ X[i - j])
        A = G + a[0] * C
        if spoil:
            A[spoil[0], spoil[1]] *= spoil[2]
        X.append(solve(A, rhs))
        t.append(tn)
        orders.append(k)
        h *= RATIOS[(i - 1) % len(RATIOS)]
    return np.array(t), np.array(orders), np.array(X)


@pytest.mark.parametrize("which", ["mixed", "mesh9"])
def test_helper_passes_a_float64_bdf_and_sees_an_entry_wrong_by_1e_10(O, which):
    c = sc.TRAN_CASES[which]["build"]()
    G, C, s = sd.linear_parts(O(c))
    h0 = sc.TRAN_CASES[which]["dtmax"] / 2
    t, orders, X = float64_bdf(G, C, s, h0, 36)
    assert set(orders[1:]) == {1, 2, 3, 4, 5}
    ratios = np.diff(t)[1:] / np.diff(t)[:-1]
    assert abs(ratios.min() - 0.25) < 1e-9 and abs(ratios.max() - 2.0) < 1e-9
    w = sd.step_defects(t, orders, X, G, C, s)
    wr = sd.reference_defects(t, orders, X, G, C, s)
    print("%s: float64 BDF worst w = %.3e (numpy restatement from the same rows: %.3e)" % (which, w.max(), wr.max()))
    assert w.max() <= 2.0 ** -50
    # one diagonal entry of the matrix, of a node the source drives, wrong by a relative 1e-10 in the solve
    p = c.mna_index("v", "a" if which == "mixed" else "n1")
    t2, o2, X2 = float64_bdf(G, C, s, h0, 36, spoil=(p, p, 1.0 + 1e-10))
    w2 = sd.step_defects(t2, o2, X2, G, C, s)
    print("%s: with G[%d][%d] scaled by 1 + 1e-10 in the solve: worst w = %.3e" % (which, p, p, w2.max()))
    assert w2.max() > 1e-12
    # ... and the operating point
    x0 = np.linalg.solve(G, s(0.0, 0))
    assert sd.dc_defect(x0, G, s(0.0, 0)) <= 2.0 ** -50 and sd.dc_reference_defect(G, s(0.0, 0)) <= 2.0 ** -50
    Gs = G.copy()
    Gs[p, p] *= 1.0 + 1e-10
    assert sd.dc_defect(np.linalg.solve(Gs, s(0.0, 0)), G, s(0.0, 0)) > 1e-12


def test_unobserved_columns_take_their_rows_out(O):
    """A grounded source's branch current is not observed: its node's KCL row is not checked, every other row is."""
    c = sc.mixed_linear()
    G, C, s = sd.linear_parts(O(c))
    t, orders, X = float64_bdf(G, C, s, 1e-7, 8)
    br = c.mna_index("i", "v1")
    X[:, br] = np.nan
    rows = sd.observable_rows(X, G, C)
    assert c.mna_index("v", "in") not in rows and br in rows and len(rows) == c.n_mna - 1
    assert sd.step_defects(t, orders, X, G, C, s).max() <= 2.0 ** -50
    assert sd.reference_defects(t, orders, X, G, C, s).max() <= 2.0 ** -50
    X[:, c.mna_index("v", "b")] = np.nan                     # a node that carries charge: the history cannot be formed
    with pytest.raises(AssertionError):
        sd.step_defects(t, orders, X, G, C, s)


def test_bdf_alpha_is_exact_to_the_longdouble(O):
    """Uniform steps give the textbook coefficients; the coefficients of any grid sum to zero (a constant has no derivative)."""
    a = sd.bdf_alpha(3.0, [2.0, 1.0])
    assert [float(v) for v in a] == [1.5, -2.0, 0.5]
    a = sd.bdf_alpha(1.0, [1.0 - 2.0 ** -30, 0.5, -0.25, -1.0, -1.5])
    assert abs(sum(a)) <= 8 * np.finfo(np.longdouble).eps * sum(abs(v) for v in a)


def test_linear_parts_refuses_a_mosfet(O):
    with pytest.raises(ValueError):
        sd.linear_parts(O(sc.mos_mesh(7)))
    G, C, s = sd.linear_parts(O(sc.linear_mesh(7)))          # the same mesh without them is fine
    assert G.shape == (9, 9) and np.count_nonzero(C) == 7


@pytest.mark.parametrize("name", list(sc.TRAN_CASES))
def test_every_transient_case_is_excited_on_the_oracle(O, name):
    case = sc.TRAN_CASES[name]
    c = case["build"]()
    o = O(c)
    rc, t, v, _, st = o.tran(case["span"][0], case["span"][1], tran_opts(dtmax=case["dtmax"], **case["tol"]))
    assert rc == 0 and 12 <= len(t) - 1 <= 60 and np.all(np.diff(t) > 0)
    med, move = sd.excitation(sc.rows_to_mna(c, v), sc.unknown_columns(c), c.n_nodes)
    print("%s: %d steps, median step %.3e of max|x|, least-moved unknown %.3e of its kind's size" % (name, len(t) - 1, med, move))
    assert med >= 1e-2 and move >= 1e-3
    sd.linear_parts(o)                                       # and it is linear


def test_hub_ladder_matrices_match_the_oracle_at_40(O):
    c = sc.hub_ladder(40, 10)
    G, C, s = sd.linear_parts(O(c))
    Gs, Cs, ss = sc.hub_ladder_matrices(40, 10)
    assert c.n_mna == 43 and c.mna_index("v", "hub") == 41 and c.mna_index("i", "vin") == 42
    assert np.allclose(Gs.toarray(), G, rtol=4e-16, atol=0) and np.allclose(Cs.toarray(), C, rtol=4e-16, atol=0)
    for t in (0.0, 3e-10, 1e-9, 5e-9):
        assert np.array_equal(ss(t), s(t))
    assert np.array_equal(ss(0.0, 0), s(0.0, 0))
    # the sparse route of the helper gives what the dense one gives
    rng = np.random.default_rng(3)
    x0 = rng.uniform(0.0, 1.0, 43)
    X = [x0]
    tt = [0.0, 2e-10, 5e-10, 1.1e-9, 2e-9]
    for i in range(1, len(tt)):
        a0 = 1.0 / (tt[i] - tt[i - 1])
        X.append(np.linalg.solve(G + a0 * C, s(tt[i]) + a0 * (C @ X[-1])))
    orders = [0, 1, 1, 1, 1]
    wd, ws = sd.step_defects(tt, orders, X, G, C, s), sd.step_defects(tt, orders, X, Gs, Cs, ss)
    assert wd.max() <= 2.0 ** -50 and ws.max() <= 2.0 ** -50 and np.array_equal(wd > 0, ws > 0)   # (the two G differ in last bits)
    assert sd.reference_defects(tt, orders, X, Gs, Cs, ss).max() <= 2.0 ** -50


@pytest.mark.parametrize("n", sc.DC_MESH_SIZES)
def test_nonlinear_operating_point_counts_do_not_sit_on_a_rounding_boundary(O, n):
    """The oracle's Newton count from the perturbed start is the same at abstol, ten times it and a tenth of it.  (abstol 1e-12:
    at 1e-10 the 7-node mesh sits within a factor six of the boundary, its residual after one iteration being 5.7e-10.  From 12
    nodes on the mesh's MOSFETs are cut off at its operating point, the residual falls from 1e-4 to 1e-18 in one iteration and the
    count is one: there the count sees a linear solve wrong by more than 1e-12 / 1e-4 = 1e-8.)"""
    c = sc.mos_mesh(n)
    o = O(c)
    rc, x_op, _ = o.dc(dc_opts(abstol=1e-14))
    assert rc == 0
    unknown = [False] + [c.mna_index("v", nm) in sc.unknown_columns(c) for nm in c.node_names[1:]]
    x0 = sc.perturbed_start(c, x_op, unknown)
    counts = []
    for tol in (sc.DC_ABSTOL, sc.DC_ABSTOL * 10, sc.DC_ABSTOL / 10):
        rc, x, st = o.dc(dc_opts(abstol=tol, x0=x0, dv_max=0, n_restarts=1))
        assert rc == 0 and st["nrestarts"] == 0
        counts.append(st["nnonliniter"])
    print("mesh of %d with MOSFETs: %d Newton iterations at abstol %g, x10, /10: %s" % (n, counts[0], sc.DC_ABSTOL, counts))
    assert counts[0] == counts[1] == counts[2] >= 1
