"""Pins the numpy + mpmath small-signal reference (smallsignal_reference.py) before any kernel is judged by it: closed
forms, the oracle on every case of smallsignal_cases.py, its banded solver against its dense one, its analytic
sensitivities against differences of its own solves — and the condition every case has to meet: two CPU double-precision
solvers reproduce the refined solution to 1e-11 (`e_cpu`), so a correct double LU has room below the GPU tolerance
max(1e-12, 32 e_cpu).  If a seed gives a worse-conditioned system, change the seed, not the bound.  CPU only."""
import math

import numpy as np
import pytest

import smallsignal_cases as cases
import smallsignal_reference as ref
from cedarsim_jl_amd import acdec

from test_ac_noise_oracle import C2, L1, L3, R4, butterworth_circuit


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def test_butterworth_closed_forms():
    c = butterworth_circuit()
    out, l3 = c.mna_index("v", "vout"), c.mna_index("i", "l3")
    par = lambda a, b: a * b / (a + b)  # noqa: E731
    for f in acdec(4, 0.01, 10):
        s = 2j * math.pi * f
        H = 1.0 / ((s + 1) * (s * s + s + 1))
        x, _, _ = ref.solve(*ref.mna(c, 2 * math.pi * f))
        assert abs(x[out] - H) <= 1e-12 * abs(H)
        assert abs(x[c.mna_index("v", "vin")] - 1.0) <= 1e-15
        assert abs(x[l3] - H) <= 1e-12 * abs(H)            # the load R4 || R5 = 1 Ohm carries l3's current
        Z = par(par(s * L1, 1 / (s * C2)) + s * L3, R4)
        apsd = abs(4 * ref.K_BOLTZMANN * (23 + 273.15) / R4 * Z * Z)
        assert ref.noise_psd(c, out, 2 * math.pi * f) == pytest.approx(apsd, rel=1e-12)


def _check_case(O, key, c, freqs, noise_rows, groups=None):
    r = cases.ac_reference(key, c, freqs, O, groups)
    print("%s: e_lapack %.2e, e_oracle %.2e" % (key, r["e_lapack"].max(), r["e_oracle"].max()))
    assert r["e_cpu"] <= cases.E_CPU_MAX, (key, r["e_lapack"], r["e_oracle"])
    tol = cases.tolerance(r["e_cpu"])
    nz = freqs[freqs > 0.0]
    for row in noise_rows:
        want = cases.noise_reference(key, c, row, nz)
        rc, got = O(c).noise(row, nz)
        assert rc == 0 and np.all(want >= 0.0)
        assert np.all(np.abs(got - want) <= 2.0 * tol * want), (key, row, np.max(np.abs(got - want) / want))


@pytest.mark.parametrize("n", cases.LADDER_SIZES)
def test_ladder_agrees_with_the_oracle_and_is_well_conditioned(O, n):
    c = cases.ladder(n)
    assert c.n_mna == n                                   # every MNA row is an engine unknown while the source is AC-driven
    rows = [c.mna_index("v", c.far)] + ([c.mna_index("i", c.mid_l)] if c.mid_l else [])
    _check_case(O, ("ladder", n), c, cases.ladder_freqs(n), rows)


def test_pivot_torture_agrees_with_the_oracle_and_is_well_conditioned(O):
    c = cases.pivot_torture()
    assert c.n_mna == 15
    Y, _ = ref.mna(c, 0.0)
    assert np.sum(np.diag(Y) == 0.0) >= 7                 # four source rows, two inductor rows, the gyrator node q
    Y, _ = ref.mna(c, 2 * math.pi * 1e-3)
    br = [c.mna_index("i", nm) for nm in ("la", "lb")]
    assert all(0.0 < abs(Y[k, k]) <= 1e-6 * np.max(np.abs(Y[:, k])) for k in br)
    _check_case(O, "pivot", c, cases.FREQS, [c.mna_index("v", "c"), c.mna_index("v", "q"), c.mna_index("i", "vf")])


def test_blocks_agree_with_the_oracle_and_are_well_conditioned(O):
    c = cases.blocks()
    groups = cases.block_groups(c)
    assert [len(groups[2 * k]) + len(groups[2 * k + 1]) for k in range(5)] == cases.BLOCK_SIZES
    assert sorted(i for g in groups for i in g) == list(range(c.n_mna))
    rows = [c.mna_index("v", nm) for nm in ("u1", c.block_nodes[3][-1], c.block_nodes[4][-1])]
    slots, values = c.sweep
    for s in range(3):
        cs = cases.at_params(c, {slots[0]: values[0][s], slots[1]: values[1][s]})
        _check_case(O, ("blocks", s), cs, cases.FREQS, rows if s == 0 else [], groups)
    r = cases.ac_reference(("blocks", 0), c, cases.FREQS, O, groups)
    assert np.all(r["x"][:, groups[0]] == 0.0)            # the undriven block


def test_offset_source_agrees_with_the_oracle(O):
    c = cases.offset_source()
    _check_case(O, "offset", c, cases.FREQS, [c.mna_index("v", "b")], cases.offset_groups(c))
    r = cases.ac_reference("offset", c, cases.FREQS, O, cases.offset_groups(c))
    H = 1.0 / (1.0 + 2j * math.pi * cases.FREQS * c.rc)
    assert np.allclose(r["x"][:, c.mna_index("v", "b")] / 1e-3, H, rtol=1e-14, atol=0.0)


def test_banded_solver_agrees_with_the_dense_refined_solve(O):
    """The Thomas recurrence (complex128, vectorised over frequency) and its 40-digit form against the dense refined solve
    of a 40-section RC ladder; then the conditions of the chunking ladder at its four 40-digit frequencies."""
    from cedarsim_jl_amd import Circuit
    rng = np.random.default_rng(5)
    rs, cs_ = rng.uniform(0.5e3, 2e3, 40), rng.uniform(0.5e-12, 2e-12, 40)
    c = Circuit()
    c.V("vin", "n0", 0, dc=0.0, ac=1.0)
    for i in range(40):
        c.R("r%d" % (i + 1), "n%d" % i, "n%d" % (i + 1), rs[i])
        c.C("c%d" % (i + 1), "n%d" % (i + 1), 0, cs_[i])
    freqs = np.array([0.0, 1e4, 1e7, 1e9, 1e11])
    v, i = ref.rc_ladder_ac(rs, cs_, 2 * np.pi * freqs)
    nodes = [c.mna_index("v", "n%d" % k) for k in range(1, 41)]
    for k, f in enumerate(freqs):
        x, _, _ = ref.solve(*ref.mna(c, 2 * np.pi * f))
        vm, im = ref.rc_ladder_mp(rs, cs_, 2 * np.pi * f)
        # the dense system holds 1/R and the diagonal sums rounded to double, the recurrences divide by R themselves: at DC
        # the matrix is a bare Laplacian of condition N^2, which is what a rounding of its entries is amplified by
        bound = 40 * 40 * 2.0 ** -52
        assert np.max(np.abs(v[k] - x[nodes])) <= bound * np.max(np.abs(x[nodes]))
        assert np.max(np.abs(vm - x[nodes])) <= bound * np.max(np.abs(x[nodes]))
        if f > 0.0:    # at DC nothing loads the ladder: the source current is 0 up to rounding
            assert abs(i[k] - x[c.mna_index("i", "vin")]) <= bound * abs(im) and abs(im - x[c.mna_index("i", "vin")]) <= bound * abs(im)
            want = ref.noise_psd(c, c.mna_index("v", "n17"), 2 * np.pi * f)
            assert ref.rc_ladder_noise(rs, cs_, [2 * np.pi * f], 17, c.temp)[0] == pytest.approx(want, rel=1e-12)
            assert ref.rc_ladder_noise_mp(rs, cs_, 2 * np.pi * f, 17, c.temp) == pytest.approx(want, rel=1e-12)
    # the chunking ladder: the Thomas solve and the oracle (both samples) against the 40-digit recurrence
    c = cases.chunk_ladder()
    r = cases.chunk_reference(c, 366, O)
    print("chunk ladder: e_thomas %.2e, e_oracle %.2e" % (r["e_thomas"], r["e_oracle"]))
    assert r["e_cpu"] <= cases.E_CPU_MAX
    cases.tolerance(r["e_cpu"])


@pytest.mark.parametrize("n", cases.SENS_SIZES)
def test_analytic_sensitivities_agree_with_differences_of_refined_solves(n):
    """dx/dp of the reference against a central difference of its own refined operating points, taken at 40 digits, on
    the sensitivity ladders.  The perturbed systems are stamped in double: a diagonal of 1e-2 S carries a rounding of
    1e-18 S, the perturbation of a 1e-6 S shunt at the relative step 3e-5 is 3e-11 S, so the difference is good to 3e-8;
    its truncation is 1e-9.  Bound 1e-7.  And the conditions the GPU test needs: at DC the far node stays above 1e-9 of the
    source, and the reference's own value for a resistor without DC current is below the absolute bound of such a slot."""
    c = cases.ladder(n, dc=1.0)
    names = cases.sens_slot_names(c, n)[:12]
    ids = [c.slot(nm) for nm in names]
    x, s = ref.dc_sens(c, [c.slots[i] for i in ids])
    assert abs(x[c.mna_index("v", c.far)]) >= 1e-9
    assert x[c.mna_index("v", "n0")] == 1.0
    print("ladder(%d): far node / source %.2e" % (n, abs(x[c.mna_index("v", c.far)])))
    for k, nm in enumerate(names):
        if cases.carries_no_dc_current(c, nm):
            assert np.max(np.abs(s[k])) <= cases.zero_slot_bound(c, names, s), nm
    for k in (0, 5, 10, 11):
        p, h = cases.base_value(c, ids[k]), 3e-5 * abs(cases.base_value(c, ids[k]))
        _, xp, _ = ref.solve(*ref.mna(cases.at_params(c, {ids[k]: p + h}), 0.0, "dc"))
        _, xm, _ = ref.solve(*ref.mna(cases.at_params(c, {ids[k]: p - h}), 0.0, "dc"))
        fd = np.array([float((a - b).real / (2 * h)) for a, b in zip(xp, xm)])
        assert np.max(np.abs(fd - s[k])) <= 1e-7 * np.max(np.abs(s[k])), names[k]
    assert np.all(s[10][c.mna_index("v", "n0")] == 1.0)
