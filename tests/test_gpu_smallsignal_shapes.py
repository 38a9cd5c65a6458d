"""GPU tests of ch_ac / ch_noise / ch_dc_sens at the shape edges of `ac_block_kernel` and `sens_block_kernel`: every size
at which the solvers change regime (64 | 65: fused path | sparse path, 96 | 97: LDS | global workspace, 256 | 257: a second
trip of the 256-thread loops), blocks of unequal size with several samples, systems whose diagonal is useless for pivoting,
branch-current noise outputs, a small AC magnitude on a large DC value, and a sweep whose workspace takes two launches.

The reference (smallsignal_reference.py) is a numpy stamp of the full MNA system refined to 40 digits; it shares nothing
with the engine or the oracle and is itself pinned by test_smallsignal_reference.py.  Tolerance of a case:
max(1e-12, 32 e_cpu) of the largest phasor (node voltages and branch currents scaled apart), where e_cpu is the error
the oracle and LAPACK make on the same systems, measured in the fixture; PSDs relative, at twice that
(smallsignal_cases.tolerance).  Sensitivities: the tolerances of test_gpu_dc_sens.test_ladder_of_100_sections.
Everything goes through the public entry points."""
import math

import numpy as np
import pytest

import smallsignal_cases as cases
import smallsignal_reference as ref
from cedarsim_jl_amd import dc_opts

from test_ac_noise_oracle import butterworth_circuit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def opts(c, samples=1):
    """abstol 1e-12 and a zero start: a linear circuit is then solved by one Newton step that is the solution itself, the
    same for every sample index."""
    return dc_opts(abstol=1e-12, x0=np.zeros((samples, c.n_mna)))


def forced_sparse(monkeypatch, fn):
    monkeypatch.setenv("CEDARHIP_FORCE_SPARSE", "1")
    try:
        return fn()
    finally:
        monkeypatch.delenv("CEDARHIP_FORCE_SPARSE", raising=False)


def expected_path(n):
    return 1 if n <= 64 else 2


def check_ac(what, x, r, tol):
    """x[n_freq][n_mna] against the refined solution, frequency by frequency; returns the worst scaled error."""
    assert x.shape == r["x"].shape and not np.isnan(x).any(), what
    worst = max(ref.scaled_error(x[k], r["x"][k], r["groups"]) for k in range(len(x)))
    print("%s: GPU error %.2e, e_cpu %.2e (LAPACK %.2e, oracle %.2e), tolerance %.2e" % (
        what, worst, r["e_cpu"], r["e_lapack"].max(), r["e_oracle"].max(), tol))
    assert worst <= tol, (what, worst, tol)
    return worst


def check_psd(what, got, want, tol):
    worst = float(np.max(np.abs(got - want) / want))
    print("%s: GPU PSD error %.2e, tolerance %.2e" % (what, worst, 2.0 * tol))
    assert np.all(np.abs(got - want) <= 2.0 * tol * want), (what, worst, tol)


@pytest.fixture(scope="module")
def ladder_case(O):
    """(circuit, frequencies, refined AC solution with e_cpu, tolerance) of ladder(n), computed once."""
    memo = {}

    def get(n):
        if n not in memo:
            c, f = cases.ladder(n), cases.ladder_freqs(n)
            r = cases.ac_reference(("ladder", n), c, f, O)
            memo[n] = (c, f, r, cases.tolerance(r["e_cpu"]))
        return memo[n]
    return get


# ---- AC at the size edges ----
@pytest.mark.parametrize("n", cases.LADDER_SIZES)
def test_ac_at_every_size_edge(E, ladder_case, monkeypatch, n):
    c, f, r, tol = ladder_case(n)
    e = E(c, small_signal=True)
    rc, x, st = e.ac(f, opts(c))
    info = e.info()
    assert rc == 0, e.ctx.last_error()
    assert info["n_unknowns"] == n and info["path"] == expected_path(n) and info["n_components"] == 1
    check_ac("ladder(%d)" % n, x[0], r, tol)
    if n <= 64:   # the same LDS kernel, G and C arriving through csr_to_dense_kernel
        def run():
            e2 = E(c, small_signal=True)
            rc2, x2, _ = e2.ac(f, opts(c))
            return rc2, x2, e2.info()
        rc2, x2, info2 = forced_sparse(monkeypatch, run)
        assert rc2 == 0 and info2["path"] == 2 and info2["n_unknowns"] == n
        check_ac("ladder(%d) forced sparse" % n, x2[0], r, tol)


# ---- noise at the size edges ----
@pytest.mark.parametrize("n", cases.LADDER_SIZES)
def test_noise_at_every_size_edge(E, ladder_case, n):
    """Far node, and a mid-ladder inductor current (out_kind = 1) where the ladder has an inductor.  small_signal=True keeps
    the AC source's node and branch (n unknowns); small_signal=False folds the source into a known node (n - 2 unknowns, or n
    for the two current-driven cells): two structures of the same circuit, each against the adjoint reference and against each
    other.  f = 0 is left out (noise)."""
    c, f, r, tol = ladder_case(n)
    f = f[f > 0.0]
    outs = [(0, c._n(c.far), c.mna_index("v", c.far))]
    if c.mid_l:
        outs.append((1, c.dev_names.index(c.mid_l), c.mna_index("i", c.mid_l)))
    for kind, index, row in outs:
        want = cases.noise_reference(("ladder", n), c, row, f)
        got = {}
        for ss in (True, False):
            e = E(c, small_signal=ss)
            rc, psd, st = e.noise(kind, index, f, opts(c))
            info = e.info()
            assert rc == 0, e.ctx.last_error()
            assert info["n_unknowns"] == (n if ss or n <= 2 else n - 2) and info["path"] == expected_path(info["n_unknowns"])
            check_psd("ladder(%d) noise kind %d small_signal=%s" % (n, kind, ss), psd[0], want, tol)
            got[ss] = psd[0]
        assert np.all(np.abs(got[True] - got[False]) <= 2.0 * tol * want)


# ---- pivoting ----
def test_pivoting_circuit(E, O):
    c = cases.pivot_torture()
    r = cases.ac_reference("pivot", c, cases.FREQS, O)
    tol = cases.tolerance(r["e_cpu"])
    e = E(c, small_signal=True)
    rc, x, st = e.ac(cases.FREQS, opts(c))
    info = e.info()
    assert rc == 0, e.ctx.last_error()
    assert info["n_unknowns"] == 15 and info["n_components"] == 1 and info["path"] == 1
    check_ac("pivot_torture", x[0], r, tol)
    f = cases.FREQS[1:]
    for kind, index, row in ((0, c._n("c"), c.mna_index("v", "c")), (0, c._n("q"), c.mna_index("v", "q")),
                             (1, c.dev_names.index("vf"), c.mna_index("i", "vf"))):
        want = cases.noise_reference("pivot", c, row, f)
        for ss in (True, False):
            rc, psd, st = E(c, small_signal=ss).noise(kind, index, f, opts(c))
            assert rc == 0
            check_psd("pivot_torture noise row %d small_signal=%s" % (row, ss), psd[0], want, tol)


# ---- blocks of unequal size, three samples ----
@pytest.fixture(scope="module")
def blocks_case(O):
    c = cases.blocks()
    groups = cases.block_groups(c)
    slots, values = c.sweep
    at = [cases.at_params(c, {slots[0]: values[0][s], slots[1]: values[1][s]}) for s in range(3)]
    refs = [cases.ac_reference(("blocks", s), at[s], cases.FREQS, O, groups) for s in range(3)]
    return c, at, refs, groups


def test_blocks_of_unequal_size_and_three_samples(E, blocks_case):
    c, at, refs, groups = blocks_case
    slots, values = c.sweep
    e = E(c, small_signal=True)
    e.set_samples(3)
    e.set_params(slots, values)
    rc, x, st = e.ac(cases.FREQS, opts(c, 3))
    info = e.info()
    assert rc == 0, e.ctx.last_error()
    assert info["n_components"] == 5 and info["max_component"] == 64 and info["path"] == 1 and info["n_unknowns"] == sum(cases.BLOCK_SIZES)
    for s in range(3):
        check_ac("blocks sample %d" % s, x[s], refs[s], cases.tolerance(refs[s]["e_cpu"]))
        assert np.all(x[s][:, groups[0]] == 0.0 + 0.0j)                      # the block without a source
    assert not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2])
    # sample 1 has the bits of a one-sample call at its parameters
    e1 = E(c, small_signal=True)
    e1.set_params(slots, [[values[0][1]], [values[1][1]]])
    rc1, x1, _ = e1.ac(cases.FREQS, opts(c))
    assert rc1 == 0 and np.array_equal(x1[0], x[1])
    # noise: output in the first, the 17- and the 64-block in turn, all three samples
    f = cases.FREQS[1:]
    tol = max(cases.tolerance(r["e_cpu"]) for r in refs)
    for k in (0, 3, 4):
        node = c.block_nodes[k][-1]
        rc, psd, st = e.noise(0, c._n(node), f, opts(c, 3))
        assert rc == 0, e.ctx.last_error()
        for s in range(3):
            want = cases.noise_reference(("blocks", s), at[s], c.mna_index("v", node), f)
            check_psd("blocks noise at %s sample %d" % (node, s), psd[s], want, tol)
        if k == 0:      # the swept resistor and capacitor sit in other blocks: not a bit may move
            eb = E(c, small_signal=True)
            rcb, psd_b, _ = eb.noise(0, c._n(node), f, opts(c))
            assert rcb == 0 and all(np.array_equal(psd[s], psd_b[0]) for s in range(3))
    # the inductor current of the 3-block (out_kind 1 in a block that is neither first nor largest)
    rc, psd, st = e.noise(1, c.dev_names.index("wl"), f, opts(c, 3))
    assert rc == 0
    check_psd("blocks noise at wl", psd[2], cases.noise_reference(("blocks", 2), at[2], c.mna_index("i", "wl"), f), tol)


# ---- branch-current output and its refusals ----
def test_noise_branch_output_and_its_refusals(E, O):
    c = butterworth_circuit()
    c.V("vaux", "aux", 0, dc=1.0)            # an unobserved DC source: its branch current is eliminated
    c.R("raux", "aux", 0, 1e3)
    f = np.array([0.01, 0.1, 0.16, 1.0, 10.0])
    e = E(c, small_signal=True)
    rc, psd, st = e.noise(1, c.dev_names.index("l3"), f, opts(c))
    assert rc == 0, e.ctx.last_error()
    assert e.maps()[2][c.branch_devices.index(c.dev_names.index("l3"))] >= 0
    want = np.array([ref.noise_psd(c, c.mna_index("i", "l3"), 2 * math.pi * fk) for fk in f])
    tol = cases.tolerance(cases.ac_reference("butterworth", c, f, O)["e_cpu"])
    check_psd("butterworth l3 current", psd[0], want, tol)
    for index in (c.dev_names.index("r4"), len(c.dev_names), -1):
        rc, _, _ = e.noise(1, index, f, opts(c))
        assert rc == -1 and e.ctx.last_error() == "noise: output device has no branch current"
    rc, _, _ = e.noise(1, c.dev_names.index("vaux"), f, opts(c))
    assert rc == -1 and e.ctx.last_error() == "noise: the output branch current was eliminated (observe it when building the circuit)"
    assert e.maps()[2][c.branch_devices.index(c.dev_names.index("vaux"))] < 0


# ---- small AC on a large DC ----
def test_small_ac_magnitude_on_a_large_dc_value(E, O):
    """b = F(src) - F(src + |ac|) is exact up to the rounding of dc + |ac|: the response scaled by 1/|ac| may be off by
    4 * 2^-52 * (|dc| + |ac|) / |ac| on top of the case tolerance, no more."""
    c = cases.offset_source()
    r = cases.ac_reference("offset", c, cases.FREQS, O, cases.offset_groups(c))
    tol = cases.tolerance(r["e_cpu"])
    dc, ac = 5.0, 1e-3
    e = E(c, small_signal=True)
    rc, x, st = e.ac(cases.FREQS, opts(c))
    assert rc == 0 and e.info()["n_unknowns"] == 3 and e.info()["path"] == 1
    H = 1.0 / (1.0 + 2j * math.pi * cases.FREQS * c.rc)
    err = np.max(np.abs(x[0][:, c.mna_index("v", "b")] / ac - H))
    bound = 4.0 * 2.0 ** -52 * (dc + ac) / ac + tol
    print("offset source: error %.2e, bound %.2e" % (err, bound))
    assert err <= bound
    assert np.max(np.abs(x[0][:, c.mna_index("v", "a")] / ac - 1.0)) <= bound


# ---- frequency chunks of the global workspace ----
def test_frequency_chunks_of_the_global_workspace(E, O):
    c = cases.chunk_ladder()
    S, n_freq = cases.CHUNK_SAMPLES, len(c.freqs)
    e = E(c, small_signal=True)
    e.set_samples(S)
    e.set_params([c.sweep[0]], [c.sweep[1]])
    rc, x, st = e.ac(c.freqs, opts(c, S))
    info = e.info()
    assert rc == 0, e.ctx.last_error()
    # launch_ac (csrc/ch_engine_ac.hpp) caps the workspace of one launch at 2^27 doubles, 2 ds (ds + 1) per system
    ds = info["n_unknowns"]
    per, cap = 2 * ds * (ds + 1), 2 ** 27
    chunk = min(n_freq, cap // (per * S))
    assert info["path"] == 2 and 260 <= ds <= 400
    assert S * n_freq * per > 1.05 * cap and n_freq % chunk != 0 and chunk < n_freq
    r = cases.chunk_reference(c, chunk, O)
    tol = cases.tolerance(r["e_cpu"])
    nodes = [c.mna_index("v", "n%d" % k) for k in range(1, cases.CHUNK_SECTIONS + 1)]
    iv, n0 = c.mna_index("i", "vin"), c.mna_index("v", "n0")
    rcn, psd, _ = e.noise(0, c._n("n%d" % c.out), c.freqs, opts(c, S))
    assert rcn == 0, e.ctx.last_error()
    for s in range(S):
        ev = np.max(np.abs(x[s][:, nodes] - r["v"][s]), axis=1) / np.max(np.abs(r["v"][s]), axis=1)
        ei = np.abs(x[s][:, iv] - r["i"][s]) / np.abs(r["i"][s])
        ep = np.abs(psd[s] - r["psd"][s]) / r["psd"][s]
        print("chunk ladder sample %d: GPU error v %.2e (at f[%d]), i %.2e, PSD %.2e; e_cpu %.2e, tolerance %.2e" % (
            s, ev.max(), int(ev.argmax()), ei.max(), ep.max(), r["e_cpu"], tol))
        assert np.all(ev <= tol) and np.all(ei <= tol) and np.all(ep <= 2.0 * tol)
        assert np.all(np.abs(x[s][:, n0] - 1.0) <= tol)
        for k in r["check"]:    # first, last of the first launch, first of the second launch, last: against 40 digits
            vm, im = r["v_mp"][s, k]
            assert np.max(np.abs(x[s][k][nodes] - vm)) <= tol * np.max(np.abs(vm)) and abs(x[s][k][iv] - im) <= tol * abs(im)
            assert abs(psd[s][k] - r["psd_mp"][s, k]) <= 2.0 * tol * r["psd_mp"][s, k]
    assert not np.array_equal(x[0], x[1])


# ---- sensitivities at the size edges ----
def check_sens(what, s, want, groups, zero_bound=0.0):
    """rtol 1e-8, atol 1e-8 max|dx/dp_k| (test_ladder_of_100_sections), node rows and branch rows each on their own scale.
    A group whose reference does not exceed `zero_bound` is identically zero (a resistor fed by a VCCS alone moves its own
    node and no current): the reference holds rounding noise there, and the device is held to the same absolute bound."""
    for g in groups:
        g = np.asarray(g, dtype=int)
        if g.size and np.max(np.abs(want[g])) <= zero_bound:
            assert np.max(np.abs(s[g])) <= zero_bound, what
        elif g.size:
            assert np.allclose(s[g], want[g], rtol=1e-8, atol=1e-8 * np.max(np.abs(want[g]))), what
    scale = np.max(np.abs(want))
    return np.max(np.abs(s - want)) / scale if scale else 0.0


@pytest.mark.parametrize("n", cases.SENS_SIZES)
def test_sensitivity_solver_at_the_size_edges(E, n):
    """At DC every inductor row has a zero diagonal: sens_block_kernel has to swap rows.  At 96 unknowns every element of the
    ladder is requested — the capacitors and inductors too, whose rows are exactly zero — so that the right-hand sides exceed
    the columns one LDS launch holds.  A trailing series resistor carries no DC current: its column is identically zero and is
    held to an absolute bound (smallsignal_cases.zero_slot_bound)."""
    c = cases.ladder(n, dc=1.0)
    names = cases.sens_slot_names(c, n)
    names = names if n == 96 else names[:12]
    ids = [c.slot(nm) for nm in names]
    xr, want = ref.dc_sens(c, [c.slots[i] for i in ids])
    assert abs(xr[c.mna_index("v", c.far)]) >= 1e-9
    e = E(c, small_signal=True)
    rc, x, s, status, st = e.dc_sens(ids, opts(c))
    info = e.info()
    assert rc == 0 and status[0] == 0, e.ctx.last_error()
    assert info["n_unknowns"] == n and info["path"] == expected_path(n)
    if n == 96:
        # launch_sens (csrc/ch_engine_sens.hpp) gives sens_block_kernel<64> 2*96*97 doubles of LDS; beside the nc x nc matrix
        # sens_lds_columns (csrc/ch_sens_host.hpp) fits budget / nc - nc - 1 right-hand sides: the call takes two chunks, and the
        # second chunk has the bits of a call of its own
        kc = (2 * 96 * 97) // info["n_unknowns"] - info["n_unknowns"] - 1
        assert kc < len(ids) <= 2 * kc
        rc2, _, s2, _, _ = e.dc_sens(ids[kc:], opts(c))
        assert rc2 == 0 and np.array_equal(s[0][kc:], s2[0])
    assert np.allclose(x[0], xr, rtol=1e-9, atol=1e-9)
    worst = 0.0
    zero_bound = cases.zero_slot_bound(c, names, want)
    for k, nm in enumerate(names):
        if cases.carries_no_dc_current(c, nm):
            print("ladder(%d) %s: max|dx/dp| %.2e on the device, %.2e in the reference, bound %.2e" % (
                n, nm, np.max(np.abs(s[0][k])), np.max(np.abs(want[k])), zero_bound))
            assert np.max(np.abs(want[k])) <= zero_bound and np.max(np.abs(s[0][k])) <= zero_bound, nm
            continue
        worst = max(worst, check_sens("ladder(%d) %s" % (n, nm), s[0][k], want[k], ref.unit_groups(c), zero_bound))
        if nm[0] in "cl":
            assert np.all(s[0][k] == 0.0), nm
    print("ladder(%d) sensitivities, %d parameters: worst error %.2e of max|dx/dp_k|" % (n, len(ids), worst))


def test_sensitivities_of_unequal_blocks_and_three_samples(E, blocks_case):
    c, at, _, groups = blocks_case
    slots, values = c.sweep
    names = ["vr1", "xrs3", "yv", "wr2"]          # the 2-, 17-, 64- and 3-block; xrs3 is also swept over the samples
    ids = [c.slot(nm) for nm in names]
    own = [1, 3, 4, 2]
    e = E(c, small_signal=True)
    e.set_samples(3)
    e.set_params(slots, values)
    rc, x, s, status, st = e.dc_sens(ids, opts(c, 3))
    info = e.info()
    assert rc == 0 and np.all(status == 0), e.ctx.last_error()
    assert info["n_components"] == 5 and info["max_component"] == 64 and info["path"] == 1
    for smp in range(3):
        xr, want = ref.dc_sens(at[smp], [c.slots[i] for i in ids])
        assert np.allclose(x[smp], xr, rtol=1e-9, atol=1e-9)
        for k, nm in enumerate(names):
            for b in range(5):
                rows = list(groups[2 * b]) + list(groups[2 * b + 1])
                if b != own[k]:
                    assert np.all(s[smp][k][rows] == 0.0), (nm, b)
                else:
                    assert np.any(want[k][rows] != 0.0)
                    check_sens("blocks sample %d %s" % (smp, nm), s[smp][k], want[k], [groups[2 * b], groups[2 * b + 1]])
    assert not np.array_equal(s[0][1], s[1][1])
