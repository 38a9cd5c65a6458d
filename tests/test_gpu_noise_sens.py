"""GPU tests of the noise PSD parameter sensitivities (ch_noise_sens, direct method on the adjoint system).

Linear circuits: against the analytic yardstick of noisesens_reference.py (numpy stamps, every solve refined at 40 digits, sums in
mpmath) at the shape edges of noisesens_solve_kernel — 64 | 65: fused path | sparse path, 96 | 97: LDS | global workspace,
256 | 257: a second trip of the 256-thread loops.  The error of a (parameter, frequency) is |got - want| / D, D the conditioning
scale sum_e (|2 Re(conj dy_e d(dy)_e)| pwr_e + |dy_e|^2 |dpwr_e|) the yardstick returns; where D = 0 the result must be exactly 0.  The
bound is acsens_reference.tolerance(e_cpu) = max(1e-10, 32 e_cpu), e_cpu being the worst error of the SAME METHOD in numpy doubles
(fd_noise_sens) in the same metric over the case; a case with e_cpu > 1e-7 is refused by that function.  e_cpu is recomputed and
printed with every case.

Nonlinear circuits: against Richardson-extrapolated central differences (relative steps 2e-5 and 1e-5) of full Oracle.noise solves,
oracle DC at abstol 1e-14; for the MOSFETs' own noise, which the oracle does not know, of the engine's own ch_noise_ex (that
yardstick runs on the GPU; the analysis is pinned by test_gpu_b4_noise.py and not changed by ch_noise_sens).  Metric, for the
yardstick's own estimate and the engine alike: the error in dS/dp divided by S(f), scaled by max_f |(dS/dp)/S| of the slot.  A
(slot, frequency) whose estimate exceeds 1e-7 is refused; the engine's tolerance is 1e-6."""
import ctypes as C
import math

import numpy as np
import pytest

import acsens_reference as AR
import noisesens_reference as NR
import smallsignal_cases as cases
from cedarsim_jl_amd import CedarError, Circuit, CircuitSweep, Sweep, dc_opts, noise_sens
from cedarsim_jl_amd.circuit import DEV_C, DEV_L, DEV_R, ERR_UNSUPPORTED

from test_gpu_ac_noise import amp_circuit
from test_gpu_ac_sens import element_names, forced_sparse, pivot_names, spread, PIVOT_CASES
from test_gpu_b4_noise import card, one_fet
from test_gpu_dc_sens import base_value, slot_of

pytestmark = pytest.mark.gpu

F4 = np.array([0.0, 1e3, 1e6, 1e10])   # up to 2 unknowns
F3 = np.array([0.0, 1e3, 1e6])         # from 63 unknowns up: at 1e10 Hz the far node's PSD is 1e-70 and e_cpu reaches 4.5e-4 at ladder(96)


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return lambda c: EngineCircuit(c, small_signal=True)


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def opts(c, samples=1):
    """abstol 1e-12 and a zero start: a linear circuit is solved by one Newton step, the same for every sample index."""
    return dc_opts(abstol=1e-12, x0=np.zeros((samples, c.n_mna)))


def node_out(c, name):
    return 0, c._n(name), c.mna_index("v", name)


def branch_out(c, name):
    return 1, c.dev_names.index(name), c.mna_index("i", name)


def run(e, c, names, out, freqs, o=None, **kw):
    ids = [slot_of(c, nm) for nm in names]
    return e.noise_sens(out[0], out[1], ids, freqs, o or opts(c, e.n_samples), **kw)


# ---- the linear yardstick, computed once per case ----
_REF = {}


def linear_reference(key, c, names, out, freqs):
    """{S[f], want[f][k], D[f][k], e_cpu, tol} of a case."""
    key = (key, tuple(names), out[2], tuple(float(f) for f in freqs))
    if key in _REF:
        return _REF[key]
    slots = [c.slots[slot_of(c, nm)] for nm in names]
    S, want, D, e = [], [], [], []
    for f in freqs:
        w = 2.0 * np.pi * f
        s0, ds, d = NR.noise_sens(c, slots, out[2], w)
        _, g = NR.fd_noise_sens(c, slots, out[2], w)
        S.append(s0), want.append(ds), D.append(d), e.append(NR.scaled_error(g, ds, d))
    e_cpu = float(np.max(e))
    r = dict(S=np.array(S), want=np.array(want), D=np.array(D), e_cpu=e_cpu, tol=AR.tolerance(e_cpu))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REF[key] = r
    return r


def check_linear(what, psd, dpsd, r, freqs, names):
    """psd[n_freq], dpsd[n_freq][n_par] against the yardstick; returns the worst scaled error."""
    assert dpsd.shape == r["want"].shape and not np.isnan(dpsd).any() and not np.isnan(psd).any(), what
    worst = 0.0
    for fi in range(len(freqs)):
        assert abs(psd[fi] - r["S"][fi]) <= 1e-9 * r["S"][fi], (what, freqs[fi])
        err = NR.scaled_error(dpsd[fi], r["want"][fi], r["D"][fi])
        for k in range(len(names)):
            assert err[k] <= r["tol"], (what, freqs[fi], names[k], err[k], r["tol"], dpsd[fi][k], r["want"][fi][k])
        worst = max(worst, float(np.max(err)))
    print("%s: %d parameters x %d frequencies: GPU error %.2e, e_cpu %.2e, tolerance %.2e" % (what, len(names), len(freqs), worst, r["e_cpu"], r["tol"]))
    return worst


def case_names(c, count):
    """`count` elements spread over the device list (all of them when count is None), one multiplier and the temperature."""
    el = element_names(c)
    res = [nm for nm in el if c.dev_kind[c.dev_names.index(nm)] == DEV_R]
    return (el if count is None else spread(el, count)) + [(res[len(res) // 2], "m"), "temp"]


def reactive(c, nm):
    return not isinstance(nm, tuple) and nm != "temp" and c.dev_kind[c.dev_names.index(nm)] in (DEV_C, DEV_L)


# ---- 1. linear shape edges ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 96])
def test_ladders_up_to_96_unknowns(E, monkeypatch, n):
    """noisesens_solve_kernel<64>: every element (n <= 2; with 1e10 Hz) or eight spread over the device list, one multiplier and the
    temperature, at the far node; the fused path and the forced sparse path where both exist; psd_out has the bits of ch_noise."""
    c = cases.ladder(n)
    names, f, out = case_names(c, None if n <= 2 else 8), (F4 if n <= 2 else F3), node_out(c, c.far)
    ids = [slot_of(c, nm) for nm in names]        # declared before the engine circuit is built
    r = linear_reference(("ladder", n), c, names, out, f)
    e = E(c)
    rc, psd, dpsd, ds, status, st = run(e, c, names, out, f)
    info = e.info()
    assert rc == 0, e.ctx.last_error()
    assert info["n_unknowns"] == n and info["path"] == (1 if n <= 64 else 2)
    check_linear("ladder(%d)" % n, psd[0], dpsd[0], r, f, names)
    rcn, psd_n, _ = E(c).noise(out[0], out[1], f, opts(c))
    assert rcn == 0 and np.array_equal(psd_n, psd)                       # first call on a fresh engine circuit against the same
    for k, nm in enumerate(names):                                      # at 0 Hz a capacitance or an inductance does not enter Y at all
        if reactive(c, nm):
            assert dpsd[0][0][k] == 0.0, nm
    if n <= 64:
        def again():
            e2 = E(c)
            return run(e2, c, names, out, f) + (e2.info(),)
        rc2, psd2, dpsd2, _, _, _, info2 = forced_sparse(monkeypatch, again)
        assert rc2 == 0 and info2["path"] == 2 and info2["n_unknowns"] == n
        check_linear("ladder(%d) forced sparse" % n, psd2[0], dpsd2[0], r, f, names)


def on_both_paths(monkeypatch, fn):
    """[(label, result of fn())] on the circuit's own (fused) path and with the sparse path forced; fn returns the engine circuit last."""
    out = []
    for label, call, path in (("", lambda: fn(), 1), (" forced sparse", lambda: forced_sparse(monkeypatch, fn), 2)):
        res = call()
        assert res[-1].info()["path"] == path, (label, res[-1].info()["path"])
        out.append((label, res))
    return out


def test_inductor_current_as_the_output(E, monkeypatch):
    """out_kind = 1, a mid-ladder inductor of ladder(64), on the fused and on the forced sparse path."""
    c = cases.ladder(64)
    names, out = case_names(c, 8), branch_out(c, c.mid_l)
    ids = [slot_of(c, nm) for nm in names]
    r = linear_reference(("ladder-il", 64), c, names, out, F3)

    def once():
        e = E(c)
        return run(e, c, names, out, F3) + (e,)
    for label, (rc, psd, dpsd, _, _, _, e) in on_both_paths(monkeypatch, once):
        assert rc == 0, e.ctx.last_error()
        check_linear("ladder(64), current of %s%s" % (c.mid_l, label), psd[0], dpsd[0], r, F3, names)


@pytest.mark.parametrize("n", [97, 256, 257])
def test_ladders_on_the_global_workspace(E, n):
    """noisesens_solve_kernel<256>: eight parameters at most (six elements, a multiplier, the temperature): the 40-digit yardstick of
    a 257-unknown system is slow."""
    c = cases.ladder(n)
    names, out = case_names(c, 6), node_out(c, c.far)
    ids = [slot_of(c, nm) for nm in names]
    r = linear_reference(("ladder", n), c, names, out, F3)
    e = E(c)
    rc, psd, dpsd, _, _, _ = run(e, c, names, out, F3)
    assert rc == 0, e.ctx.last_error()
    assert e.info()["n_unknowns"] == n and e.info()["path"] == 2
    check_linear("ladder(%d)" % n, psd[0], dpsd[0], r, F3, names)
    for k, nm in enumerate(names):
        if reactive(c, nm):
            assert dpsd[0][0][k] == 0.0, nm
    rc1, psd1, dpsd1, _, _, _ = run(E(c), c, [names[3]], out, F3)
    assert rc1 == 0 and np.array_equal(dpsd1[0][:, 0], dpsd[0][:, 3]) and np.array_equal(psd1, psd)


def test_pivoting_circuit(E, monkeypatch):
    """pivot_torture at node p, on the fused and on the forced sparse path: zero diagonals at 0 Hz and 1 mHz.  Left out, as in
    test_gpu_ac_sens.py and for its reason (a derivative that is structurally zero or nearly so, where the numpy version of the
    method is itself off by more than 1e-7): rl at every frequency; at 0 Hz and 1 mHz also the gyrator gains, cp and rm."""
    c = cases.pivot_torture()
    out = node_out(c, "p")
    sets = [(tag, f, pivot_names(c, without) + ["temp"]) for tag, f, without in PIVOT_CASES]
    for tag, f, names in sets:
        ids = [slot_of(c, nm) for nm in names]
    for tag, f, names in sets:
        r = linear_reference(("pivot", tag), c, names, out, f)

        def once():
            e = E(c)
            return run(e, c, names, out, f) + (e,)
        for label, (rc, psd, dpsd, _, _, _, e) in on_both_paths(monkeypatch, once):
            assert rc == 0, e.ctx.last_error()
            check_linear("pivot_torture " + tag + label, psd[0], dpsd[0], r, f, names)


# ---- 2. panels, batches, blocks: exactness ----
def test_a_column_does_not_depend_on_its_panel(E):
    """ladder(96): the 64-lane kernel holds 8 columns beside the factors and y (ch_noisesens_host.hpp; tests/host_noisesens.cpp
    works the figure out), so 17 parameters are a full panel, a second full panel and a panel of one column.  Every column has the
    bits of the call with that parameter alone."""
    c = cases.ladder(96)
    names, out = spread(element_names(c), 15) + [("rs5", "m"), "temp"], node_out(c, c.far)
    assert len(names) == 2 * 8 + 1
    ids = [slot_of(c, nm) for nm in names]
    rc, psd, dpsd, _, _, _ = run(E(c), c, names, out, F3)
    assert rc == 0 and not np.isnan(dpsd).any()
    for k in (0, 7, 8, 15, 16):
        rc1, psd1, dpsd1, _, _, _ = run(E(c), c, [names[k]], out, F3)
        assert rc1 == 0 and np.array_equal(dpsd1[0][:, 0], dpsd[0][:, k]) and np.array_equal(psd1, psd), names[k]


def test_blocks_do_not_see_each_other(E, monkeypatch):
    """The output in the 3-, the 17- and the 64-block in turn, three samples, on the fused path (five blocks) and on the forced
    sparse path (one system of all 87 unknowns): the derivative with respect to an element of another block is exactly 0; sample 1
    against the yardstick at its own values and bit for bit against a one-sample call."""
    c = cases.blocks()
    names = ["ur", "vr1", "wl", "wr2", "xrs3", "xc2", "yc7", "yrs2", "temp"]
    owner = [0, 1, 2, 2, 3, 3, 4, 4, None]
    ids = [slot_of(c, nm) for nm in names]
    sw_ids, sw_vals = c.sweep
    c1 = cases.at_params(c, {sw_ids[0]: sw_vals[0][1], sw_ids[1]: sw_vals[1][1]})
    for blk in (2, 3, 4):
        out = node_out(c, c.block_nodes[blk][-1])
        r = linear_reference(("blocks-s1", blk), c1, names, out, F3)

        def three():
            e = E(c)
            e.set_samples(3)
            e.set_params(sw_ids, sw_vals)
            return run(e, c, names, out, F3) + (e,)

        def one():
            e1 = E(c)
            e1.set_samples(1)
            e1.set_params(sw_ids, [[v[1]] for v in sw_vals])
            return run(e1, c, names, out, F3) + (e1,)
        for (label, (rc, psd, dpsd, ds, status, st, e)), (_, (rc1, psd1, dpsd1, ds1, _, _, e1)) in zip(on_both_paths(monkeypatch, three),
                                                                                                         on_both_paths(monkeypatch, one)):
            assert rc == 0, e.ctx.last_error()
            assert e.info()["n_components"] == 5 or label
            for k, own in enumerate(owner):
                if own is not None and own != blk:
                    assert not dpsd[:, :, k].any(), (label, blk, names[k])
            check_linear("blocks, output in block %d, sample 1%s" % (blk, label), psd[1], dpsd[1], r, F3, names)
            assert rc1 == 0 and np.array_equal(dpsd1[0], dpsd[1]) and np.array_equal(psd1[0], psd[1]) and np.array_equal(ds1[0], ds[1], equal_nan=True), label


def test_an_output_held_by_a_source_gives_zeros(E):
    c = Circuit()
    c.V("vb", "k", 0, dc=1.0)
    c.R("r1", "k", "a", 1e3)
    c.R("r2", "a", 0, 2e3)
    names = ["r1", "r2", "vb"]
    ids = [slot_of(c, nm) for nm in names]
    e = E(c)
    rc, psd, dpsd, ds, status, _ = run(e, c, names, node_out(c, "k"), F3)
    assert rc == 0 and not psd.any() and not dpsd.any() and psd.shape == (1, 3) and dpsd.shape == (1, 3, 3)
    a = c.mna_index("v", "a")
    assert ds[0][2][a] == pytest.approx(2.0 / 3.0, rel=1e-12) and ds[0][0][a] == pytest.approx(-2e3 / 9e6, rel=1e-9)   # dc_sens_out is served
    rc, psd, dpsd, _, _, _ = run(E(c), c, names, (0, 0, None), F3)     # ground
    assert rc == 0 and not psd.any() and not dpsd.any()


def test_two_frequency_chunks(E):
    """chunk_ladder: 302 unknowns, 2 samples x 400 frequencies, 3 parameters: more than one launch under the workspace cap.  The
    frequencies of the second launch have the bits of a call on those frequencies alone; the two frequencies around the launch
    boundary against the yardstick.  The chunk is the engine's rule (ch_noisesens_host.hpp: the resident part 2 n (n|1) + 2 n, a
    panel 2 n kp and the permutation (n + 1) / 2 per system, S systems per frequency, under 2^27 doubles), not a constant."""
    c = cases.chunk_ladder()
    names, out = ["r8", "c150", "r299"], node_out(c, "n%d" % c.out)
    ids = [slot_of(c, nm) for nm in names]
    n, S = 302, cases.CHUNK_SAMPLES
    per = 2 * n * (n | 1) + 2 * n + 2 * n * len(names) + (n + 1) // 2
    cut = (1 << 27) // (per * S)
    assert 0 < cut < cases.CHUNK_NFREQ

    def engine():
        e = E(c)
        e.set_samples(S)
        e.set_params([c.sweep[0]], [c.sweep[1]])
        return e
    e = engine()
    rc, psd, dpsd, _, _, _ = run(e, c, names, out, c.freqs)
    assert rc == 0, e.ctx.last_error()
    assert e.info()["n_unknowns"] == n and not np.isnan(dpsd).any()
    rc2, psd2, dpsd2, _, _, _ = run(engine(), c, names, out, c.freqs[cut:])
    assert rc2 == 0 and np.array_equal(dpsd2, dpsd[:, cut:]) and np.array_equal(psd2, psd[:, cut:])
    fi = [cut - 1, cut]
    for smp in range(S):
        cs = cases.at_params(c, {c.sweep[0]: c.sweep[1][smp]})
        r = linear_reference(("chunk", smp), cs, names, (out[0], out[1], cs.mna_index("v", "n%d" % c.out)), c.freqs[fi])
        check_linear("chunk_ladder sample %d" % smp, psd[smp][fi], dpsd[smp][fi], r, c.freqs[fi], names)


# ---- 3. nonlinear: the oracle yardstick ----
AMP_SLOTS = ["rd", "vdd", ("rb1", "m"), ("m1", "w"), ("m1", "l"), ("nfet_06v0", "vth0"), "temp", "co", "rs", "ro"]
AMP_FREQS = np.array([1e2, 1e4, 1e6, 1e7, 1e8])
STEPS = (2e-5, 1e-5)
TOL, ADMIT = 1e-6, 1e-7


def richardson(psd_at, p, steps=STEPS):
    """(r, y2): dS/dp [n_freq] extrapolated from central differences of psd_at(value) at the two relative steps, and the finer one."""
    y = []
    for rel in steps:
        h = rel * abs(p)
        y.append((psd_at(p + h) - psd_at(p - h)) / (2.0 * h))
    return (4.0 * y[1] - y[0]) / 3.0, y[1]


def relative_errors(got, r, S):
    """|got - r| / S per frequency, scaled by max_f |r / S|: the metric of the nonlinear cases."""
    return np.abs(got - r) / S / np.max(np.abs(r / S))


def oracle_yardstick(O, c, ids, out_row, freqs):
    """(r[n_slots][n_freq], est[n_slots][n_freq], S[n_freq]) from full Oracle.noise solves, oracle DC at abstol 1e-14."""
    o = O(c)
    rc, xb, _ = o.dc(dc_opts(abstol=1e-14))
    assert rc == 0

    def psd():
        rc, p = o.noise(out_row, freqs, dc_opts(x0=xb, abstol=1e-14))
        assert rc == 0
        return p
    S = psd()
    rs, est = [], []
    for s in ids:
        p = base_value(c, s)

        def at(v):
            o.set_param(s, v)
            return psd()
        r, y2 = richardson(at, p)
        o.set_param(s, p)
        rs.append(r), est.append(relative_errors(y2, r, S))
    return np.array(rs), np.array(est), S


def assert_close(got, r, S, names, freqs, what, admitted):
    worst = np.zeros(len(names))
    for k, nm in enumerate(names):
        err = relative_errors(got[:, k], r[k], S)
        for fi, f in enumerate(freqs):
            if admitted[k][fi]:
                assert err[fi] <= TOL, (what, nm, f, err[fi])
                worst[k] = max(worst[k], err[fi])
    print(what + ": " + ", ".join("%s %.2e" % (nm, w) for nm, w in zip(names, worst)))
    return worst


def amp_both_paths(E, monkeypatch, c, ids, out, r, S, admitted, what):
    e = E(c)
    rc, psd, dpsd, _, _, _ = e.noise_sens(0, c._n(out), ids, AMP_FREQS, dc_opts(abstol=1e-12))
    assert rc == 0, e.ctx.last_error()
    assert e.info()["path"] != 2 and np.allclose(psd[0], S, rtol=1e-6, atol=0.0)
    assert_close(dpsd[0], r, S, AMP_SLOTS, AMP_FREQS, what + ", fused path", admitted)

    def again():
        e2 = E(c)
        return e2.noise_sens(0, c._n(out), ids, AMP_FREQS, dc_opts(abstol=1e-12)) + (e2.info(),)
    rc2, psd2, dpsd2, _, _, _, info2 = forced_sparse(monkeypatch, again)
    assert rc2 == 0 and info2["path"] == 2
    assert_close(dpsd2[0], r, S, AMP_SLOTS, AMP_FREQS, what + ", sparse path", admitted)


@pytest.fixture(scope="module")
def amp_d(O):
    """The amplifier with its slots declared and the oracle yardstick at node d — computed once, shared, never modified."""
    c = amp_circuit()
    ids = [slot_of(c, nm) for nm in AMP_SLOTS]
    r, est, S = oracle_yardstick(O, c, ids, c.mna_index("v", "d"), AMP_FREQS)
    for v in (r, est, S):
        v.setflags(write=False)
    return c, ids, r, est, S


def test_amplifier_at_the_drain_matches_the_oracle_yardstick(E, amp_d, monkeypatch):
    """Output d: the yardstick admits every slot and frequency (measured with the oracle alone: worst estimate 8.8e-9, co).
    Measured on the MI355X, the same on both paths: rd 2.5e-10, vdd 4.5e-10, rb1.m 2.9e-10, m1.w 3.4e-10, m1.l 5.1e-10, vth0 2.2e-10,
    temp 6.2e-10, co 3.3e-8, rs 2.4e-10, ro 1.3e-8."""
    c, ids, r, est, S = amp_d
    print("yardstick's own estimates: " + ", ".join("%s %.1e" % (nm, e.max()) for nm, e in zip(AMP_SLOTS, est)))
    assert np.all(est <= ADMIT), est
    amp_both_paths(E, monkeypatch, c, ids, "d", r, S, est <= ADMIT, "amplifier at d")


# (slot, frequency) pairs of AMP_SLOTS x AMP_FREQS the yardstick refuses at node o: d ln S / d ln vdd = -76 there
O_REFUSED = {"vdd": [1e2, 1e4, 1e6]}


def test_amplifier_at_the_output_matches_the_oracle_yardstick(E, O, monkeypatch):
    """Output o, where the PSD is very steep in the supply: the yardstick refuses vdd at the three lowest frequencies (estimates
    1.5e-7, 1.5e-7, 1.3e-7) and admits everything else (<= 6.9e-8).  The test pins exactly that: a pair that starts or stops
    passing the admission fails it.  Measured on the MI355X on the admitted pairs, the same on both paths: rd 6.6e-10, vdd 1.8e-10,
    rb1.m 9.9e-10, m1.w 8.7e-10, m1.l 1.0e-9, vth0 9.9e-10, temp 9.6e-10, co 1.7e-10, rs 9.6e-10, ro 6.7e-10."""
    c = amp_circuit()
    ids = [slot_of(c, nm) for nm in AMP_SLOTS]
    r, est, S = oracle_yardstick(O, c, ids, c.mna_index("v", "o"), AMP_FREQS)
    for nm, e in zip(AMP_SLOTS, est):
        print("yardstick's own estimates, %s: %s" % (nm, " ".join("%.1e" % v for v in e)))
    want = np.array([[f not in O_REFUSED.get(nm, []) for f in AMP_FREQS] for nm in AMP_SLOTS])
    assert np.array_equal(est <= ADMIT, want), (est <= ADMIT)
    amp_both_paths(E, monkeypatch, c, ids, "o", r, S, want, "amplifier at o")


def test_the_explicit_terms_alone_miss_the_yardstick(O, amp_d):
    """With the oracle alone: the formula WITHOUT the bias shift — dY/dp and dpwr/dp at the fixed operating point — is off by more
    than 100 tolerances for rd and vdd at d, so a result within tolerance proves that the state terms are there.  G = J(alpha0 = 0),
    C = J(alpha0 = 1) - G from Oracle.eval at the fixed operating point, dY/dp by central differences through Oracle.set_param at
    that same point; the sources are the resistors' 4kT m / R, whose explicit derivative is analytic."""
    c, ids, r, est, S = amp_d
    o = O(c)
    rc, xb, _ = o.dc(dc_opts(abstol=1e-14))
    xop = np.nan_to_num(xb)
    out = c.mna_index("v", "d")
    table = NR.source_table(c)
    pwr = np.array([p for _, _, p in table])

    def delta(v):
        return np.array([(v[a - 1] if a else 0.0) - (v[b - 1] if b else 0.0) for a, b, _ in table])

    def gc():
        _, _, g = o.eval(xop, 0.0, 0.0, 0)
        _, _, g1 = o.eval(xop, 0.0, 1.0, 0)
        return g, g1 - g

    g0, c0 = gc()
    live = ~np.isnan(xb)                                         # rows the oracle solves (an eliminated branch current has none)
    ix = np.nonzero(live)[0]
    for k, nm in enumerate(AMP_SLOTS[:2]):
        p = base_value(c, ids[k])
        h = 1e-4 * abs(p)
        o.set_param(ids[k], p + h)
        gp, cp = gc()
        o.set_param(ids[k], p - h)
        gm, cm = gc()
        o.set_param(ids[k], p)
        dpw = np.array(NR.dpwr_analytic(c, c.slots[ids[k]]))
        got = []
        for f in AMP_FREQS:
            w = 2.0 * np.pi * f
            Y = (g0 + 1j * w * c0)[np.ix_(ix, ix)]
            dY = (((gp - gm) + 1j * w * (cp - cm)) / (2.0 * h))[np.ix_(ix, ix)]
            e = np.zeros(len(ix), dtype=complex)
            e[list(ix).index(out)] = 1.0
            y = np.linalg.solve(Y.T, e)
            z = np.linalg.solve(Y.T, -(dY.T @ y))
            yf, zf = np.zeros(c.n_mna, dtype=complex), np.zeros(c.n_mna, dtype=complex)
            yf[ix], zf[ix] = y, z
            dy, dz = delta(yf), delta(zf)
            got.append(float(np.sum(2.0 * np.real(np.conj(dy) * dz) * pwr + np.abs(dy) ** 2 * dpw)))
        miss = relative_errors(np.array(got), r[k], S)
        print("explicit terms alone, %s: %s" % (nm, " ".join("%.1e" % v for v in miss)))
        assert np.max(miss) > 100 * TOL, (nm, miss)


# ---- 4. the MOSFETs' own noise: the yardstick is the engine's ch_noise_ex ----
def engine_yardstick(E, c, ids, out, freqs, o):
    """(r, est, S) as oracle_yardstick, from ch_noise_ex with mos_noise on one engine circuit, ch_set_params between the calls.  This
    yardstick runs on the GPU."""
    e = E(c)

    def psd():
        rc, p, _, _ = e.noise_ex(0, c._n(out), freqs, o, mos_noise=True)
        assert rc == 0, e.ctx.last_error()
        return p[0].copy()
    S = psd()
    rs, est = [], []
    for s in ids:
        p = base_value(c, s)

        def at(v):
            e.set_params([s], [[v]])
            return psd()
        r, y2 = richardson(at, p)
        e.set_params([s], [[p]])
        rs.append(r), est.append(relative_errors(y2, r, S))
    return np.array(rs), np.array(est), S


def mos_case(E, c, names, out, freqs, what):
    ids = [slot_of(c, nm) for nm in names]
    o = dc_opts(abstol=1e-12)
    r, est, S = engine_yardstick(E, c, ids, out, freqs, o)
    for nm, v in zip(names, est):
        print("%s, yardstick's own estimates, %s: %s" % (what, nm, " ".join("%.1e" % x for x in v)))
    e = E(c)
    rc, psd, dpsd, _, _, _ = e.noise_sens(0, c._n(out), ids, freqs, o, mos_noise=True)
    assert rc == 0, e.ctx.last_error()
    assert np.allclose(psd[0], S, rtol=1e-9, atol=0.0)
    rcx, psd_x, _, _ = E(c).noise_ex(0, c._n(out), freqs, o, mos_noise=True)     # first call on a fresh engine circuit against the same
    assert rcx == 0 and np.array_equal(psd_x, psd)
    for k, nm in enumerate(names):
        print("%s, engine against the yardstick, %s: %s" % (what, nm, " ".join("%.1e" % x for x in relative_errors(dpsd[0][:, k], r[k], S))))
    return e, ids, r, est, S, dpsd[0]


FET_SLOTS = ["rd", ("m1", "w"), ("m1", "l"), ("nfet_06v0", "vth0"), "temp"]
FET_FREQS = np.array([10.0, 1e5, 1e8])      # flicker-dominated, white, past the output pole


def test_one_mosfet_with_its_own_noise(E):
    """one_fet of test_gpu_b4_noise.py with a load capacitor, output d, mos_noise = 1.  Every (slot, frequency) the yardstick admits
    is held to 1e-6; all must be admitted.  rd reaches the MOSFET's records through the bias alone: at 10 Hz the term
    |dy|^2 dpwr of the flicker entry must be more than 1e-3 of the result, which proves the state part of dpwr.
    Measured on the MI355X: the yardstick's estimates are at most 9.4e-10; errors rd 1.4e-9, m1.w 2.8e-9, m1.l 9.1e-10, vth0 2.8e-9,
    temp 1.0e-9; the share is 0.106."""
    c = one_fet(cl=1e-12)
    e, ids, r, est, S, got = mos_case(E, c, FET_SLOTS, "d", FET_FREQS, "one_fet")
    assert np.all(est <= ADMIT), est
    assert_close(got, r, S, FET_SLOTS, FET_FREQS, "one_fet at d", est <= ADMIT)
    # the share of the flicker entry's |dy|^2 dpwr in dS/d(rd) at 10 Hz: dpwr by a central difference of the table ch_noise_sources returns
    o = dc_opts(abstol=1e-12)
    p = base_value(c, ids[0])
    e2 = E(c)
    tab = {}
    for sign in (+1, -1):
        e2.set_params([ids[0]], [[p * (1.0 + sign * 1e-4)]])
        rc, _, contrib, _ = e2.noise_ex(0, c._n("d"), FET_FREQS[:1], o, mos_noise=True, contributions=True)
        assert rc == 0
        tab[sign] = e2.noise_sources(0, c._n("d"))
    e2.set_params([ids[0]], [[p]])
    rc, _, contrib, _ = e2.noise_ex(0, c._n("d"), FET_FREQS[:1], o, mos_noise=True, contributions=True)
    src = e2.noise_sources(0, c._n("d"))
    k = [j for j, d in enumerate(src["dev"]) if c.dev_names[d] == "m1"][1]          # the MOSFET's second column: flicker
    assert src["ex"][k] > 0.0 and src["pwr"][k] > 0.0
    dpwr = (tab[+1]["pwr"][k] - tab[-1]["pwr"][k]) / (2e-4 * p)
    share = abs(contrib[0][0][k] / src["pwr"][k] * dpwr / got[0][0])                 # contrib / pwr = |dy|^2 / f^ex
    print("one_fet: share of the flicker entry's |dy|^2 dpwr in dS/d(rd) at 10 Hz: %.3e" % share)
    assert share > 1e-3


def test_amplifier_with_mosfet_noise(E):
    """The amplifier at d with the MOSFETs' own sources.  Measured on the MI355X: estimates at most 1.0e-9; errors rd 2.3e-10,
    m1.w 1.1e-8, temp 3.4e-9."""
    names = ["rd", ("m1", "w"), "temp"]
    c = amp_circuit()
    e, ids, r, est, S, got = mos_case(E, c, names, "d", AMP_FREQS, "amplifier, mos_noise")
    assert np.all(est <= ADMIT), est
    assert_close(got, r, S, names, AMP_FREQS, "amplifier at d, mos_noise", est <= ADMIT)


def test_a_shared_class_moves_one_instance_only(E):
    """Two equal MOSFETs in parallel share a class; the slot ma.w gives one of them a column of its own (class n_cls), and the noise
    parameter table one more row.  A result that moved both instances, or read the table out of range, misses the yardstick.
    Measured on the MI355X: ma.w 2.6e-9, rd 1.4e-9."""
    c = Circuit(gmin=1e-12)
    mi = c.add_model(*card("nfet_06v0"))
    c.V("vdd", "vdd", 0, dc=5.0)
    c.V("vg", "g", 0, dc=1.6)
    c.R("rd", "vdd", "d", 10e3)
    c.M("ma", "d", "g", 0, 0, mi, 2e-6, 6e-7)
    c.M("mb", "d", "g", 0, 0, mi, 2e-6, 6e-7)
    c.C("cl", "d", 0, 1e-12)
    names = [("ma", "w"), "rd"]
    e, ids, r, est, S, got = mos_case(E, c, names, "d", FET_FREQS, "shared class")
    assert np.all(est <= ADMIT), est
    assert_close(got, r, S, names, FET_FREQS, "shared class at d", est <= ADMIT)


# ---- 5. compiled Verilog-A ----
def test_verilog_a_slots(E, O):
    """The diode's IS behind 1 kOhm (its shot noise moves explicitly and through the bias) and the noisy resistor's parameters,
    against Richardson differences of Oracle.noise.  Measured on the MI355X: IS 4.9e-7 (estimate 3.9e-9; the explicit and the state
    term cancel to 1/30 for this slot), r1 2.6e-8."""
    c = Circuit(gmin=1e-12)
    c.V("v1", "in", 0, dc=1.5)
    c.R("r1", "in", "a", 1e3)
    c.VA("d1", "va_diode", ["a", 0], {"IS": 1e-13, "RS": 2.0})
    c.C("c1", "a", 0, 1e-12)
    names = [("d1", "is"), "r1"]
    ids = [slot_of(c, nm) for nm in names]
    f = np.array([1e3, 1e8])
    r, est, S = oracle_yardstick(O, c, ids, c.mna_index("v", "a"), f)
    print("diode, yardstick's own estimates: " + ", ".join("%s %.1e" % (nm, v.max()) for nm, v in zip(names, est)))
    assert np.all(est <= ADMIT), est
    e = E(c)
    rc, psd, dpsd, _, _, _ = e.noise_sens(0, c._n("a"), ids, f, dc_opts(abstol=1e-12))
    assert rc == 0, e.ctx.last_error()
    assert_close(dpsd[0], r, S, names, f, "diode behind 1 kOhm", est <= ADMIT)


def noisy_resistor():
    """The current-biased noisy resistor of test_gpu_ac_noise.py: white and flicker noise, the flicker exponent a parameter."""
    c = Circuit()
    c.temp = 50.0
    c.I("ib", 0, "a", dc=1e-3)
    c.VA("r1", "va_noisy_resistor", ["a", 0], {"R": 2e3, "KF": 1e-10, "AF": 2.0, "EF": 1.2}, m=2.0)
    c.C("c1", "a", 0, 1e-9)
    return c


def test_verilog_a_noisy_resistor(E, O):
    """White and flicker noise of a compiled module: R, KF, the bias current and the temperature.  Measured on the MI355X: at most
    4.9e-11 (estimates at most 3.3e-11)."""
    c = noisy_resistor()
    names = [("r1", "r"), ("r1", "kf"), "ib", "temp"]
    ids = [slot_of(c, nm) for nm in names]
    f = np.array([10.0, 1e4, 1e6])
    r, est, S = oracle_yardstick(O, c, ids, c.mna_index("v", "a"), f)
    print("noisy resistor, yardstick's own estimates: " + ", ".join("%s %.1e" % (nm, v.max()) for nm, v in zip(names, est)))
    assert np.all(est <= ADMIT), est
    e = E(c)
    rc, psd, dpsd, _, _, _ = e.noise_sens(0, c._n("a"), ids, f, dc_opts(abstol=1e-12))
    assert rc == 0, e.ctx.last_error()
    assert_close(dpsd[0], r, S, names, f, "noisy resistor", est <= ADMIT)


def test_a_slot_that_moves_a_flicker_exponent_is_refused(E):
    """EF of the noisy resistor is the exponent of its flicker source: ch_noise_sens does not differentiate f^-ex in ex and says so,
    naming the slot; the other slots of the same call's circuit are served when EF is not among them."""
    c = noisy_resistor()
    ef, kf = slot_of(c, ("r1", "ef")), slot_of(c, ("r1", "kf"))
    e = E(c)
    f = np.array([10.0, 1e4])
    rc = e.noise_sens(0, c._n("a"), [kf, ef], f, dc_opts(abstol=1e-12))[0]
    assert rc == ERR_UNSUPPORTED and ("slot %d " % ef) in e.ctx.last_error() and "exponent" in e.ctx.last_error()
    rc, psd, dpsd, _, _, _ = e.noise_sens(0, c._n("a"), [kf], f, dc_opts(abstol=1e-12))
    assert rc == 0 and np.all(dpsd > 0)
    with pytest.raises(CedarError):
        noise_sens(c, [("r1", "ef")], abstol=1e-12).sens("a", ("r1", "ef"), 2 * math.pi * f)


# ---- 6. refusals and failures ----
def rc_cell(r=1.3e3, cap=2.2e-9):
    c = Circuit()
    c.V("vin", "a", 0, dc=0.0, ac=1.0)
    c.R("r1", "a", "b", r)
    c.C("c1", "b", 0, cap)
    return c


def test_errors_are_return_codes(E):
    c = rc_cell()
    ids = [c.slot("r1")]
    e = E(c)
    o = opts(c)
    f = np.array([1e3])
    b = c._n("b")
    for bad in ([7], [-1], [ids[0], 99]):
        rc = e.noise_sens(0, b, bad, f, o)[0]
        assert rc == -1 and "slot" in e.ctx.last_error()
    for bad_f in ([-1.0], [1e3, math.nan], [math.inf]):
        rc = e.noise_sens(0, b, ids, np.array(bad_f), o)[0]
        assert rc == -1 and "frequenc" in e.ctx.last_error()
    assert e.noise_sens(0, 99, ids, f, o)[0] == -1 and e.noise_sens(2, b, ids, f, o)[0] == -1
    i32 = (C.c_int32 * 1)(ids[0])
    ff = (C.c_double * 1)(1e3)
    psd, dpsd = (C.c_double * 1)(), (C.c_double * 1)()
    call = e.L.ch_noise_sens
    assert call(e.h, o, None, 0, i32, None, 0, b, 1, ff, psd, dpsd, None, None, None) == -1       # n_par = 0
    assert call(e.h, o, None, 1, i32, None, 0, b, 1, ff, psd, None, None, None, None) == -1       # no dpsd_out
    assert call(e.h, o, None, 1, i32, None, 0, b, 1, ff, None, dpsd, None, None, None) == -1      # no psd_out
    assert call(e.h, o, None, 1, i32, None, 0, b, 0, ff, psd, dpsd, None, None, None) == -1       # no frequency
    assert call(e.h, o, None, 1, i32, None, 0, b, 1, ff, psd, dpsd, None, None, None) == 0        # the options and optional outputs may be NULL
    x = 2.0 * math.pi * 1e3 * 1.3e3 * 2.2e-9
    kt4 = 4.0 * 1.380649e-23 * (c.temp + 273.15)
    assert psd[0] == pytest.approx(kt4 * 1.3e3 / (1 + x * x), rel=1e-12) and dpsd[0] == pytest.approx(kt4 * (1 - x * x) / (1 + x * x) ** 2, rel=1e-9)
    with pytest.raises(CedarError):
        noise_sens(c, ["nosuchdevice"])


def test_holistic_thermal_noise_is_refused_only_with_mosfet_noise(E):
    c = one_fet(tnoimod=1)
    ids = [slot_of(c, "rd")]
    e = E(c)
    rc = e.noise_sens(0, c._n("d"), ids, FET_FREQS, dc_opts(abstol=1e-12), mos_noise=True)[0]
    assert rc == ERR_UNSUPPORTED and "model card 0" in e.ctx.last_error()
    rc, psd, dpsd, _, _, _ = e.noise_sens(0, c._n("d"), ids, FET_FREQS, dc_opts(abstol=1e-12), mos_noise=False)
    assert rc == 0 and np.all(psd > 0) and not np.isnan(dpsd).any()
    with pytest.raises(CedarError) as ex:
        noise_sens(c, ["rd"], device_noise=True, abstol=1e-12).sens("node_d", "rd", 2 * math.pi * FET_FREQS)
    assert "tnoimod = 1" in str(ex.value) and "nfet_06v0" in str(ex.value)


def test_a_failed_sample_is_reported_and_the_others_are_served(E):
    """Sample 1 has no operating point (an infinite resistor leaves a current source on a node nothing else holds): NaN rows and
    its ch_dc status; sample 0 has the bits of a one-sample call."""
    c = rc_cell()
    c.I("i1", "n", 0, dc=1e-3)
    c.R("rn", "n", 0, 1e3)
    names = ["rn", "r1", "c1"]
    ids = [slot_of(c, nm) for nm in names]
    f = np.array([0.0, 1e5])
    o = dict(abstol=1e-12, n_restarts=2, maxiters=5)
    b = c._n("b")
    e = E(c)
    e.set_samples(2)
    e.set_params(ids[:1], [[1e3, math.inf]])
    rc, psd, dpsd, ds, status, _ = e.noise_sens(0, b, ids, f, dc_opts(**o))
    assert rc == -3 and status[0] == 0 and status[1] != 0
    assert np.isnan(psd[1]).all() and np.isnan(dpsd[1]).all() and not np.isnan(psd[0]).any() and not np.isnan(dpsd[0]).any()
    rc1, psd1, dpsd1, _, _, _ = E(c).noise_sens(0, b, ids, f, dc_opts(**o))
    assert rc1 == 0 and np.array_equal(dpsd1[0], dpsd[0]) and np.array_equal(psd1[0], psd[0])
    # an output held by a source (here: ground) carries no noise in the sample that is served; the other one is still not served
    rcg, psd_g, dpsd_g, ds_g, status_g, _ = e.noise_sens(0, 0, ids, f, dc_opts(**o))
    assert rcg == -3 and status_g[0] == 0 and status_g[1] != 0
    assert not psd_g[0].any() and not dpsd_g[0].any() and np.isnan(psd_g[1]).all() and np.isnan(dpsd_g[1]).all()
    assert np.isnan(ds_g[1][:, b]).all() and not np.isnan(ds_g[0][:, b]).any()
    x = 2.0 * math.pi * 1e5 * 1.3e3 * 2.2e-9
    kt4 = 4.0 * 1.380649e-23 * (c.temp + 273.15)
    assert dpsd[0][1][1] == pytest.approx(kt4 * (1 - x * x) / (1 + x * x) ** 2, rel=1e-8) and dpsd[0][1][0] == 0.0


# ---- 7. the Python surface ----
def test_circuit_sweep_and_the_solution_object(E):
    """noise_sens(CircuitSweep) over three points: each point has the closed forms of the RC cell — S = 4kTR/(1+x^2),
    dS/dR = 4kT(1-x^2)/(1+x^2)^2, dS/dC = -8kTR x^2/(C(1+x^2)^2), dS/dT = S/T — and equals its own single call; log_sens and the band
    integrals follow from them."""
    cap, t = 2.2e-9, rc_cell().temp + 273.15
    rs = [500.0, 1.3e3, 2e4]
    cs = CircuitSweep(lambda r1=1e3: rc_cell(r1, cap), Sweep(r1=rs))
    names = ["r1", "c1", "temp"]
    sols = noise_sens(cs, names, abstol=1e-12)
    assert len(sols) == 3
    w = 2.0 * np.pi * np.array([1e3, 5e4, 2e6])
    kt4 = 4.0 * 1.380649e-23 * t
    for sol, p in zip(sols, cs):
        r1 = p["r1"]
        x = w * r1 * cap
        S = kt4 * r1 / (1 + x * x)
        want = {"r1": kt4 * (1 - x * x) / (1 + x * x) ** 2, "c1": -2 * kt4 * r1 * x * x / (cap * (1 + x * x) ** 2), "temp": S / t}
        assert np.allclose(sol.psd("b", w), S, rtol=1e-12, atol=0.0)
        for nm in names:
            assert np.allclose(sol.sens("b", nm, w), want[nm], rtol=1e-8, atol=1e-9 * np.max(np.abs(want[nm]))), nm
        assert np.allclose(sol.log_sens("b", "r1", w), r1 * want["r1"] / S, rtol=1e-8, atol=1e-9)
        f = w / (2.0 * np.pi)
        assert sol.integrated("b", w) == pytest.approx(float(np.sum(0.5 * (S[1:] + S[:-1]) * np.diff(f))), rel=1e-12)
        dr = sol.sens("b", "r1", w)
        assert sol.integrated_sens("b", "r1", w) == pytest.approx(float(np.sum(0.5 * (dr[1:] + dr[:-1]) * np.diff(f))), rel=1e-12)
        assert sol.integrated_sens("b", "temp", w[:1]) == pytest.approx(S[0] / t, rel=1e-9)
        assert sol.op.params == p and sol.op.rc == 0 and sol.dc_sens.rc == 0
        one = noise_sens(rc_cell(r1, cap), names, abstol=1e-12)
        assert np.allclose(one.sens("b", "r1", w), dr, rtol=1e-12, atol=0.0)
    with pytest.raises(KeyError):
        sols[0].sens("b", "vin", w)
    assert len(cs.noise_sens(["r1"], abstol=1e-12)) == 3
