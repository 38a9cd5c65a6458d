"""GPU tests of the DC parameter sensitivities (ch_dc_sens, direct method): closed forms on linear circuits, and on nonlinear
circuits a yardstick computed with the CPU oracle alone — central differences of full oracle operating points at relative steps
1e-3 and 5e-4, Richardson-extrapolated.  Tolerance against the yardstick: 1e-6 of max|d x / d p_k| over the MNA rows, the
project's DC parity contract."""
import math

import numpy as np
import pytest

from cedarsim_jl_amd import Circuit, CircuitSweep, PULSE, Sweep, dc_opts, dc_sens, tran_opts
from cedarsim_jl_amd.circuit import (CedarError, SLOT_DEV_MULT, SLOT_DEV_PAR, SLOT_GMIN, SLOT_MODEL_PAR, SLOT_SRC_DC, SLOT_SRC_PAR,
                                     SLOT_TEMP, SLOT_VA_PAR)
from cedarsim_jl_amd.workloads import gf180_models

from test_gpu_ac_noise import amp_circuit

pytestmark = pytest.mark.gpu
ENG = dc_opts(abstol=1e-12)


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def O(oracle_lib):
    from oracle_binding import Oracle
    return Oracle


def base_value(c, slot):
    k, a, b = c.slots[slot]
    return {SLOT_DEV_PAR: lambda: c.dev_par[a][b], SLOT_DEV_MULT: lambda: c.dev_mult[a], SLOT_MODEL_PAR: lambda: c.models[a][b],
            SLOT_SRC_DC: lambda: c.sources[a][0], SLOT_SRC_PAR: lambda: c.sources[a][1].par[b], SLOT_TEMP: lambda: c.temp,
            SLOT_GMIN: lambda: c.gmin, SLOT_VA_PAR: lambda: c.va_par[a]}[k]()


def yardstick(O, c, slots, point=None):
    """d x_mna / d p for every slot in `slots`, from the oracle only: central differences of Oracle.dc(abstol=1e-14) at relative
    steps 1e-3 and 5e-4 through Oracle.set_param, Richardson-extrapolated r = (4*y2 - y1)/3.  `point`: {slot: value} applied first.
    Returns (r[n_slots][n_mna], y2[n_slots][n_mna], x[n_mna])."""
    o = O(c)
    at = {s: base_value(c, s) for s in slots}
    for s, v in (point or {}).items():
        o.set_param(s, v)
        at[s] = v
    rc, xb, _ = o.dc(dc_opts(abstol=1e-14))
    assert rc == 0

    def solve():
        rc, x, _ = o.dc(dc_opts(abstol=1e-14, x0=xb))
        assert rc == 0
        return x

    r, y2 = [], []
    for s in slots:
        p = at[s]
        assert math.isfinite(p) and p != 0.0
        y = []
        for rel in (1e-3, 5e-4):
            h = rel * abs(p)
            o.set_param(s, p + h)
            xp = solve()
            o.set_param(s, p - h)
            xm = solve()
            y.append((xp - xm) / (2.0 * h))
        o.set_param(s, p)
        r.append((4.0 * y[1] - y[0]) / 3.0)
        y2.append(y[1])
    return np.array(r), np.array(y2), xb


def assert_close(s, r, tol=1e-6, what=""):
    """|s - r| <= tol * max|r| over the MNA rows the engine reports (an eliminated branch current is NaN on the engine's side)."""
    ok = ~np.isnan(s)
    assert ok.any()
    scale = np.max(np.abs(r[ok]))
    err = np.max(np.abs(s[ok] - r[ok]))
    print("%s: max|s - r| / max|r| = %.3e (max|r| = %.3e)" % (what, err / scale if scale else err, scale))
    assert err <= tol * scale, (what, err, scale)


# ---- circuits ----
def divider(observe_branch=True):
    c = Circuit()
    c.V("v", "vcc", 0, dc=1.0)
    c.R("r1", "vcc", "out", 1e3)
    c.R("r2", "out", "n2", 1e3)
    c.L("l1", "n2", 0, 1e-6)
    c.C("c1", "out", 0, 1e-9)
    if observe_branch:
        c.observe_branch("v")
    return c


AMP_SLOTS = ["vdd", "rd", ("rb1", "m"), ("m1", "w"), ("m1", "l"), ("nfet_06v0", "vth0"), ("nfet_06v0", "u0"), ("pfet_06v0", "toxe"), "temp", "iinj"]


def slot_of(c, name):
    return c.slot(*name) if isinstance(name, tuple) else c.slot(name)


@pytest.fixture(scope="module")
def amp(O):
    """The amplifier with its slots declared, and the yardstick at its base point — computed once, shared, never modified."""
    c = amp_circuit()
    ids = [slot_of(c, n) for n in AMP_SLOTS]
    r, y2, xb = yardstick(O, c, ids)
    r.setflags(write=False)
    xb.setflags(write=False)
    return c, ids, r, xb


def ladder(n):
    """Resistor ladder: n sections of series r (about 1 kOhm) and shunt r (about 2 kOhm) to ground, driven by 1 V, every value distinct."""
    c = Circuit()
    c.V("v", "n0", 0, dc=1.0)
    rs = [1e3 * (1.0 + 0.01 * ((7 * i) % 13) + 1e-4 * i) for i in range(1, n + 1)]
    rp = [2e3 * (1.0 + 0.01 * ((5 * i) % 11) + 1e-4 * i) for i in range(1, n + 1)]
    for i in range(1, n + 1):
        c.R("rs%d" % i, "n%d" % (i - 1), "n%d" % i, rs[i - 1])
        c.R("rp%d" % i, "n%d" % i, 0, rp[i - 1])
    return c, rs, rp


def LADDER_ENG(c):
    """abstol 1e-12 and a zero initial guess.  The node voltages of a ladder halve from section to section, and a derivative with
    respect to a resistor halfway down is proportional to the voltages THERE (1e-15 V at section 50).  A linear circuit is solved by
    one Newton step x0 + dx; from the default start x0 = 1e-7*randn the cancellation in that sum leaves an absolute error of about
    1e-7 * 2^-53 = 1e-23 V in every node — far inside abstol, but 1e-8 of those voltages, and the same 1e-8 of the derivative.
    From x0 = 0 the step is the solution itself, relatively accurate in every row."""
    return dc_opts(abstol=1e-12, x0=np.zeros((1, c.n_mna)))


def ladder_reference(n, rs, rp, names):
    """numpy: G x = b for the nodes n1..nn, then s_k = -G^-1 (dF/dr_k) with F = G x - b."""
    G = np.zeros((n, n))
    b = np.zeros(n)
    for i in range(n):
        g = 1.0 / rs[i]
        G[i, i] += g + 1.0 / rp[i]
        if i > 0:
            G[i - 1, i - 1] += g
            G[i, i - 1] -= g
            G[i - 1, i] -= g
        else:
            b[0] = g * 1.0
    x = np.linalg.solve(G, b)
    v = np.concatenate(([1.0], x))   # v[i] = node n_i
    out = []
    for nm in names:
        dF = np.zeros(n)
        if nm == "v":
            dF[0] = -1.0 / rs[0]
        elif nm.startswith("rs"):
            i = int(nm[2:])
            d = -(v[i - 1] - v[i]) / rs[i - 1] ** 2    # d/dr of the current (v[i-1] - v[i])/r leaving node i-1, entering node i
            if i - 1 >= 1:
                dF[i - 2] += d
            dF[i - 1] -= d
        else:
            i = int(nm[2:])
            dF[i - 1] = -v[i] / rp[i - 1] ** 2
        out.append(np.linalg.solve(G, -dF))
    return x, np.array(out)


def inverter_blocks():
    """Two structurally identical, unconnected inverters with separate supplies (each behind a supply resistor) and one divider."""
    c = Circuit()
    m = gf180_models()
    n = c.add_model(*m["nfet_06v0"])
    p = c.add_model(*m["pfet_06v0"])
    for k, vin in ((1, 2.0), (2, 2.6)):
        c.V("vdd%d" % k, "vdd%d" % k, 0, dc=5.0)
        c.V("vin%d" % k, "in%d" % k, 0, dc=vin)
        c.R("rsup%d" % k, "vdd%d" % k, "vp%d" % k, 500.0)
        c.M("mp%d" % k, "o%d" % k, "in%d" % k, "vp%d" % k, "vp%d" % k, p, 4e-6, 5e-7)
        c.M("mn%d" % k, "o%d" % k, "in%d" % k, 0, 0, n, 2e-6, 6e-7)
        c.R("rl%d" % k, "o%d" % k, 0, 100e3)
    c.V("v", "vcc", 0, dc=1.0)
    c.R("r1", "vcc", "out", 1e3)
    c.R("r2", "out", 0, 1e3)
    return c


# ---- 1. closed form, linear ----
def test_divider_closed_forms(E):
    c = divider()
    names = ["r1", "r2", "v", ("r1", "m"), "c1", "l1"]
    ids = [slot_of(c, n) for n in names]
    rc, x, s, status, st = E(c).dc_sens(ids, ENG)
    assert rc == 0 and status[0] == 0
    s = s[0]
    out, vcc, iv = c.mna_index("v", "out"), c.mna_index("v", "vcc"), c.mna_index("i", "v")
    V, R1, R2 = 1.0, 1e3, 1e3
    assert s[0][out] == pytest.approx(-V * R2 / (R1 + R2) ** 2, rel=1e-9)
    assert s[1][out] == pytest.approx(+V * R1 / (R1 + R2) ** 2, rel=1e-9)
    assert s[0][out] == pytest.approx(-s[1][out], rel=1e-9)            # dR1 ≈ -dR2 at R1 = R2 (test/sensitivity.jl:40)
    assert s[0][iv] == pytest.approx(+V / (R1 + R2) ** 2, rel=1e-9)    # branch current flows from net+ to net- through the source
    assert s[2][out] == pytest.approx(R2 / (R1 + R2), rel=1e-12)
    assert s[2][vcc] == pytest.approx(1.0, rel=1e-12)
    assert s[3][out] == pytest.approx(V * R1 * R2 / (R1 + R2) ** 2, rel=1e-12)   # R_eff = R1/m at m = 1
    assert np.all(s[4] == 0.0) and np.all(s[5] == 0.0)                 # C and L values do not enter a DC residual
    assert x[0][out] == pytest.approx(0.5, rel=1e-12)
    # the supply node eliminated as a known node: its row is the derivative of its known-value expression
    c = divider(observe_branch=False)
    ids = [slot_of(c, n) for n in names]
    rc, x, s, status, st = E(c).dc_sens(ids, ENG)
    assert rc == 0
    s = s[0]
    assert E(c).maps()[1][c._n("vcc")] >= 0                            # vcc is a known node here
    assert s[2][vcc] == 1.0 and all(s[k][vcc] == 0.0 for k in (0, 1, 3, 4, 5))
    assert np.isnan(s[:, iv]).all()                                    # the eliminated branch current
    assert s[0][out] == pytest.approx(-V * R2 / (R1 + R2) ** 2, rel=1e-9) and s[2][out] == pytest.approx(0.5, rel=1e-12)
    # the user-facing form
    sol = dc_sens(divider(observe_branch=False), ["r1", "r2", "v", ("r1", "m")], abstol=1e-12)
    assert sol["node_out", "r1"] == pytest.approx(-0.25e-3, rel=1e-9) and sol["out", "r2"] == pytest.approx(0.25e-3, rel=1e-9)
    assert sol["v.i", "r1"] == pytest.approx(0.25e-6, rel=1e-9) and sol["r1.v", "v"] == pytest.approx(0.5, rel=1e-12)
    assert sol["out", ("r1", "m")] == pytest.approx(0.25, rel=1e-12)
    assert sol.op["node_out"][0] == pytest.approx(0.5, rel=1e-12) and sol.retcode == "Success"
    with pytest.raises(KeyError):
        sol["out", "c1"]


# ---- 2. nonlinear, against the yardstick ----
def test_amplifier_matches_oracle_yardstick(E, amp):
    c, ids, r, xb = amp
    rc, x, s, status, st = E(c).dc_sens(ids, ENG)
    assert rc == 0
    ok = ~np.isnan(x[0])
    assert np.allclose(x[0][ok], xb[ok], rtol=1e-6, atol=1e-9)
    for k, name in enumerate(AMP_SLOTS):
        assert_close(s[0][k], r[k], what=str(name))
    assert np.max(np.abs(s[0][AMP_SLOTS.index("rd")][ok])) > 0.0


def test_amplifier_gmin_slot(E, O):
    """gmin differentiated at 1e-9 S, where the yardstick's own steps (1e-12, 5e-13 S) are resolvable.  The yardstick, not the
    feature, limits this comparison: its own error estimate e = max|y2 - r| / max|r| is measured here and the tolerance is
    max(1e-6, 10 e)."""
    c = amp_circuit()
    c.gmin = 1e-9
    g = c.slot("gmin")
    r, y2, xb = yardstick(O, c, [g])
    e = np.max(np.abs(y2[0] - r[0])) / np.max(np.abs(r[0]))
    print("gmin yardstick: e = %.3e, max|r| = %.3e" % (e, np.max(np.abs(r[0]))))
    rc, x, s, status, st = E(c).dc_sens([g], ENG)
    assert rc == 0
    assert_close(s[0][0], r[0], tol=max(1e-6, 10.0 * e), what="gmin")


# ---- 3. class sharing ----
def test_instance_slot_on_a_shared_mos_class(E, O):
    """Two identical NMOS share one column of the packed BSIM4 table; a declared-but-unset W slot on one of them must move that
    instance alone, a model-card slot both."""
    c = Circuit()
    n = c.add_model(*gf180_models()["nfet_06v0"])
    c.V("vdd", "vdd", 0, dc=5.0)
    c.V("vg", "g", 0, dc=1.3)
    c.R("rsup", "vdd", "vs", 1e3)
    c.R("ra", "vs", "da", 20e3)
    c.R("rb", "vs", "db", 10e3)
    c.M("ma", "da", "g", 0, 0, n, 2e-6, 6e-7)
    c.M("mb", "db", "g", 0, 0, n, 2e-6, 6e-7)
    ids = [c.slot("ma", "w"), c.slot("nfet_06v0", "vth0")]
    r, _, xb = yardstick(O, c, ids)
    e = E(c)
    rc, x, s, status, st = e.dc_sens(ids, ENG)
    assert rc == 0 and e.info()["n_mos"] == 2 and e.info()["n_mos_classes"] == 1
    assert_close(s[0][0], r[0], what="ma.w")
    assert_close(s[0][1], r[1], what="vth0")
    da, db = c.mna_index("v", "da"), c.mna_index("v", "db")
    assert s[0][0][da] != 0.0 and abs(s[0][0][da]) > 5.0 * abs(s[0][0][db])
    # mb moves only through the shared supply resistor: small, not zero — and not what perturbing both instances would give
    assert r[0][db] != 0.0 and abs(s[0][0][db] - r[0][db]) <= 1e-6 * np.max(np.abs(r[0]))


# ---- 4. batch with per-sample values ----
def test_batch_of_three_samples_each_at_its_own_point(E, O, amp):
    c, _, _, xb = amp
    names = ["rd", ("m1", "w"), "vdd", ("nfet_06v0", "vth0")]
    ids = [slot_of(c, n) for n in names]
    rd, w = [18e3, 20e3, 25e3], [1.8e-6, 2e-6, 2.4e-6]
    x0 = np.nan_to_num(np.tile(xb, (3, 1)))
    e3 = E(c)
    e3.set_samples(3)
    e3.set_params(ids[:2], [rd, w])
    rc, x, s, status, st = e3.dc_sens(ids, dc_opts(abstol=1e-12, x0=x0))
    assert rc == 0 and s.shape == (3, 4, c.n_mna)
    for k in range(3):
        r, _, _ = yardstick(O, c, ids, point={ids[0]: rd[k], ids[1]: w[k]})
        for j, name in enumerate(names):
            assert_close(s[k][j], r[j], what="sample %d %s" % (k, name))
    assert not np.array_equal(s[0], s[1]) and not np.array_equal(s[1], s[2])
    # sample 1 sits at the base point: the same bits as a single-sample call there
    e1 = E(c)
    rc, x1, s1, status, st = e1.dc_sens(ids, dc_opts(abstol=1e-12, x0=x0[:1]))
    assert rc == 0
    assert np.array_equal(x1[0], x[1], equal_nan=True) and np.array_equal(s1[0], s[1], equal_nan=True)


# ---- 5. several blocks ----
def test_independent_blocks_do_not_see_each_other(E, O):
    c = inverter_blocks()
    names = [("mn1", "w"), "vdd2", "r1", ("pfet_06v0", "vth0")]
    ids = [slot_of(c, n) for n in names]
    e = E(c)
    rc, x, s, status, st = e.dc_sens(ids, ENG)
    info = e.info()
    assert rc == 0 and info["n_components"] == 3 and info["n_classes"] == 2 and info["path"] == 1
    s = s[0]
    blk = {1: [c.mna_index("v", n) for n in ("o1", "vp1")], 2: [c.mna_index("v", n) for n in ("o2", "vp2")], 3: [c.mna_index("v", "out")]}
    assert np.all(s[0][blk[2] + blk[3]] == 0.0) and np.all(s[0][blk[1]] != 0.0)
    assert np.all(s[1][blk[1] + blk[3]] == 0.0) and np.all(s[1][blk[2]] != 0.0)
    assert np.all(s[2][blk[1] + blk[2]] == 0.0)
    assert s[2][blk[3][0]] == pytest.approx(-0.25e-3, rel=1e-9)
    assert np.all(s[3][blk[3]] == 0.0) and np.all(s[3][blk[1] + blk[2]] != 0.0)
    r, _, _ = yardstick(O, c, [ids[0], ids[1], ids[3]])
    for j, k in enumerate((0, 1, 3)):
        assert_close(s[k], r[j], what=str(names[k]))


# ---- 6. sparse path ----
def test_amplifier_on_the_sparse_path(E, amp, monkeypatch):
    c, ids, r, xb = amp
    monkeypatch.setenv("CEDARHIP_FORCE_SPARSE", "1")
    try:
        e = E(c)
        rc, x, s, status, st = e.dc_sens(ids, ENG)
        path = e.info()["path"]
    finally:
        monkeypatch.delenv("CEDARHIP_FORCE_SPARSE", raising=False)
    assert rc == 0 and path == 2
    for k, name in enumerate(AMP_SLOTS):
        assert_close(s[0][k], r[k], what="sparse " + str(name))


# ---- 7. above 96 unknowns: the global-workspace variant of the solve kernel ----
def test_ladder_of_100_sections(E):
    n = 100
    c, rs, rp = ladder(n)
    names = ["v", "rs1", "rs50", "rs100", "rp1", "rp50", "rp100"]
    ids = [c.slot(nm) for nm in names]
    e = E(c)
    rc, x, s, status, st = e.dc_sens(ids, LADDER_ENG(c))
    info = e.info()
    assert rc == 0 and info["n_unknowns"] == n and info["path"] == 2
    xr, sr = ladder_reference(n, rs, rp, names)
    rows = [c.mna_index("v", "n%d" % i) for i in range(1, n + 1)]
    assert np.allclose(x[0][rows], xr, rtol=1e-9, atol=1e-9)   # abstol 1e-12 A into about 1 kOhm
    for k, nm in enumerate(names):
        assert np.allclose(s[0][k][rows], sr[k], rtol=1e-8, atol=1e-8 * np.max(np.abs(sr[k]))), nm
    assert s[0][0][c.mna_index("v", "n0")] == 1.0


# ---- 8. right-hand-side chunking ----
def test_more_parameters_than_one_lds_chunk(E):
    """80 sections: one dense block of nc = 80 unknowns per sample (sparse path, LDS variant of the solve kernel).  Beside the
    80 x 80 matrix the LDS budget of 2*96*97 doubles holds Kc = 18624/80 - 81 = 151 right-hand sides; all 160 resistors are
    requested (n_par = 160), so the call takes two chunks (151 + 9) and must give the bits of two separate calls of 80."""
    n = 80
    c, rs, rp = ladder(n)
    names = ["rs%d" % i for i in range(1, n + 1)] + ["rp%d" % i for i in range(1, n + 1)]
    ids = [c.slot(nm) for nm in names]
    e = E(c)
    rc, x, s, status, st = e.dc_sens(ids, LADDER_ENG(c))
    info = e.info()
    assert rc == 0 and info["n_unknowns"] == n and info["path"] == 2 and len(ids) == 160
    xr, sr = ladder_reference(n, rs, rp, names)
    rows = [c.mna_index("v", "n%d" % i) for i in range(1, n + 1)]
    for k, nm in enumerate(names):
        assert np.allclose(s[0][k][rows], sr[k], rtol=1e-8, atol=1e-8 * np.max(np.abs(sr[k]))), nm
    rc_a, _, sa, _, _ = e.dc_sens(ids[:80], LADDER_ENG(c))
    rc_b, _, sb, _, _ = e.dc_sens(ids[80:], LADDER_ENG(c))
    assert rc_a == 0 and rc_b == 0
    assert np.array_equal(s[0][:80], sa[0], equal_nan=True) and np.array_equal(s[0][80:], sb[0], equal_nan=True)


# ---- 9. compiled Verilog-A ----
def test_verilog_a_parameter_slots(E, O):
    c = Circuit()
    c.V("v", "in", 0, dc=1.0)
    c.VA("rs", "va_resistor", ["in", "out"], {"R": 1e3})
    c.R("r2", "out", 0, 1e3)
    ids = [c.slot("rs", "r"), c.slot("r2"), c.slot("gmin")]
    rc, x, s, status, st = E(c).dc_sens(ids, ENG)
    assert rc == 0
    out = c.mna_index("v", "out")
    assert s[0][0][out] == pytest.approx(-0.25e-3, rel=1e-9) and s[0][1][out] == pytest.approx(+0.25e-3, rel=1e-9)
    assert s[0][2][out] == 0.0      # no device of this circuit reads gmin (central relative rule: a compiled instance is present)
    # a diode behind a resistor, slot on the saturation current: against the yardstick (the oracle's set_param serves CH_SLOT_VA_PAR)
    c = Circuit(gmin=1e-12)
    c.V("v1", "in", 0, dc=1.5)
    c.R("r1", "in", "a", 1e3)
    c.VA("d1", "va_diode", ["a", 0], {"IS": 1e-13, "RS": 2.0})
    ids = [c.slot("d1", "is"), c.slot("r1"), c.slot("temp")]
    r, _, xb = yardstick(O, c, ids)
    rc, x, s, status, st = E(c).dc_sens(ids, ENG)
    assert rc == 0
    for k, nm in enumerate(("d1.is", "r1", "temp")):
        assert_close(s[0][k], r[k], what=nm)
    assert s[0][0][c.mna_index("v", "a")] < 0.0


# ---- 10. nothing moved ----
def test_the_circuit_is_left_as_it_was(E):
    def build():
        c = Circuit(gmin=1e-12)
        m = gf180_models()
        n = c.add_model(*m["nfet_06v0"])
        p = c.add_model(*m["pfet_06v0"])
        c.V("vdd", "vdd", 0, dc=5.0)
        c.V("vin", "in", 0, dc=0.0, tran=PULSE(0.0, 5.0, 2e-9, 1e-9, 1e-9, 8e-9, 40e-9))
        c.R("rsup", "vdd", "vp", 200.0, m=2.0)
        c.M("mp", "o", "in", "vp", "vp", p, 4e-6, 5e-7)
        c.M("mn", "o", "in", 0, 0, n, 2e-6, 6e-7)
        c.M("mn2", "o2", "o", 0, 0, n, 2e-6, 6e-7)
        c.R("rl2", "vp", "o2", 50e3)
        c.C("cl", "o", 0, 5e-14)
        c.C("cl2", "o2", 0, 5e-14)
        c.observe_node("o")
        c.observe_node("o2")
        names = ["vdd", "rsup", ("rsup", "m"), ("mn", "w"), ("nfet_06v0", "vth0"), "temp", "gmin", "cl", ("vin", 1)]
        return c, [slot_of(c, nm) for nm in names]

    c, ids = build()
    e = E(c)
    rc0, x0, _, _ = e.dc(ENG)
    rc1, xs, s, status, st = e.dc_sens(ids, ENG)
    rc2, x2, _, _ = e.dc(ENG)
    assert rc0 == 0 and rc1 == 0 and rc2 == 0
    assert np.array_equal(x0, x2, equal_nan=True) and np.array_equal(x0, xs, equal_nan=True)
    assert np.all(np.isfinite(s[0][:, c.mna_index("v", "o2")])) and np.any(s[0] != 0.0)
    opts = dict(abstol=1e-8, reltol=1e-6, saveat=np.linspace(0.0, 2e-8, 21))
    rc_a, t_a, v_a, xf_a, _ = e.tran(0.0, 2e-8, tran_opts(dc=dc_opts(abstol=1e-12), **opts))
    c2, _ = build()
    rc_b, t_b, v_b, xf_b, _ = E(c2).tran(0.0, 2e-8, tran_opts(dc=dc_opts(abstol=1e-12), **opts))
    assert rc_a == 0 and rc_b == 0 and len(t_a) == 21
    assert np.array_equal(t_a, t_b) and np.array_equal(v_a, v_b) and np.array_equal(xf_a, xf_b, equal_nan=True)


# ---- 11. errors ----
def test_errors_are_return_codes(E):
    c = divider(observe_branch=False)
    ids = [c.slot("r1")]
    e = E(c)
    for bad in ([7], [-1], [ids[0], 99]):
        rc, x, s, status, st = e.dc_sens(bad, ENG)
        assert rc == -1 and "slot" in e.ctx.last_error()
    rc = e.L.ch_dc_sens(e.h, ENG, 0, None, None, None, None, None, None)
    assert rc == -1
    # a node that hangs on a capacitor alone: its KCL row holds at any voltage (the operating point "converges"), its row of G is zero
    c = divider(observe_branch=False)
    c.C("cf", "f", 0, 1e-9)
    ids = [c.slot("r1")]
    e = E(c)
    rc, x, s, status, st = e.dc_sens(ids, ENG)
    assert rc == -2 and "singular" in e.ctx.last_error()
    assert np.isnan(s[0][0][c.mna_index("v", "f")])
    assert s[0][0][c.mna_index("v", "out")] == pytest.approx(-0.25e-3, rel=1e-9)     # the other block is still served
    with pytest.raises(CedarError, match="singular"):
        dc_sens(c, ["r1"], abstol=1e-12)
    with pytest.raises(CedarError):
        dc_sens(divider(), ["nosuchdevice"])


def test_a_failed_sample_is_reported_and_the_others_are_served(E):
    """Sample 1 has no operating point: its resistor is infinite, so a current source feeds a node that nothing else holds (the
    construction of test_singular_and_invalid_inputs).  It comes back with its ch_dc status and NaN rows — except the known node's
    row, which never depended on the solve — while sample 0 gets its derivatives."""
    c = divider(observe_branch=False)
    c.I("i1", "a", 0, dc=1e-3)
    c.R("ra", "a", 0, 1e3)
    ids = [c.slot("ra"), c.slot("r1"), c.slot("v")]
    e = E(c)
    e.set_samples(2)
    e.set_params(ids[:1], [[1e3, math.inf]])
    rc, x, s, status, st = e.dc_sens(ids, dc_opts(abstol=1e-12, n_restarts=2, maxiters=5))
    a, out, vcc = c.mna_index("v", "a"), c.mna_index("v", "out"), c.mna_index("v", "vcc")
    assert rc == -3 and status[0] == 0 and status[1] != 0
    assert abs(s[0][0][a]) == pytest.approx(1e-3, rel=1e-9) and s[0][0][out] == 0.0           # |d(I R)/dR| = I
    assert s[0][1][out] == pytest.approx(-0.25e-3, rel=1e-9) and s[0][2][out] == pytest.approx(0.5, rel=1e-12)
    assert np.isnan(s[1][:, [a, out]]).all() and s[1][2][vcc] == 1.0 and s[1][0][vcc] == 0.0


# ---- 12. sweeps ----
def test_circuit_sweep_differentiates_every_point_at_its_own_parameters():
    def build(r1=1e3):
        c = Circuit()
        c.V("v", "vcc", 0, dc=2.0)
        c.R("r1", "vcc", "out", r1)
        c.R("r2", "out", 0, 1e3)
        return c

    cs = CircuitSweep(build, Sweep(r1=[500.0, 1e3, 4e3]))
    sols = dc_sens(cs, ["r1", "r2", "v"], abstol=1e-12)
    assert len(sols) == 3
    for sol, p in zip(sols, cs):
        r1, r2, V = p["r1"], 1e3, 2.0
        assert sol.rc == 0 and sol.op.params == p
        assert sol["out", "r1"] == pytest.approx(-V * r2 / (r1 + r2) ** 2, rel=1e-9)
        assert sol["out", "r2"] == pytest.approx(+V * r1 / (r1 + r2) ** 2, rel=1e-9)
        assert sol["out", "v"] == pytest.approx(r2 / (r1 + r2), rel=1e-12)
        assert sol.op["node_out"][0] == pytest.approx(V * r2 / (r1 + r2), rel=1e-12)
