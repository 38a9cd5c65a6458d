"""Self-consistency of the oracle's BSIM4 restatement.  The device arithmetic is PARITY UNPINNED
against the reference (bsim4.va is not in /root/reference); these tests pin what can be pinned:
dual-number derivatives vs finite differences, KCL / charge neutrality, source-drain symmetry,
polarity mirror, temperature and gmin behaviour; then the same on every card variant of bsim4_cards.py, with
identities between the model's branches, a conditioning guard for the shared bias set and the refusal of
sub-models that are not implemented.  CPU only."""
import ctypes

import numpy as np

from cedarsim_jl_amd import Circuit
from cedarsim_jl_amd import bsim4_params as B4
from cedarsim_jl_amd.workloads import gf180_models
from oracle_binding import Oracle


def two_fets(**kw):
    c = Circuit(**kw)
    m = gf180_models()
    n, p = c.add_model(*m["nfet_06v0"]), c.add_model(*m["pfet_06v0"])
    c.M("mn", "d", "g", "s", "b", n, 3.6e-7, 6e-7)
    c.M("mp", "d", "g", "s", "b", p, 4.95e-7, 5e-7)
    return c


def test_dual_derivatives_match_finite_differences():
    o = Oracle(two_fets())
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(100):
        v = rng.uniform(-1, 6, size=(2, 4))
        v[1] = -v[1]
        out = o.mos_eval(v)
        h = 1e-6
        for k in range(2):
            for j in range(4):
                vp, vm = v.copy(), v.copy()
                vp[k, j] += h
                vm[k, j] -= h
                fd = (o.mos_eval_values(vp)[k] - o.mos_eval_values(vm)[k]) / (2 * h)
                g = np.concatenate([out[k, 8:24].reshape(4, 4)[:, j], out[k, 24:40].reshape(4, 4)[:, j]])
                scale = np.concatenate([np.full(4, 1e-9 + np.abs(out[k, 8:24]).max()), np.full(4, 1e-20 + np.abs(out[k, 24:40]).max())])
                worst = max(worst, np.max(np.abs(fd - g) / scale))
    assert worst < 1e-6


def test_kcl_and_charge_neutrality():
    o = Oracle(two_fets())
    rng = np.random.default_rng(1)
    v = rng.uniform(-1, 6, size=(2, 4))
    out = o.mos_eval(v)
    for k in range(2):
        assert abs(out[k, 0:4].sum()) < 1e-12 * np.abs(out[k, 0:4]).max() + 1e-18  # currents sum to zero
        assert abs(out[k, 4:8].sum()) < 1e-12 * np.abs(out[k, 4:8]).max()            # charges sum to zero
        G, C = out[k, 8:24].reshape(4, 4), out[k, 24:40].reshape(4, 4)
        assert np.abs(G.sum(axis=1)).max() < 1e-9 * np.abs(G).max()  # rows sum to zero: only differences matter
        assert np.abs(C.sum(axis=1)).max() < 1e-9 * np.abs(C).max()
        assert np.abs(G.sum(axis=0)).max() < 1e-9 * np.abs(G).max()


def test_source_drain_symmetry_and_zero_vds():
    o = Oracle(two_fets())
    v = np.array([[1.3, 3.0, 0.4, 0.0], [0.0, 0.0, 0.0, 0.0]])
    vs = v.copy()
    vs[0, [0, 2]] = v[0, [2, 0]]  # swap drain and source voltages
    a, b = o.mos_eval(v)[0], o.mos_eval(vs)[0]
    assert abs(a[0] - b[2]) < 1e-12 * abs(a[0]) and abs(a[2] - b[0]) < 1e-12 * abs(a[0])  # Id <-> Is
    assert abs(a[4] - b[6]) < 1e-9 * abs(a[5])  # Qd <-> Qs
    z = o.mos_eval(np.array([[2.0, 3.0, 2.0, 0.0], [0, 0, 0, 0.0]]))[0]
    assert abs(z[0] - z[2]) < 1e-18 and abs(z[0] + z[2] + z[3]) < 1e-18  # vds=0: no channel current, only the two (equal) junction leakages


def test_iv_is_monotonic_and_off_current_small():
    o = Oracle(two_fets())
    ids = [o.mos_eval(np.array([[5.0, vg, 0.0, 0.0], [0, 0, 0, 0.0]]))[0][0] for vg in np.linspace(0, 5, 26)]
    assert all(b > a for a, b in zip(ids, ids[1:]))
    assert ids[0] < 1e-9 and 5e-5 < ids[-1] < 5e-4
    idp = o.mos_eval(np.array([[0, 0, 0, 0.0], [-5.0, -5.0, 0.0, 0.0]]))[1][0]
    assert -5e-4 < idp < -2e-5


def test_pmos_is_mirror_of_nmos_with_mirrored_card():
    m = gf180_models()
    c = Circuit()
    pn = dict(m["nfet_06v0"][2])
    n = c.add_model("n", "nmos", pn)
    pp = dict(pn)
    pp["vth0"] = -pn["vth0"]
    p = c.add_model("p", "pmos", pp)
    c.M("mn", "d", "g", "s", "b", n, 1e-6, 6e-7)
    c.M("mp", "d", "g", "s", "b", p, 1e-6, 6e-7)
    o = Oracle(c)
    v = np.array([[2.0, 3.0, 0.2, -0.3]])
    out = o.mos_eval(np.vstack([v, -v]))
    assert np.allclose(out[0, :8], -out[1, :8], rtol=1e-12, atol=1e-30)
    assert np.allclose(out[0, 8:], out[1, 8:], rtol=1e-12, atol=1e-30)


def test_temperature_and_gmin_slots():
    c = two_fets(gmin=1e-12)
    st, sg = c.slot("temp"), c.slot("gmin")
    o = Oracle(c)
    v = np.array([[5.0, 5.0, 0.0, 0.0], [0, 0, 0, 0.0]])
    i27 = o.mos_eval(v)[0][0]
    o.set_param(st, 125.0)
    i125 = o.mos_eval(v)[0][0]
    assert i125 < i27  # mobility degradation wins at high Vgs
    off = np.array([[5.0, 0.0, 0.0, 0.0], [0, 0, 0, 0.0]])
    o.set_param(st, 27.0)
    a = o.mos_eval(off)[0][0]
    o.set_param(sg, 1e-9)
    b = o.mos_eval(off)[0][0]
    assert abs((b - a) - (1e-9 - 1e-12) * 5.0) < 1e-12  # gmin sits across the drain-bulk junction


# ------------------------------------------------------------------------------------------------
# The card space (tests/bsim4_cards.py): the checks above on every variant, and identities between model branches that
# hold whatever the restatement says about any one of them.
import pytest  # noqa: E402

import bsim4_cards as BC  # noqa: E402
from cedarsim_jl_amd.circuit import ERR_UNSUPPORTED  # noqa: E402

ROWS = BC.bias_rows()
VBANK = BC.bank_voltages(ROWS)
_bank = {}


def bank(variant, **kw):
    """Oracle of the whole bias set on one variant (or on a dict of card overrides), built once."""
    key = (variant if isinstance(variant, str) else tuple(sorted(variant.items())), tuple(sorted(kw.items())))
    if key not in _bank:
        _bank[key] = Oracle(BC.two_fets(variant, rows=len(ROWS), **kw))
    return _bank[key]


def records(variant, **kw):
    return bank(variant, **kw).mos_eval(VBANK)


@pytest.mark.parametrize("name", BC.NAMES)
def test_variant_dual_derivatives_match_finite_differences(name):
    o = Oracle(BC.two_fets(name))
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(100):
        v = rng.uniform(-1, 6, size=(2, 4))
        v[1] = -v[1]
        out = o.mos_eval(v)
        h = 1e-6
        for j in range(4):
            vp, vm = v.copy(), v.copy()
            vp[:, j] += h
            vm[:, j] -= h
            fd = (o.mos_eval_values(vp) - o.mos_eval_values(vm)) / (2 * h)
            for k in range(2):
                g = np.concatenate([out[k, 8:24].reshape(4, 4)[:, j], out[k, 24:40].reshape(4, 4)[:, j]])
                scale = np.concatenate([np.full(4, 1e-9 + np.abs(out[k, 8:24]).max()), np.full(4, 1e-20 + np.abs(out[k, 24:40]).max())])
                worst = max(worst, np.max(np.abs(fd[k] - g) / scale))
    assert worst < 1e-6, (name, worst)


@pytest.mark.parametrize("name", BC.NAMES)
def test_variant_kcl_and_charge_neutrality(name):
    o = Oracle(BC.two_fets(name))
    rng = np.random.default_rng(1)
    for _ in range(20):
        v = rng.uniform(-1, 6, size=(2, 4))
        out = o.mos_eval(v)
        for k in range(2):
            assert abs(out[k, 0:4].sum()) < 1e-12 * np.abs(out[k, 0:4]).max() + 1e-18
            assert abs(out[k, 4:8].sum()) < 1e-12 * np.abs(out[k, 4:8]).max()
            G, C = out[k, 8:24].reshape(4, 4), out[k, 24:40].reshape(4, 4)
            assert np.abs(G.sum(axis=1)).max() < 1e-9 * np.abs(G).max()
            assert np.abs(C.sum(axis=1)).max() < 1e-9 * np.abs(C).max()
            assert np.abs(G.sum(axis=0)).max() < 1e-9 * np.abs(G).max()


@pytest.mark.parametrize("name", BC.NAMES)
def test_variant_source_drain_symmetry_and_zero_vds(name):
    o, om = Oracle(BC.two_fets(name)), Oracle(BC.two_fets(name, mirror=True))   # the mirrored instance: as/ad and ps/pd exchanged
    v = np.array([[1.3, 3.0, 0.4, 0.0], [0.0, 0.0, 0.0, 0.0]])
    vs = v.copy()
    vs[0, [0, 2]] = v[0, [2, 0]]
    a, b = o.mos_eval(v)[0], om.mos_eval(vs)[0]
    assert abs(a[0] - b[2]) < 1e-12 * abs(a[0]) and abs(a[2] - b[0]) < 1e-12 * abs(a[0])
    assert abs(a[4] - b[6]) <= 1e-9 * abs(a[5])   # "<=": a card without gate charge (capmod 0) must swap exactly
    z = o.mos_eval(np.array([[2.0, 3.0, 2.0, 0.0], [0, 0, 0, 0.0]]))[0]
    assert abs(z[0] - z[2]) < 1e-18 and abs(z[0] + z[2] + z[3]) < 1e-18


def test_mobility_models_coincide_without_degradation():
    """ua = ub = uc = 0 (and their temperature slopes): the three mobility models differ only in how the degradation terms
    enter the denominator, so they give one record."""
    recs = [records(dict(BC._NOMOB, mobmod=m)) for m in (0, 1, 2)]
    assert np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2])
    assert not np.array_equal(recs[0], records("base"))   # and the degradation terms do matter on these rows


def test_charge_partition_moves_only_the_split_between_drain_and_source():
    r0, r5, r1 = records("base"), records("xp05"), records("xp1")
    sc = BC.row_scales(r0)
    assert not np.allclose(r0[:, 4], r1[:, 4], rtol=1e-3, atol=0) and not np.allclose(r5[:, 4], r1[:, 4], rtol=1e-3, atol=0)
    for r in (r5, r1):
        keep = np.r_[0:4, 5, 7, 8:24, 28:32, 36:40]   # currents, qg, qb, G, and the gate and bulk rows of C
        assert np.array_equal(r[:, keep], r0[:, keep])
        # qd + qs = -(qg + qb) and its derivatives: equal up to the rounding of the two sums
        assert np.max(np.abs((r[:, 4] + r[:, 6]) - (r0[:, 4] + r0[:, 6])) / sc[:, 4]) < 1e-14
        assert np.max(np.abs((r[:, 24:28] + r[:, 32:36]) - (r0[:, 24:28] + r0[:, 32:36])) / sc[:, 24:28]) < 1e-14
    # vds = 0: the channel charge splits evenly whatever the partition
    sym = np.repeat(ROWS[:, 0] == ROWS[:, 2], 2)
    assert sym.sum() >= 8
    for r in (r0, r5, r1):
        assert np.max(np.abs(r[sym, 4] - r[sym, 6]) / sc[sym, 4]) < 1e-13


def test_no_intrinsic_charge_for_negative_xpart_and_capmod_0():
    nojn = BC.VARIANTS["nojn"][0]
    noov = dict(cgso=0.0, cgdo=0.0, cgbo=0.0, cf=0.0, cgsl=0.0, cgdl=0.0)
    # without junction capacitance: capmod 0 leaves no charge at all (intrinsic, overlap and gate-bulk charges are gone) ...
    r = records(dict(nojn, capmod=0))
    assert np.all(r[:, 4:8] == 0.0) and np.all(r[:, 24:40] == 0.0)
    # ... xpart < 0 only the overlap charges
    r = records(dict(nojn, xpart=-1.0))
    assert np.abs(r[:, 24:40]).max() > 0.0
    r = records(dict(nojn, xpart=-1.0, **noov))
    assert np.all(r[:, 4:8] == 0.0) and np.all(r[:, 24:40] == 0.0)
    # with junctions: both are the junction charges alone, and the currents never notice
    a, b, base = records("cap0"), records(dict(xpart=-1.0, **noov)), records("base")
    assert np.array_equal(a[:, 4:8], b[:, 4:8]) and np.array_equal(a[:, 24:40], b[:, 24:40]) and np.abs(a[:, 24:40]).max() > 0.0
    assert np.all(a[:, 5] == 0.0) and np.all(a[:, 28:32] == 0.0)   # nothing on the gate
    for r in (a, b, records("xpneg")):
        assert np.array_equal(r[:, 0:4], base[:, 0:4]) and np.array_equal(r[:, 8:24], base[:, 8:24])


def test_poly_depletion_is_off_on_both_sides_of_its_window():
    a, b = records("ngate0"), records("ngate_hi")
    assert np.array_equal(a, b)
    assert not np.array_equal(a[:, 0], records("base")[:, 0])   # inside the window (the GF180 cards) it acts


def test_impact_ionisation_flows_from_the_mode_drain_to_the_bulk():
    a, b = records("isub"), records("isub0")
    md = np.where(np.repeat(ROWS[:, 0] >= ROWS[:, 2], 2), 0, 2)   # terminal that acts as the drain
    rows = np.arange(len(a))
    dI = a[:, 0:4] - b[:, 0:4]
    assert np.all(dI[:, 1] == 0.0) and np.all(dI[rows, 2 - md] == 0.0)
    sI = BC.row_scales(b)[:, 0]
    assert np.max(np.abs(dI[rows, md] + dI[:, 3]) / sI) < 1e-14
    assert np.max(np.abs(dI[rows, md]) / sI) > 1e-3                # it is a current worth the name on some rows
    assert np.all((a[rows, md] - b[rows, md]) * np.where(rows % 2 == 0, 1.0, -1.0) >= 0.0)   # into the drain of the NMOS, out of the PMOS's
    assert np.array_equal(a[:, 4:8], b[:, 4:8]) and np.array_equal(a[:, 24:40], b[:, 24:40])
    G = (a[:, 8:24] - b[:, 8:24]).reshape(-1, 4, 4)
    assert np.all(G[:, 1, :] == 0.0) and np.all(G[rows, 2 - md, :] == 0.0)


def test_dead_junctions_leave_gmin_alone():
    gmin = 1e-9
    ov = dict(BC.VARIANTS["nojn"][0], alpha0=0.0, agidl=0.0, capmod=0)
    r = records(ov, gmin=gmin)
    vd, vg, vs, vb = VBANK.T
    want = gmin * (vb - vs) + gmin * (vb - vd)                     # into the bulk, through both junctions
    assert np.max(np.abs(r[:, 3] - want)) <= 4e-16 * gmin * np.abs(VBANK).max() * 4
    assert np.all(r[:, 1] == 0.0) and np.max(np.abs(r[:, 0:4].sum(axis=1))) <= 1e-12 * np.abs(r[:, 0:4]).max()
    G = r[:, 8:24].reshape(-1, 4, 4)
    assert np.allclose(G[:, 3, 3], 2 * gmin, rtol=1e-15, atol=0) and np.allclose(G[:, 3, 0], -gmin, rtol=1e-15, atol=0) and np.allclose(G[:, 3, 2], -gmin, rtol=1e-15, atol=0)
    assert np.all(r[:, 4:8] == 0.0) and np.all(r[:, 24:40] == 0.0)


@pytest.mark.parametrize("name", BC.NAMES)
def test_bias_set_is_well_conditioned(name):
    """What rounding of the INPUT alone does to the reference: one terminal moved by 1e-14 V changes no slot of the record
    by more than 2e-11 of its row scale (1e-14 V against the 1 mV floor of the scale is 1e-11 by construction).  The GPU
    comparison at 1e-10 (test_gpu_bsim4_cards.py) therefore has a margin of 5 over it.  Rows with vd == vs sit on the mode
    switch, where the record is discontinuous under perturbation: they are excluded HERE only — the GPU comparison keeps
    them, both sides seeing the same exact input."""
    o = bank(name)
    ref = o.mos_eval(VBANK)
    sc = BC.row_scales(ref)
    on = np.repeat(ROWS[:, 0] != ROWS[:, 2], 2)
    worst = 0.0
    for j in range(4):
        for dv in (1e-14, -1e-14):
            v = VBANK.copy()
            v[:, j] += dv
            assert np.all(np.sign(v[on, 0] - v[on, 2]) == np.sign(VBANK[on, 0] - VBANK[on, 2]))   # no row changes its mode
            worst = max(worst, np.max((np.abs(o.mos_eval(v) - ref) / sc)[on]))
    assert worst <= 2e-11, (name, worst)


FAR_ROWS = BC.far_bias_rows()
FAR_VBANK = BC.bank_voltages(FAR_ROWS)
FAR_TEMPS = (-40.0, 27.0, 125.0)


def far_conditioning(name):
    """per far row: the input-rounding measure of test_bias_set_is_well_conditioned (the worse of the NMOS and the PMOS of the pair),
    at the three temperatures; the records are asserted finite on the way"""
    c = BC.two_fets(name, rows=len(FAR_ROWS))
    o = Oracle(c)
    st = c.slot("temp")
    worst = np.zeros(len(FAR_ROWS))
    for temp in FAR_TEMPS:
        o.set_param(st, temp)
        ref = o.mos_eval(FAR_VBANK)
        assert np.all(np.isfinite(ref)), (name, temp, FAR_ROWS[np.nonzero(~np.isfinite(ref).all(axis=1))[0] // 2].tolist())
        sc = BC.row_scales(ref)
        for j in range(4):
            for dv in (1e-14, -1e-14):
                v = FAR_VBANK.copy()
                v[:, j] += dv
                e = (np.abs(o.mos_eval(v) - ref) / sc).max(axis=1)
                worst = np.maximum(worst, np.maximum(e[0::2], e[1::2]))
    return worst


@pytest.mark.parametrize("name", BC.NAMES)
def test_far_bias_rows_are_finite_and_well_conditioned(name):
    """The far-bias rows (20 V and 40 V): every oracle record is finite at -40, 27 and 125 C, and on the rows the GPU comparison
    keeps (all but BC.FAR_ILL_CONDITIONED, at least 90 % of them) one terminal moved by 1e-14 V changes no slot by more than 2e-11 of
    its row scale.  The row with all four terminals equal sits on the mode switch and is excluded HERE only, as in
    test_bias_set_is_well_conditioned."""
    worst = far_conditioning(name)
    keep = np.array([i not in BC.FAR_ILL_CONDITIONED for i in range(len(FAR_ROWS))])
    assert keep.mean() >= 0.9 and len(BC.far_admitted_rows()) == keep.sum()
    on = FAR_ROWS[:, 0] != FAR_ROWS[:, 2]
    over = np.nonzero(keep & on & ~(worst <= 2e-11))[0]
    assert over.size == 0, (name, [(int(i), FAR_ROWS[i].tolist(), float(worst[i])) for i in over])


@pytest.mark.parametrize("sel,val", BC.UNSUPPORTED_SELECTORS)
def test_unimplemented_sub_models_are_refused(sel, val):
    o = Oracle(BC.two_fets({sel: float(val)}))
    out = np.zeros((2, 40))
    rc = o.L.oracle_mos_eval(o.h, VBANK[:2].ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == ERR_UNSUPPORTED, (sel, val, rc)
    assert o.dc()[0] == ERR_UNSUPPORTED
