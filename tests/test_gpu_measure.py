"""GPU tests of the waveform measurements at the kernels' shape edges: ch_measure_rows on the synthetic rows of tests/measure_cases.py,
both kernel forms on the same rows through CEDARHIP_MEASURE_SPLIT.

Sample counts 1, 63, 64, 65, 130 (a wavefront short of, at and past 64 lanes; more than one block) and row counts 1, 2, 3, 64, 65, 66,
129 (the time split with empty lanes, with exactly one interval per lane, with a second interval on one lane, with two on every lane);
on 129 rows one event sits exactly on a lane-chunk boundary, and one window of every row count has its ends inside the first and the
last chunk.  Every kind, without sensitivities and with 1 and 3 parameters.  Per (measure, sample) the 40-digit yardstick
(tests/measure_reference.py) under the rule max(1e-12, 32 e_cpu); statuses and NaN positions exactly; event times, FIND_*, MIN and MAX
bit-equal between the forms; a batch's sample bit-equal to a one-sample call; a repeated call bit-equal."""
import numpy as np
import pytest

import measure_cases as mc
import measure_reference as mr
from cedarsim_jl_amd.circuit import CedarError

pytestmark = pytest.mark.gpu
FORMS = ("lanes", "time")


@pytest.fixture(scope="module")
def ctx():
    from cedarsim_jl_amd.engine import default_context
    return default_context()


def run(ctx, monkeypatch, form, t, pts, values, sens, specs):
    if form is None:
        monkeypatch.delenv("CEDARHIP_MEASURE_SPLIT", raising=False)
    else:
        monkeypatch.setenv("CEDARHIP_MEASURE_SPLIT", form)
    return ctx.measure_rows(t, values, mc.to_ctypes(specs), len(specs), pts, sens)


@pytest.mark.parametrize("nt", mc.ROWS_AT)
@pytest.mark.parametrize("form", FORMS)
def test_every_kind_against_the_yardstick_at_every_row_count(ctx, monkeypatch, nt, form):
    """65 samples (one full wavefront and one lane of the next in the lanes form; 65 wavefronts in the time split), 3 parameters."""
    specs, exp = mc.specs_for(nt), mc.expected(nt)
    t, pts, values, sens = mc.batch(nt, 65, 3)
    val, status, ds = run(ctx, monkeypatch, form, t, pts, values, sens, specs)
    mc.compare("%d rows, %s" % (nt, form), specs, lambda s: exp[s % mc.N_VARIANTS], val, status, ds, 3)


@pytest.mark.parametrize("S", mc.SAMPLES_AT)
@pytest.mark.parametrize("n_par", (0, 1))
def test_every_sample_count_in_both_forms(ctx, monkeypatch, S, n_par):
    """66 rows (lane 0 of the time split has two intervals, lanes 1..63 one, none is empty) and 129 rows; the default form — lanes from
    64 samples up — must be one of the two, bit for bit; the forms agree bit for bit where the same functions see the same arguments."""
    for nt in (66, 129):
        specs, exp = mc.specs_for(nt), mc.expected(nt)
        t, pts, values, sens = mc.batch(nt, S, n_par)
        got = {form: run(ctx, monkeypatch, form, t, pts, values, sens, specs) for form in FORMS + (None,)}
        for form in FORMS:
            val, status, ds = got[form]
            mc.compare("%d rows, %d samples, %s" % (nt, S, form), specs, lambda s: exp[s % mc.N_VARIANTS], val, status, ds, n_par, verbose=(S == 130))
        default = "lanes" if S >= 64 else "time"
        assert all(mc.same_bits(a, b) for a, b in zip(got[None][:2], got[default][:2])), "the default form at %d samples is not '%s'" % (S, default)
        assert np.array_equal(got["lanes"][1], got["time"][1])
        for k, sp in enumerate(specs):
            if sp["kind"] in mc.BIT_EQUAL_KINDS:
                assert mc.same_bits(got["lanes"][0][k], got["time"][0][k]), "%s (measure %d): the two forms differ in a value" % (sp["kind"], k)
                if n_par:
                    assert mc.same_bits(got["lanes"][2][k], got["time"][2][k]), "%s (measure %d): the two forms differ in a derivative" % (sp["kind"], k)


@pytest.mark.parametrize("pts", ([1, 2, 3], [1, 2, 2], [0, 0, 0], [1, 2, 3, 3], [1, 2, 3, 4], [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 7, 8, 8]))
def test_interpolation_weights_read_back_through_unit_rows(ctx, monkeypatch, pts):
    """Row k is 1 at time k and 0 elsewhere, so FIND_AT on row k is the k-th interpolation weight the device used: the window
    (how many rows, which) and the Lagrange weights themselves, inside the last interval, against the float64 reference."""
    nt = len(pts)
    t = mc.times(nt)[0]
    values = np.ascontiguousarray(np.eye(nt)[:, :, None])
    x = t[-1] - 0.4 * (t[-1] - t[-2])
    specs = [mr.spec("find_at", mr.side(k), at=x) for k in range(nt)]
    ref = np.array([float(mr.measure_f64(sp, t, pts, values[:, :, 0])[0]) for sp in specs])
    assert np.count_nonzero(ref) == (max(2, min(pts[-1], mr_max_rows())) if pts[-1] >= 2 else 2)
    for form in FORMS:
        val, status, _ = run(ctx, monkeypatch, form, t, np.array(pts, np.int32), values, None, specs)
        print(form, pts, val[:, 0], ref)
        assert np.all(status == 0) and np.max(np.abs(val[:, 0] - ref)) <= 1e-12 * np.max(np.abs(ref)), (form, val[:, 0], ref)


def mr_max_rows():
    return 8   # MEAS_MAX_PTS of csrc/ch_measure_host.hpp: ch_measure_rows refuses dense point counts above it


def test_the_event_on_a_lane_chunk_boundary_is_found_by_both_forms(ctx, monkeypatch):
    """129 rows: row 4 holds the level exactly and closes the chunk [3, 5) of lane 1; the first crossing of every variant must be that
    row's time, from either form (the yardstick agrees: the comparison above covers it; this pins the construction itself)."""
    nt = 129
    t, pts, values, _ = mc.batch(nt, 3, 0)
    specs = [mr.spec("when", mr.side(0, level=mc.LEVEL, edge="cross", count=n)) for n in (1, 2)]
    for form in FORMS:
        val, status, _ = run(ctx, monkeypatch, form, t, pts, values, None, specs)
        hit = (val == t[mc.BOUNDARY_ROW]) & (status == 0)
        assert np.all(hit.any(axis=0)), (form, val, status)


def test_a_sample_of_a_batch_has_the_bits_of_a_one_sample_call_and_calls_repeat(ctx, monkeypatch):
    nt, S, n_par = 129, 130, 3
    specs = mc.specs_for(nt)
    t, pts, values, sens = mc.batch(nt, S, n_par)
    for form in FORMS:
        first = run(ctx, monkeypatch, form, t, pts, values, sens, specs)
        again = run(ctx, monkeypatch, form, t, pts, values, sens, specs)
        assert all(mc.same_bits(a, b) for a, b in zip(first, again)), "%s: a repeated call differs" % form
        for s in (0, 63, 64, 129):
            one = run(ctx, monkeypatch, form, t, pts, np.ascontiguousarray(values[:, :, s:s + 1]), np.ascontiguousarray(sens[:, :, :, s:s + 1]), specs)
            assert mc.same_bits(one[0][:, 0], first[0][:, s]) and np.array_equal(one[1][:, 0], first[1][:, s]) and mc.same_bits(one[2][:, :, 0], first[2][:, :, s]), (form, s)


@pytest.mark.parametrize("n_par", (0, 3))
def test_a_samples_result_does_not_depend_on_its_chunk(ctx, monkeypatch, n_par):
    """130 samples on 66 rows with the rows one launch may hold capped (CEDARHIP_MEASURE_CAP) so that the samples go in chunks of 64, 64
    and 2 (three state rows, and their sensitivity rows, of 66 times per sample: 64 samples fit, 65 do not), and again in chunks of
    one sample: the bits of the one-launch call, in either form, and the yardstick."""
    nt, S = 66, 130
    specs, exp = mc.specs_for(nt), mc.expected(nt)
    t, pts, values, sens = mc.batch(nt, S, n_par)
    per_sample = 3 * nt * (1 + n_par)
    for form in FORMS:
        monkeypatch.delenv("CEDARHIP_MEASURE_CAP", raising=False)
        whole = run(ctx, monkeypatch, form, t, pts, values, sens, specs)
        for cap in (64 * per_sample + per_sample // 2, per_sample):
            monkeypatch.setenv("CEDARHIP_MEASURE_CAP", str(cap))
            parts = run(ctx, monkeypatch, form, t, pts, values, sens, specs)
            assert mc.same_bits(parts[0], whole[0]) and np.array_equal(parts[1], whole[1]) and (n_par == 0 or mc.same_bits(parts[2], whole[2])), (form, cap)
        mc.compare("chunks, %s" % form, specs, lambda s: exp[s % mc.N_VARIANTS], parts[0], parts[1], parts[2], n_par, verbose=False)
    monkeypatch.delenv("CEDARHIP_MEASURE_CAP", raising=False)


def test_only_lanes_and_time_select_a_form(ctx, monkeypatch):
    """Any other value of CEDARHIP_MEASURE_SPLIT (a typo, the empty string) leaves the default rule: lanes from 64 samples up."""
    nt = 66
    specs = [sp for sp in mc.specs_for(nt) if sp["kind"] in ("integ", "avg", "rms")]     # the kinds whose last bits tell the forms apart
    for S in (3, 64):
        t, pts, values, _ = mc.batch(nt, S, 0)
        got = {form: run(ctx, monkeypatch, form, t, pts, values, None, specs)[0] for form in ("lanes", "time", "", "Time", "lane", None)}
        assert not mc.same_bits(got["lanes"], got["time"]), "the case cannot tell the forms apart"
        for other in ("", "Time", "lane", None):
            assert mc.same_bits(got[other], got["lanes" if S >= 64 else "time"]), (S, other)


def test_nan_rows_of_one_sample_leave_its_neighbours_alone(ctx, monkeypatch):
    """65 samples on 66 rows; sample 3 carries NaN from row 30 on in row 0 and an infinity in row 1: its own measures follow the
    yardstick on ITS rows (statuses and NaN positions exactly), samples 2 and 4 — its neighbours in memory — those of clean rows."""
    nt, S, bad = 66, 65, 3
    specs, exp = mc.specs_for(nt), mc.expected(nt)
    t, pts, values, sens = mc.batch(nt, S, 1)
    values[0, 30:, bad] = np.nan
    values[1, 50, bad] = np.inf
    yb, sb = np.ascontiguousarray(values[:, :, bad]), np.ascontiguousarray(sens[:, :, :, bad])
    mine = []
    for sp in specs:
        v, st, d = mr.measure_mp(sp, t, pts, yb, sb)
        vs, ss = mc.scales(sp, t, yb, sb)
        mine.append(dict(value=v, status=st, sens=d, vs=vs, ss=ss, tol_v=1e-12, tol_s=1e-12, e_cpu=0.0))
        if st == 0:   # the rule's tolerance for the figures that survive
            vf, stf, df = mr.measure_f64(sp, t, pts, yb, sb)
            ev, es = mr.errors([vf], [v], vs)[0], max(mr.errors(df, d, ss))
            assert stf == 0 and ev <= 1e-9 and es <= 1e-9
            mine[-1].update(tol_v=max(1e-12, 32 * ev), tol_s=max(1e-12, 32 * es), e_cpu=max(ev, es))
    assert {r["status"] for r in mine} >= {0, 3}, "the case must hold measures the NaN rows spoil and measures they do not reach"
    for form in FORMS:
        val, status, ds = run(ctx, monkeypatch, form, t, pts, values, sens, specs)
        mc.compare("NaN rows, %s" % form, specs, lambda s: mine if s == bad else exp[s % mc.N_VARIANTS], val, status, ds, 1)
        for k, r in enumerate(mine):
            assert np.isnan(val[k, bad]) == (r["status"] in (1, 2, 3)) and np.isnan(ds[k, 0, bad]) == (r["status"] != 0)


def test_saveat_rows_without_dense_points_are_lines(ctx, monkeypatch):
    """dense_points = NULL (and all zero: the same): piecewise linear, as on a saveat grid."""
    nt = 64
    specs = mc.specs_for(nt)
    t, pts, values, sens = mc.batch(nt, 2, 1)
    refs = [[mc.reference(sp, t, None, *[a[..., s] for a in (values, sens)]) for sp in specs] for s in range(2)]
    for form in FORMS:
        for p in (None, np.zeros(nt, np.int32)):
            val, status, ds = run(ctx, monkeypatch, form, t, p, values, sens, specs)
            mc.compare("lines, %s" % form, specs, lambda s: refs[s], val, status, ds, 1, verbose=False)


def test_invalid_specs_are_refused_by_name_before_anything_runs(ctx, monkeypatch):
    nt = 8
    t, pts, values, sens = mc.batch(nt, 2, 1)
    good = mr.spec("when", mr.side(0, level=0.5))
    for bad_spec, text in ((mr.spec("when", mr.side(3, level=0.5)), "row out of range"), (mr.spec("max", mr.side(0, 7)), "row out of range"),
                           (mr.spec("when", mr.side(0, level=0.5, count=0)), "count"), (mr.spec("delay", mr.side(0, level=0.5), mr.side(1, level=float("nan"))), "non-finite level"),
                           (mr.spec("when", mr.side(0, level=float("inf"))), "non-finite level")):
        with pytest.raises(CedarError) as e:
            run(ctx, monkeypatch, None, t, pts, values, sens, [good, bad_spec])
        assert "measure 1" in str(e.value) and text in str(e.value), str(e.value)
    # sensitivities asked of rows that carry none: straight through the C entry point
    import ctypes as C
    from cedarsim_jl_amd.engine import _pf64, _pi32
    val, st, ds = np.zeros((1, 2)), np.zeros((1, 2), np.int32), np.zeros((1, 1, 2))
    rc = ctx.L.ch_measure_rows(ctx.h, nt, t.ctypes.data_as(_pf64), None, 3, 2, values.ctypes.data_as(_pf64), 0, None, 1, mc.to_ctypes([good]), val.ctypes.data_as(_pf64),
                               ds.ctypes.data_as(_pf64), st.ctypes.data_as(_pi32))
    assert rc == -1 and "carry none" in ctx.last_error()
    assert C.sizeof(mc.ChMeasureSpec) == 112
