"""GPU tests of the frequency-domain measurements at the kernels' shape edges: ch_freq_measure_rows on the synthetic complex rows of
tests/fmeasure_cases.py, both kernel forms on the same rows through CEDARHIP_MEASURE_SPLIT.

Sample counts 1, 2, 63, 64, 65, 130 (a wavefront short of, at and past 64 lanes; more than one block) and grid sizes 1, 2, 3, 63, 64, 65,
129 (the split form with empty lanes, with one interval on all but two lanes, on all but one, on every lane, with two on every lane).
On 129 rows the phase of row 0 wraps in the first interval of every lane's chunk, the wrap count of row 1 grows to 35, and the wanted
event of the gain row sits in the first, a middle and the last chunk.  Every kind and signal on both axes, without sensitivities and
with 1 and 3 parameters.  Per (measure, sample) the 40-digit yardstick (tests/fmeasure_reference.py) under the rule
max(1e-12, 32 e_cpu), on rows for which the float64 reference is itself inside 1e-12 (fmeasure_cases.reference asserts it); statuses
and NaN positions exactly; event frequencies, FIND_*, MIN, MAX and every figure read from the unwrapped phase bit-equal between the
forms; a batch's sample bit-equal to a one-sample call; 130 samples in chunks of 64, 64, 2 and of one bit-equal to one launch."""
import ctypes as C

import numpy as np
import pytest

import fmeasure_cases as fc
import fmeasure_reference as fr
from cedarsim_jl_amd.circuit import CedarError

pytestmark = pytest.mark.gpu
FORMS = ("lanes", "time")


@pytest.fixture(scope="module")
def ctx():
    from cedarsim_jl_amd.engine import default_context
    return default_context()


def run(ctx, monkeypatch, form, f, values, sens, specs):
    if form is None:
        monkeypatch.delenv("CEDARHIP_MEASURE_SPLIT", raising=False)
    else:
        monkeypatch.setenv("CEDARHIP_MEASURE_SPLIT", form)
    return ctx.freq_measure_rows(f, values, fc.to_ctypes(specs), len(specs), sens)


@pytest.mark.parametrize("nf", fc.FREQS_AT)
@pytest.mark.parametrize("form", FORMS)
def test_every_kind_against_the_yardstick_at_every_grid_size(ctx, monkeypatch, nf, form):
    """65 samples (one full wavefront and one lane of the next in the lanes form; 65 wavefronts in the split form), 3 parameters."""
    specs, exp = fc.specs_for(nf), fc.expected(nf)
    f, values, sens = fc.batch(nf, 65, 3)
    val, status, ds = run(ctx, monkeypatch, form, f, values, sens, specs)
    fc.compare("%d rows, %s" % (nf, form), specs, lambda s: exp[s % fc.N_VARIANTS], val, status, ds, 3)


@pytest.mark.parametrize("S", fc.SAMPLES_AT)
@pytest.mark.parametrize("n_par", (0, 1))
def test_every_sample_count_in_both_forms(ctx, monkeypatch, S, n_par):
    """65 and 129 rows; the default form — lanes from 64 samples up — must be one of the two, bit for bit; the forms agree bit for bit
    where the same functions see the same arguments, the unwrapped phase included."""
    for nf in (65, 129):
        specs, exp = fc.specs_for(nf), fc.expected(nf)
        f, values, sens = fc.batch(nf, S, n_par)
        got = {form: run(ctx, monkeypatch, form, f, values, sens, specs) for form in FORMS + (None,)}
        for form in FORMS:
            val, status, ds = got[form]
            fc.compare("%d rows, %d samples, %s" % (nf, S, form), specs, lambda s: exp[s % fc.N_VARIANTS], val, status, ds, n_par, verbose=(S == 130))
        default = "lanes" if S >= 64 else "time"
        assert all(fc.same_bits(a, b) for a, b in zip(got[None][:2], got[default][:2])), "the default form at %d samples is not '%s'" % (S, default)
        assert np.array_equal(got["lanes"][1], got["time"][1])
        for k, sp in enumerate(specs):
            if sp["kind"] in fc.BIT_EQUAL_KINDS:
                assert fc.same_bits(got["lanes"][0][k], got["time"][0][k]), "%s (measure %d): the two forms differ in a value" % (sp["kind"], k)
                if n_par:
                    assert fc.same_bits(got["lanes"][2][k], got["time"][2][k]), "%s (measure %d): the two forms differ in a derivative" % (sp["kind"], k)


def test_a_sample_of_a_batch_has_the_bits_of_a_one_sample_call_and_calls_repeat(ctx, monkeypatch):
    nf, S, n_par = 129, 130, 3
    specs = fc.specs_for(nf)
    f, values, sens = fc.batch(nf, S, n_par)
    for form in FORMS:
        first = run(ctx, monkeypatch, form, f, values, sens, specs)
        again = run(ctx, monkeypatch, form, f, values, sens, specs)
        assert all(fc.same_bits(a, b) for a, b in zip(first, again)), "%s: a repeated call differs" % form
        for s in (0, 63, 64, 129):
            one = run(ctx, monkeypatch, form, f, np.ascontiguousarray(values[:, :, s:s + 1]), np.ascontiguousarray(sens[:, :, :, s:s + 1]), specs)
            assert fc.same_bits(one[0][:, 0], first[0][:, s]) and np.array_equal(one[1][:, 0], first[1][:, s]) and fc.same_bits(one[2][:, :, 0], first[2][:, :, s]), (form, s)


@pytest.mark.parametrize("n_par", (0, 3))
def test_a_samples_result_does_not_depend_on_its_chunk(ctx, monkeypatch, n_par):
    """130 samples on 65 rows with the rows one launch may hold capped (CEDARHIP_MEASURE_CAP) so that the samples go in chunks of 64, 64
    and 2 (three complex rows, and their sensitivity rows, of 65 frequencies per sample: 64 samples fit, 65 do not), and again in chunks
    of one sample: the bits of the one-launch call, in either form, and the yardstick."""
    nf, S = 65, 130
    specs, exp = fc.specs_for(nf), fc.expected(nf)
    f, values, sens = fc.batch(nf, S, n_par)
    per_sample = 2 * 3 * nf * (1 + n_par)
    for form in FORMS:
        monkeypatch.delenv("CEDARHIP_MEASURE_CAP", raising=False)
        whole = run(ctx, monkeypatch, form, f, values, sens, specs)
        for cap in (64 * per_sample + per_sample // 2, per_sample):
            monkeypatch.setenv("CEDARHIP_MEASURE_CAP", str(cap))
            parts = run(ctx, monkeypatch, form, f, values, sens, specs)
            assert fc.same_bits(parts[0], whole[0]) and np.array_equal(parts[1], whole[1]) and (n_par == 0 or fc.same_bits(parts[2], whole[2])), (form, cap)
        fc.compare("chunks, %s" % form, specs, lambda s: exp[s % fc.N_VARIANTS], parts[0], parts[1], parts[2], n_par, verbose=False)
    monkeypatch.delenv("CEDARHIP_MEASURE_CAP", raising=False)


def test_nan_rows_and_a_zero_response_of_one_sample_leave_its_neighbours_alone(ctx, monkeypatch):
    """65 samples on 65 rows; sample 3 carries NaN from row 30 on in row 0 and H = 0 at row 50 of row 1: its own measures follow the
    yardstick on ITS rows (statuses and NaN positions exactly), samples 2 and 4 — its neighbours in memory — those of clean rows."""
    nf, S, bad = 65, 65, 3
    specs, exp = fc.specs_for(nf), fc.expected(nf)
    f, values, sens = fc.batch(nf, S, 1)
    values[0, 30:, bad] = np.nan
    values[1, 50, bad] = 0.0
    mine = fc.references(specs, f, np.ascontiguousarray(values[:, :, bad]), np.ascontiguousarray(sens[:, :, :, bad]))
    assert {r["status"] for r in mine} >= {0, 3}, "the case must hold measures the bad rows spoil and measures they do not reach"
    for form in FORMS:
        val, status, ds = run(ctx, monkeypatch, form, f, values, sens, specs)
        fc.compare("NaN rows, %s" % form, specs, lambda s: mine if s == bad else exp[s % fc.N_VARIANTS], val, status, ds, 1)
        for k, r in enumerate(mine):
            assert np.isnan(val[k, bad]) == (r["status"] in (1, 2, 3)) and np.isnan(ds[k, 0, bad]) == (r["status"] != 0)


def test_invalid_specs_and_grids_are_refused_by_name_before_anything_runs(ctx, monkeypatch):
    nf = 8
    f, values, sens = fc.batch(nf, 2, 1)
    S = fr.side
    good = fr.spec("when", S(0, sig="db", level=0.5))
    for bad_spec, text in ((fr.spec("when", S(3, level=0.5)), "row out of range"), (fr.spec("max", S(0, 7)), "row out of range"),
                           (fr.spec("when", S(0, level=0.5, count=0)), "count"), (fr.spec("find_when", S(0, level=float("inf")), S(1)), "non-finite level"),
                           (fr.spec("find_at", S(0), at=-1.0), "LOG"), (fr.spec("when", S(0, level=0.5, ref_at=0.0)), "LOG")):
        with pytest.raises(CedarError) as e:
            run(ctx, monkeypatch, None, f, values, sens, [good, bad_spec])
        assert "measure 1" in str(e.value) and text in str(e.value), str(e.value)
    lin = fr.spec("find_at", S(0), at=5.0, xscale="lin")
    g = f.copy()
    g[3] = g[2]
    with pytest.raises(CedarError, match="strictly increasing"):
        run(ctx, monkeypatch, None, g, values, sens, [lin])
    g = f.copy()
    g[0] = 0.0
    assert run(ctx, monkeypatch, None, g, values, sens, [lin])[1][0, 0] == 0          # 0 Hz is a frequency on a LIN axis,
    with pytest.raises(CedarError, match="LOG axis needs every frequency > 0"):        # and none on a LOG axis
        run(ctx, monkeypatch, None, g, values, sens, [good])
    # sensitivities asked of rows that carry none: straight through the C entry point
    from cedarsim_jl_amd.engine import _pf64, _pi32
    v = np.ascontiguousarray(values).view(np.float64)
    val, st, ds = np.zeros((1, 2)), np.zeros((1, 2), np.int32), np.zeros((1, 1, 2))
    rc = ctx.L.ch_freq_measure_rows(ctx.h, nf, f.ctypes.data_as(_pf64), 3, 2, v.ctypes.data_as(_pf64), 0, None, 1, fc.to_ctypes([good]), val.ctypes.data_as(_pf64),
                                    ds.ctypes.data_as(_pf64), st.ctypes.data_as(_pi32))
    assert rc == -1 and "carry none" in ctx.last_error()
    assert C.sizeof(fc.ChFMeasureSpec) == 144
