"""CPU: the synthetic rows of tests/fmeasure_cases.py are what the GPU tests of the frequency-domain measurements take them for, and
the float64 reference is inside 1e-12 of the 40-digit yardstick for every (kind, grid size) — `fmeasure_cases.reference` asserts it."""
import numpy as np
import pytest

import fmeasure_cases as fc
import fmeasure_reference as fr


@pytest.mark.parametrize("nf", fc.FREQS_AT)
def test_the_float64_reference_is_inside_1e_12_on_every_case(nf):
    exp = fc.expected(nf)
    assert max(r["e_cpu"] for v in exp for r in v) <= 1e-12
    assert len(exp) == fc.N_VARIANTS and len(exp[0]) == len(fc.specs_for(nf))


def test_the_rows_are_what_the_cases_promise():
    """CPU: on 129 rows the gain row's three events lie in the first, a middle and the last lane chunk, row 0's phase wraps in the first
    interval of every chunk, and row 1's wrap count passes 30."""
    nf = 129
    f, specs, exp = fc.grid(nf), fc.specs_for(nf), fc.expected(nf)
    for v in range(fc.N_VARIANTS):
        where = [int(np.searchsorted(f, float(exp[v][k]["value"]))) for k in range(3)]   # the interval of each event
        assert all(exp[v][k]["status"] == 0 for k in range(3)) and where[0] in (1, 2) and 20 < where[1] < 110 and where[2] in (127, 128), where
        H = fc.variant_rows(nf, v)[0]
        raw = np.degrees(np.angle(H[0]))
        d = np.diff(raw)
        assert np.all((d > 180) | (d <= -180) == (np.arange(1, nf) % 2 == 1)), "a wrap in every odd interval, none in the even ones"
        g1 = fr.signal_rows(f, H, None, fr.side(1, sig="phase"))[0]
        assert g1[-1] < -30 * 360.0
    assert {r["status"] for v in exp for r in v} >= {0, 1, 2}
