"""The outputs of ch_dc_sens, ch_ac_sens, ch_ac, ch_noise, ch_noise_ex, ch_noise_sens, ch_tran_sens and ch_ac_measure — every output array, every status, the
return code and the integer counters of ch_stats — are bit for bit those recorded in tests/golden/sens_driver_bits.npz by
tests/golden/make_sens_driver_bits.py at commit efb4340, the parent of the change that folded the drivers' repeated host code into one
step plan, one state pass, one launcher and one outcome rule.  Those of ch_loop_gain (the lg_ cases) are those
recorded in tests/golden/loopgain_bits.npz at commit c3b763b, the parent of the change that folded the family's dense LU kernels onto
csrc/ch_dense_lu.hpp.  Every driver has a case up to 96 unknowns and one above.  Cases: tests/sens_driver_bits_cases.py."""
import os

import numpy as np
import pytest

from sens_driver_bits_cases import CASES, GOLDEN_FILES, golden_file, run_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DRIVERS = ("dc_", "ac_", "noise_", "tran_", "acm_", "lg_")


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def golden():
    rec = {}
    for name, prefixes in GOLDEN_FILES.items():
        with np.load(os.path.join(GOLDEN, name)) as z:
            assert all(golden_file(k.split("/")[0]) == name for k in z.files) and not set(z.files) & set(rec), name    # every case in its own file, once
            rec.update((k, z[k]) for k in z.files)
    return rec


def differing(a, b):
    """count of elements whose bit patterns differ"""
    if a.dtype.kind in "fc":
        w = a.dtype.itemsize // 8
        return int(np.count_nonzero((a.reshape(-1).view(np.uint64).reshape(-1, w) != b.reshape(-1).view(np.uint64).reshape(-1, w)).any(axis=1)))
    return int(np.count_nonzero(a != b))


def test_every_driver_is_pinned_on_both_sides_of_96_unknowns(golden):
    for d in DRIVERS:
        for above in (False, True):
            assert any(n.startswith(d) and CASES[n][1] == above and n + "/meta" in golden for n in CASES), (d, above)
    assert all(n + "/meta" in golden for n in CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_are_bitwise_those_of_the_parent(E, golden, name):
    got = run_case(E, name)
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want)
    print("%s: meta got %r recorded %r" % (name, got["meta"].tolist(), want["meta"].tolist()))
    assert got["meta"].tolist() == want["meta"].tolist()
    assert (got["meta"][1] > 96) == CASES[name][1]           # the side of the LDS limit the case is about
    assert str(got["stats_names"]) == str(want["stats_names"])
    for nm, g, w in zip(str(got["stats_names"]).split(","), got["stats"].tolist(), want["stats"].tolist()):
        assert g == w, (nm, g, w)
    for k in sorted(got):
        if k in ("meta", "stats", "stats_names"):
            continue
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape)
        n = differing(got[k], want[k])
        if k.endswith("#sha256"):      # a large array, pinned by its digest: its sampled values (…#every) say more about where it moved
            print("%s: %s: the digest of the array's bytes %s" % (name, k, "differs" if n else "is the recorded one"))
        else:
            print("%s: %s %r, %d of %d values differ in their bits" % (name, k, got[k].shape, n, got[k].size))
        assert n == 0, (k, n)
