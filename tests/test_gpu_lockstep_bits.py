"""The device stepper's complete outputs (t, every observed row, the final state without eliminated branches) are bit-for-bit those
recorded in tests/golden/lockstep_bits.npz by tests/golden/make_lockstep_bits.py at commit bc51cfb, the parent of the change that
moved the evaluation's fp64 constants, the linear devices of a wave pair and the pair's live state: none of that
may change what the model computes.  Shapes: tests/lockstep_bits_cases.py."""
import os

import numpy as np
import pytest

from lockstep_bits_cases import CASES, run_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lockstep_bits.npz")


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def differing(a, b):
    """count of elements whose 64-bit patterns differ"""
    return int(np.count_nonzero(a.view(np.uint64) != b.view(np.uint64)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_are_bitwise_those_of_the_parent(E, golden, name):
    got = run_case(E, name)
    want = {k: golden["%s/%s" % (name, k)] for k in got}
    print("%s: meta (stepper, mode, accepted, rejected, iterations) got %r recorded %r" % (name, got["meta"].tolist(), want["meta"].tolist()))
    assert got["meta"].tolist() == want["meta"].tolist()
    assert got["meta"][0] == (1 if CASES[name][2].get("stepper") == "auto" else 2)   # the device-resident stepper, but for dff4_rails
    assert np.array_equal(got["xf_kept"], want["xf_kept"])
    for k in ("t", "v", "xf"):
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        n = differing(got[k], want[k])
        print("%s: %s %r, %d of %d values differ in their bits" % (name, k, got[k].shape, n, got[k].size))
        assert n == 0, (k, n)
