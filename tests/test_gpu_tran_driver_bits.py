"""The transient and DC drivers' outputs on the paths tests/test_gpu_lockstep_bits.py does not reach — own steps of a batch and of
blocks, resumed launches, the host stepper with and without a saveat grid, a transient from a given state, the tranop operating
point, DC restarts — are bit for bit those recorded in tests/golden/tran_driver_bits.npz by tests/golden/make_tran_driver_bits.py
at commit 135d2c2, the parent of the change that split the drivers into named steps: t, v, the final state, the DC
solution and statuses, and (stepper, mode, accepted, rejected, Newton iterations, kernel launches).  Cases:
tests/tran_driver_bits_cases.py."""
import os

import numpy as np
import pytest

from tran_driver_bits_cases import CASES, run_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tran_driver_bits.npz")


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
    """count of elements whose bit patterns differ"""
    if a.dtype == np.float64:
        return int(np.count_nonzero(a.view(np.uint64) != b.view(np.uint64)))
    return int(np.count_nonzero(a != b))


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_are_bitwise_those_of_the_parent(E, golden, name):
    got = run_case(E, name)
    want = {k: golden["%s/%s" % (name, k)] for k in got}
    print("%s: meta got %r recorded %r" % (name, got["meta"].tolist(), want["meta"].tolist()))
    assert got["meta"].tolist() == want["meta"].tolist()
    if CASES[name][1] is not None:
        assert tuple(got["meta"][:2]) == CASES[name][1]      # the stepper and the mode the case is about
    else:
        assert got["meta"][1] >= 1                           # restarts ran
    for k in sorted(got):
        if k == "meta":
            continue
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape)
        n = differing(got[k], want[k])
        print("%s: %s %r, %d of %d values differ in their bits" % (name, k, got[k].shape, n, got[k].size))
        assert n == 0, (k, n)
