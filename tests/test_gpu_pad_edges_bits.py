"""The device stepper pads every block to the register-LU size of its kernel inside the solve (csrc/ch_persist.hpp).
The outputs at the edges of that padding — no pad row, one, eleven, three on the NC = 16 kernel, own-steps mode, an all-linear pair,
the full-search fallback, the bordered form that keeps the unpadded images — are bit for bit those recorded in
tests/golden/pad_edges_bits.npz by tests/golden/make_pad_edges_bits.py at commit 89085f2, the parent of the change: t, every observed
row, the final state and (stepper, mode, accepted, rejected, Newton iterations, convergence failures).  Cases: tests/pad_edges_cases.py."""
import os

import numpy as np
import pytest

from pad_edges_cases import CASES, run_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pad_edges_bits.npz")


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
def test_outputs_are_bitwise_those_of_the_unpadded_solve(E, golden, name):
    got = run_case(E, name)
    want = {k: golden["%s/%s" % (name, k)] for k in got}
    print("%s: meta got %r recorded %r" % (name, got["meta"].tolist(), want["meta"].tolist()))
    assert tuple(got["meta"][:2]) == CASES[name][3]          # the device stepper (2) in the mode the case is about: no fall-back
    assert got["meta"].tolist() == want["meta"].tolist()
    for k in sorted(got):
        if k == "meta":
            continue
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape)
        n = differing(got[k], want[k])
        print("%s: %s %r, %d of %d values differ in their bits" % (name, k, got[k].shape, n, got[k].size))
        assert n == 0, (k, n)
