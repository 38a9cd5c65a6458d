"""The user-facing analyses end to end on the GPU — dc, tran (free steps with sol(t), and a saveat grid), ac, noise, dc_sens and ac_sens
on three small hand-built circuits and once on the GF180 inverter, and the same through a CircuitSweep (3 points; 4 points in 2 groups;
warm start; tran_arrays) — give bit for bit what tests/golden/api_gpu_bits.npz holds, recorded by tests/golden/make_api_bits.py at commit
6f257e7, the parent of the change that split the layer into solution, batch and api modules.  The timing fields of `stats` are left out;
its integer counters are compared.  Cases: tests/api_bits_cases.py."""
import os

import numpy as np
import pytest

from api_bits_cases import GPU_CASES, assert_recorded

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_gpu_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_analyses_give_the_parents_bits(golden, name):
    assert_recorded(GPU_CASES[name](), golden, name)

