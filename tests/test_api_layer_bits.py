"""The user-facing analyses — dc, tran, ac, noise, dc_sens, ac_sens, CircuitSweep and the solution classes — pinned on the CPU against a
stand-in engine (tests/api_bits_cases.py): every call the layer makes on the engine (the trace: options read back out of the ctypes
structs, x0 and its contents, slot ids, values, slot count at construction, small_signal) and every number, retcode, warning and
exception text it hands back are those recorded in tests/golden/api_layer_bits.npz by tests/golden/make_api_bits.py at commit 6f257e7,
the parent of the change that split the layer into solution, batch and api modules."""
import os
import subprocess
import sys

import numpy as np
import pytest

from api_bits_cases import CPU_CASES, assert_recorded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_layer_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_layer_does_what_the_parent_did(golden, name):
    assert_recorded(CPU_CASES[name](), golden, name)


SOLUTION_ALONE = r'''
import importlib, os, sys, types
import numpy as np
pkg = types.ModuleType("cedarsim_jl_amd")          # the package WITHOUT its __init__ (which imports api, and api the GPU binding)
pkg.__path__ = [os.path.join(sys.argv[1], "cedarsim.jl_amd")]
sys.modules["cedarsim_jl_amd"] = pkg
solution = importlib.import_module("cedarsim_jl_amd.solution")
from cedarsim_jl_amd.circuit import Circuit
c = Circuit()
c.V("v1", "vcc", 0, dc=1.0)
c.R("r1", "vcc", "out", 1e3)
c.R("r2", "out", 0, 1e3)
t = np.array([0.0, 1.0, 2.0])
sol = solution.Solution(c, t, {("v", c._n("vcc")): np.ones(3), ("v", c._n("out")): np.array([0.5, 0.5, 0.5])}, None, 0, {})
assert sol(1.5, idxs="node_out") == 0.5 and np.allclose(sol["r1.i"], 0.5e-3) and sol.retcode == "Success"
loaded = sorted(m for m in sys.modules if m.startswith("cedarsim_jl_amd."))
assert not {"cedarsim_jl_amd.engine", "cedarsim_jl_amd.api", "cedarsim_jl_amd.batch"} & set(loaded), loaded
assert "libcedarhip" not in open("/proc/self/maps").read()
print("SOLUTION_HOST_ONLY_OK")
'''


def test_solution_module_is_engine_free():
    # What a result IS needs no GPU binding: the child process imports the solution module's FILE alone (a bare package object whose
    # `__path__` is the source directory, `__init__` not executed, as in test_sweepmap_module_is_host_only), builds a Solution by hand,
    # and then finds neither `engine` in `sys.modules` nor libcedarhip.so mapped.
    r = subprocess.run([sys.executable, "-c", SOLUTION_ALONE, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SOLUTION_HOST_ONLY_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
