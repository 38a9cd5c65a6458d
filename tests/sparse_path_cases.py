"""Cases of the sparse path (path 2: ch_engine_sparse.hpp, ch_sparse.hpp), shared by tests/golden/make_sparse_path_trace.py, which
records what the commit BEFORE the host side of the path was reorganised computes on the GPU, and tests/test_gpu_sparse_trace.py,
which holds the reorganised host side to that record — bit for bit: the kernels and the launch order are the same and every sum on
this path has a fixed order.

`CASES`: name -> (environment switches set around the engine, function(EngineCircuit) -> list of runs).  A run is what `dc_run` /
`tran_run` return: return code, `info()`, every integer field of the stats (no times), and the numbers as `float.hex` strings."""
import os

import numpy as np

from cedarsim_jl_amd import dc_opts, tran_opts
from cedarsim_jl_amd.workloads import dff_array, dff_chain, rc_ladder

INFO_FIELDS = ("path", "n_unknowns", "nnz_jac", "nnz_lu")


def _hex(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def _ints(st):
    return {k: int(v) for k, v in st.items() if isinstance(v, int)}


def _info(e):
    i = e.info()
    return {k: int(i[k]) for k in INFO_FIELDS}


def dc_run(e, opts):
    rc, x, status, st = e.dc(opts)
    return {"kind": "dc", "rc": int(rc), "status": [int(s) for s in status], "info": _info(e), "stats": _ints(st), "x": _hex(x)}


def tran_run(e, t0, t1, opts):
    rc, t, v, xf, st = e.tran(t0, t1, opts)
    return {"kind": "tran", "rc": int(rc), "info": _info(e), "stats": _ints(st), "shape": list(v.shape), "t": _hex(t), "v": _hex(v)}


def hub_ladder(n=4200, n_spokes=300):
    """A linear RC ladder of n nodes with one hub node tied to n_spokes of them by resistors: n >= 4096 takes the two-stage O(n)
    passes, the hub is a CSR row of more than 256 entries and its diagonal a gather item of more than SP_ASM_HEAVY sources."""
    c = rc_ladder(n)
    step = n // n_spokes
    for k in range(n_spokes):
        c.R("rh%d" % k, "hub", "n%d" % (1 + k * step), 5e3 * (1.0 + 0.01 * (k % 11)))
    c.C("chub", "hub", 0, 2e-12)
    c.observe_node("hub")
    return c


def _ladder(E):
    e = E(rc_ladder(40))
    return [dc_run(e, dc_opts(abstol=1e-12)),
            tran_run(e, 0.0, 2e-8, tran_opts(abstol=1e-7, reltol=1e-6, saveat=np.linspace(0.0, 2e-8, 21)))]


def _ladder_batch(E):
    """Three samples with their own r0, c0, r20 and c20, one of them far stiffer (a section a thousand times faster than its neighbours), so
    that the samples leave the active list of a solve at different iterations."""
    c = rc_ladder(40)
    slots = [c.slot("r0", "r"), c.slot("c0", "c"), c.slot("r20", "r"), c.slot("c20", "c")]
    e = E(c)
    e.set_samples(3)
    e.set_params(slots, [np.array([1e3, 2.5e3, 1.0]), np.array([1e-12, 3e-12, 1e-15]), np.array([1e3, 4e2, 1e6]), np.array([1e-12, 5e-13, 1e-15])])
    return [dc_run(e, dc_opts(abstol=1e-12)),
            tran_run(e, 0.0, 2e-8, tran_opts(abstol=1e-7, reltol=1e-6, saveat=np.linspace(0.0, 2e-8, 21)))]


def _chain(stages):
    """Operating point from the cold start (voltage limiting, restart passes) and a short transient.  Six stages: no pass of the
    cold start converges on this path (return code -3 after every restart has run to maxit, and the transient ends in its operating
    point) — recorded as it is; eight stages converge and step."""
    def run(E):
        e = E(dff_chain(stages))
        return [dc_run(e, dc_opts()),
                tran_run(e, 0.0, 5e-8, tran_opts(abstol=1e-4, reltol=1e-4, saveat=np.linspace(0.0, 5e-8, 11)))]
    return run


def _array(tiles, t1):
    def run(E):
        c = dff_array(tiles, observe="q", supply_r=1.0)
        for n in ("vdd", "vss"):
            c.observe_node(n)
        e = E(c)
        return [dc_run(e, dc_opts(abstol=1e-12)),
                tran_run(e, 0.0, t1, tran_opts(abstol=1e-4, reltol=1e-4, saveat=np.linspace(0.0, t1, 13), dc=dc_opts(abstol=1e-12)))]
    return run


def _hub(E):
    e = E(hub_ladder())
    return [dc_run(e, dc_opts(abstol=1e-12)),
            tran_run(e, 0.0, 4e-9, tran_opts(abstol=1e-7, reltol=1e-6, saveat=np.linspace(0.0, 4e-9, 9)))]


SPARSE = {"CEDARHIP_FORCE_SPARSE": "1"}
NO_TEAR = {"CEDARHIP_NO_TEAR": "1"}
NO_SUBTREE = {"CEDARHIP_NO_TEAR": "1", "CEDARHIP_SPARSE_NO_SUBTREE": "1"}
CASES = {
    "ladder40": (SPARSE, _ladder),                        # one-workgroup LU, small-system passes
    "ladder40_batch3": (SPARSE, _ladder_batch),
    "dff_chain6": ({}, _chain(6)),
    "dff_chain8": ({}, _chain(8)),
    "dff_array12": (NO_TEAR, _array(12, 6e-8)),
    "dff_array12_no_subtree": (NO_SUBTREE, _array(12, 6e-8)),
    # twelve tiles are fewer groups than the subtree form asks for (64): the same pair at the smallest size that has it
    "dff_array70_subtree": (NO_TEAR, _array(70, 2e-8)),
    "dff_array70_levels": (NO_SUBTREE, _array(70, 2e-8)),
    "hub_ladder4200": (SPARSE, _hub),                     # two-stage passes, heavy CSR row, heavy gather items
}


def run_case(E, name):
    """The runs of one case, with its environment switches set around the engine and restored afterwards."""
    env, fn = CASES[name]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn(E)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
