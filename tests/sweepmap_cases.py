"""Random builders and sweeps for the sweep-map learner (cedarsim_jl_amd.sweepmap), shared by test_netlist_and_sweeps.py,
tests/golden/make_sweepmap_trace.py and scripts/extended_fuzz_sweepmap.py.  A plain helper module: no fixtures, no test collection.

A case is a three-device divider whose resistor / capacitor values are random expressions of up to three sweep variables (constant,
identity, proportional, affine, product, sum, reciprocal, square, conditional, clipped) under a product or a tandem sweep.  The
order of the RNG draws is fixed: a seed number names the same case everywhere, tests/golden/sweepmap_trace.json included."""
import numpy as np

from cedarsim_jl_amd import Circuit, ProductSweep, TandemSweep


def random_case(seed):
    """(build, sweep) of case `seed`: `build(**point) -> Circuit`, and the sweep to hand to `CircuitSweep(build, sweep)`."""
    rng = np.random.default_rng(seed)
    nvar = int(rng.integers(1, 4))
    vnames = ["a", "b", "m"][:nvar]

    def expr():
        kind = rng.integers(0, 10)
        v = vnames[rng.integers(nvar)]
        w = vnames[rng.integers(nvar)]
        k, a0 = float(rng.uniform(0.5, 3.0)), float(rng.uniform(10.0, 1e3))
        if kind == 0: return lambda p: a0
        if kind == 1: return lambda p: p[v]
        if kind == 2: return lambda p: k * p[v]
        if kind == 3: return lambda p: a0 + k * p[v]
        if kind == 4: return lambda p: (p[v] * p[w]) if v != w else p[v] * p[v]
        if kind == 5: return lambda p: a0 + p[v] + p[w]
        if kind == 6: return lambda p: 1e4 / p[v]
        if kind == 7: return lambda p: a0 + p[v] ** 2
        if kind == 8: return lambda p: (p[v] if p[w] > 2.0 else a0)
        return lambda p: max(p[v], 2.0) * k
    exprs = [expr() for _ in range(3)]
    defaults = {n: float(rng.uniform(1.0, 4.0)) for n in vnames}

    def build(**kw):
        p = dict(defaults); p.update(kw)
        c = Circuit()
        c.V("V", "vcc", 0, dc=1.0)
        c.R("R1", "vcc", "mid", 1.0 + abs(exprs[0](p)))
        c.R("R2", "mid", 0, 1.0 + abs(exprs[1](p)))
        c.C("C1", "mid", 0, 1e-12 * (1.0 + abs(exprs[2](p))))
        return c
    if rng.random() < 0.5:
        sweep = ProductSweep(**{n: [float(x) for x in np.round(rng.uniform(0.5, 4.0, int(rng.integers(2, 7))), 3)] for n in vnames})
    else:
        npts = int(rng.integers(5, 60))
        sweep = TandemSweep(**{n: [float(x) for x in rng.uniform(0.5, 4.0, npts)] for n in vnames})
    return build, sweep


def table_mismatch(build, points, base, vals):
    """First disagreement between a learned table and one build per point, or None: every slotted entry must equal the per-point
    build (to rounding of an affine fit), every `dev_par` entry that is not a slot must equal the base build's."""
    slotted = {tuple(s) for s in base.slots}
    for r, point in enumerate(points):
        c = build(**point)
        for i, sl in enumerate(base.slots):
            want, got = c.dev_par[sl[1]][sl[2]], vals[i][r]
            if not (got == want or abs(got - want) <= 1e-12 * abs(want)):
                return (r, tuple(sl), got, want)
        for d, row in enumerate(c.dev_par):
            for j, x in enumerate(row):
                y = base.dev_par[d][j]
                if (1, d, j) not in slotted and not (x == y or (x != x and y != y)):
                    return (r, "unslotted entry differs", d, j, x, y)
    return None
