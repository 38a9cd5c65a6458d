"""Host logic: SPICE front-end semantics and the sweep iterators (mirrors test/sweep.jl:71-242,
test/basic.jl:609-684,739-752, test/binning/bins.jl).  CPU only."""
import os

import numpy as np
import pytest

from cedarsim_jl_amd import (NoBinException, ProductSweep, SerialSweep, Sweep, TandemSweep, find_param_ranges, frange,
                             parse_number, parse_spice, parse_spice_file, shard_range, sweepify, sweepvars)
from cedarsim_jl_amd.circuit import CedarError
from cedarsim_jl_amd.workloads import dff_array, gf180_resolver

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_magnitudes():  # src/spectre.jl:402-415, test/basic.jl:609-638
    assert parse_number("1Meg") == 1e6 and parse_number("1meg") == 1e6
    assert parse_number("1Mil") == 25.4e-6
    assert parse_number("0.22u") == 0.22e-6  # exact, not 2.2000000000000001e-7
    assert parse_number("10ns") == 1e-8 and parse_number("3.3333333333333e-10") == 3.3333333333333e-10
    assert parse_number("1k") == 1e3 and parse_number("2.5m") == 2.5e-3 and parse_number("1f") == 1e-15
    assert parse_number("5v") == 5.0 and parse_number("abc") is None


def test_spice_functions_and_if_else():  # test/basic.jl:651-684, :739-752
    nl = parse_spice("""* fn
.param a='int(3.7)' b='nint(2.5)' c='floor(-1.5)' d='ceil(1.2)' e='pow(2,3)' f='ln(exp(2))'
.param sel=1
.if (sel==1)
r1 1 0 'a+b+c+d+e+f'
.else
r1 1 0 1
.endif
v1 1 0 1
""")
    c = nl.build()
    assert abs(c.dev_par[c.dev_names.index("r1")][0] - (3 + 3 - 2 + 2 + 8 + 2)) < 1e-12
    assert abs(nl.build(sel=0).dev_par[0][0] - 1.0) < 1e-12


def test_param_scoping_and_overrides():  # test/sweep.jl:342-371, test/params.jl:90-100
    nl = parse_spice("""* Parameter scoping test
.subckt subcircuit1 vss gnd
.param r_load=1
r1 vss gnd 'r_load'
.ends
.param v_in=1
x1 vss 0 subcircuit1
v1 vss 0 'v_in'
""")
    c = nl.build(**{"v_in": 3.0, "x1.r_load": 7.0})
    assert c.dev_par[c.dev_names.index("x1.r1")][0] == 7.0 and c.sources[0][0] == 3.0
    with pytest.raises(CedarError):
        nl.build(nonexistent=1.0)


def test_binning_find_bin():  # test/binning/bins.jl:19-20
    nl = parse_spice_file(os.path.join(GOLD, "bins_nmos_3p3.cir"))
    assert len(nl.models["nmos_3p3"]) == 16
    assert nl.find_bin("nmos_3p3", 2.8e-7, 2.2e-7)[0] == "nmos_3p3.0"
    assert nl.find_bin("nmos_3p3", 5.0e-7, 2.2e-7)[0] == "nmos_3p3.1"  # half-open ranges
    with pytest.raises(NoBinException):
        nl.find_bin("nmos_3p3", 1e-3, 1e-3)
    # (the file's first line is the SPICE title line, so its m0 device is not part of the circuit)
    text = "* binning\nm0 d1 g s1 b nmos_3p3 W=1e-6 l=1e-6\n" + open(os.path.join(GOLD, "bins_nmos_3p3.cir")).read().split("\n", 1)[1]
    c = parse_spice(text).build()
    assert c.model_names == ["nmos_3p3.5"]
    assert c.models[0][__import__("cedarsim_jl_amd").bsim4_params.PARAM_INDEX["level"]] == 54.0


def test_dff_netlist_matches_generated_workload(gf180):
    nl = parse_spice_file(os.path.join(GOLD, "DFF_cap_all.cir"), lib_resolver=gf180)
    a, b = nl.build(), dff_array(1)
    assert a.gmin == b.gmin == 1e-15 and nl.tran == (3.3333333333333e-10, 6.0e-7)
    assert a.n_nodes == b.n_nodes == 18 and a.n_mna == b.n_mna == 25
    key = lambda c: sorted((c.dev_kind[i], tuple(c.node_names[n] for n in c.dev_node[i]), tuple(np.nan_to_num(c.dev_par[i], nan=-1)))
                           for i in range(len(c.dev_kind)))
    assert key(a) == key(b)
    assert sorted(w.ts for _, w in a.sources if w.ts) == sorted(w.ts for _, w in b.sources if w.ts)


def test_unknown_model_parameter_is_rejected():
    with pytest.raises(CedarError):
        parse_spice("* t\n.model n1 nmos level=54 notaparam=1\nm1 d g 0 0 n1 w=1u l=1u\n").build()


# ---- sweeps (test/sweep.jl:71-242) ----
def test_sweep_algebra():
    s = Sweep("R1", frange(0.1, 0.1, 1.0))
    assert len(s) == 10 and list(s)[0] == (("R1", 0.1),)
    with pytest.raises(ValueError):
        Sweep(R1=[1], R2=[2])
    p = ProductSweep(R1=[1, 2, 3, 4], R2=[10, 20], R3=[5])
    assert p.shape == (4, 2, 1) and len(p) == 8
    pts = list(p)
    assert pts[0] == (("R1", 1), ("R2", 10), ("R3", 5)) and pts[1][0] == ("R1", 2)  # first axis fastest
    t = TandemSweep(R1=[1, 2, 3], R2=[4, 5, 6])
    assert list(t)[2] == (("R1", 3), ("R2", 6))
    with pytest.raises(ValueError):
        TandemSweep(R1=[1, 2], R2=[1])
    ss = SerialSweep(R1=[1, 2], R2=[3])
    assert len(ss) == 3 and dict(list(ss)[0]) == {"R1": 1, "R2": None} and dict(list(ss)[2]) == {"R1": None, "R2": 3}
    assert ProductSweep(R1=[1, 2]) == Sweep("R1", [1, 2])
    assert sweepvars(p, ss) == {"R1", "R2", "R3"}
    sw = sweepify([{"r1": [1, 2], "r2": [1, 2]}, {"r3": [1, 2, 3]}])
    assert len(sw) == 7
    assert find_param_ranges(p) == {"R1": (1, 4, 4), "R2": (10, 20, 2), "R3": (5, 5, 1)}


def test_shard_range_partitions_exactly():
    for n in (1, 7, 8192, 400):
        for w in (1, 2, 3, 8):
            parts = [shard_range(n, r, w) for r in range(w)]
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[i][1] == parts[i + 1][0] for i in range(w - 1))
            assert max(h - l for l, h in parts) - min(h - l for l, h in parts) <= 1


def test_solution_name_map_and_csv(tmp_path):
    """default_name_map (src/util.jl:239-260) and CSV.write(file, sol) (ext/CedarSimCSVExt.jl:13-19) on a Solution
    object built by hand (no GPU needed: the surface is host-side post-processing)."""
    import numpy as np
    from cedarsim_jl_amd import Circuit
    from cedarsim_jl_amd.api import Solution
    c = Circuit()
    c.V("v1", "vcc", 0, dc=1.0)
    c.R("r1", "vcc", "out", 1e3)
    c.R("r2", "out", 0, 1e3)
    t = np.array([0.0, 1.0, 2.0])
    cols = {("v", c._n("vcc")): np.ones(3), ("v", c._n("out")): np.array([0.5, 0.5, 0.5])}
    sol = Solution(c, t, cols, None, 0, {})
    assert sol.default_name_map() == {"node_vcc": "vcc", "node_out": "out"}
    p = sol.write_csv(str(tmp_path / "sol.csv"))
    rows = open(p).read().strip().splitlines()
    assert rows[0] == "t,vcc,out" and rows[1] == "0.0,1.0,0.5" and len(rows) == 4
    assert sol(1.5, idxs="node_out") == 0.5 and np.allclose(sol["r1.i"], 0.5e-3)


def test_spectre_model_card_parser():
    """`model <name> <master> key=value …` with `+` continuations and `//` comments (the card format of the ASAP7 file the
    reference's parser tests hold)."""
    from cedarsim_jl_amd import parse_spectre_models
    m = parse_spectre_models("""// header
simulator lang=spectre
model nmos_x bsimcmg type=n LEVEL = 110
//+version=110
+  bulkmod = 1   eot = 1e-009  // trailing comment
+  phig=4.3  l = 21n
model pmos_x bsimcmg type=p
+ phig = 4.8
resistor1 (a b) resistor r=1k
""")
    assert set(m) == {"nmos_x", "pmos_x"}
    assert m["nmos_x"][0] == "bsimcmg" and m["nmos_x"][1] == {"type": "n", "level": 110.0, "bulkmod": 1.0, "eot": 1e-9, "phig": 4.3, "l": 2.1e-8}
    assert m["pmos_x"][1] == {"type": "p", "phig": 4.8}


def test_solution_call_interpolates_with_pchip():
    import numpy as np
    from cedarsim_jl_amd import Circuit
    from cedarsim_jl_amd.api import Solution
    c = Circuit()
    c.V("v1", "a", 0, dc=1.0)
    c.R("r1", "a", 0, 1.0)
    t = np.sort(np.concatenate(([0.0, 1.0], np.random.default_rng(0).uniform(0, 1, 60))))
    t = np.insert(t, 20, t[20])                          # a repeated time, as after a break-point restart
    sol = Solution(c, t, {("v", c._n("a")): np.sin(6 * t)}, None, 0, {})
    tq = np.linspace(0.01, 0.99, 200)
    err = np.abs(sol(tq, idxs="node_a") - np.sin(6 * tq)).max()
    lin = np.abs(np.interp(tq, t, np.sin(6 * t)) - np.sin(6 * tq)).max()
    assert err < 6e-3 and err < 0.6 * lin
    assert isinstance(sol(0.5, idxs="node_a"), float) and len(sol(0.5, idxs=["node_a"])) == 1


def test_sweep_batch_learns_the_parameter_map_from_few_builds():
    """CircuitSweep._batch (the host half of `remake(prob, p=sim)` over a sweep, src/sweeps.jl:471-482): a product sweep whose
    variables act on disjoint table entries is assembled from a handful of builds (the base point, two per axis for the
    identity / affine map, up to four validation points plus the two extremes of every fitted variable: at most 13 for the
    reference's 400-point sweep, test/sweep.jl:326-340),
    a sweep with a coupled entry falls back to one build per point, and both give the per-point tables exactly."""
    import numpy as np
    from cedarsim_jl_amd import Circuit, CircuitSweep, ProductSweep, TandemSweep, frange
    count = {"n": 0}

    def two_resistor(R1=100.0, R2=100.0):
        count["n"] += 1
        c = Circuit()
        c.V("V", "vcc", 0, dc=1.0)
        c.R("R1", "vcc", "mid", R1)
        c.R("R2", "mid", 0, R2)
        return c

    cs = CircuitSweep(two_resistor, ProductSweep(R1=frange(100.0, 100.0, 2000.0), R2=frange(100.0, 100.0, 2000.0)))
    base, ids, vals = cs._batch(0, 400)
    assert count["n"] <= 13 and vals.shape == (2, 400) and len(base.slots) == 2 and cs.setup["circuit_builds"] == count["n"]
    r1 = [p["R1"] for p in cs]
    r2 = [p["R2"] for p in cs]
    by_slot = {s[1]: vals[i] for i, s in enumerate(base.slots)}
    assert np.array_equal(by_slot[base.dev_names.index("r1")], r1) and np.array_equal(by_slot[base.dev_names.index("r2")], r2)

    def coupled(a=1.0, b=1.0):   # one resistor answers to both variables: not separable
        count["n"] += 1
        c = Circuit()
        c.V("V", "vcc", 0, dc=1.0)
        c.R("R", "vcc", 0, a * b)
        return c

    count["n"] = 0
    cs2 = CircuitSweep(coupled, ProductSweep(a=[1.0, 2.0, 3.0, 4.0], b=[1.0, 10.0, 100.0, 1000.0]))
    base2, _, vals2 = cs2._batch(0, 16)
    assert vals2.shape == (1, 16) and np.array_equal(vals2[0], [p["a"] * p["b"] for p in cs2])
    assert count["n"] > 16   # the separable attempt was abandoned, then one build per point
    count["n"] = 0
    cs3 = CircuitSweep(two_resistor, TandemSweep(R1=[1.0, 2.0, 3.0], R2=[4.0, 5.0, 6.0]))   # zipped: as many values as points
    base3, _, vals3 = cs3._batch(0, 3)
    assert count["n"] == 3 and vals3.shape == (2, 3)


def test_sweep_batch_is_validated_against_full_builds():
    """a dependence that vanishes at the base point is invisible to single-axis builds around it —
    R = 1e3 + a*b with a base of a = 0, or a conditional.  The assembled table is checked against full builds of the far
    corner and of seeded random points, and any mismatch falls back to one build per point."""
    from cedarsim_jl_amd import Circuit, CircuitSweep

    def make(f):
        def build(**kw):
            c = Circuit()
            c.V("V", "vcc", 0, dc=1.0)
            c.R("R", "vcc", 0, f(**kw))
            return c
        return build

    cs = CircuitSweep(make(lambda a=0.0, b=1.0: 1e3 + a * b), ProductSweep(a=[0.0, 1.0, 2.0], b=[1.0, 2.0, 3.0]))
    _, _, vals = cs._batch(0, 9)
    assert np.array_equal(vals[0], [1e3 + p["a"] * p["b"] for p in cs]) and cs.setup["how"] == "one build per point"
    # conditional: the entry follows `a` only in mode 1, and the base point is in mode 0
    cs = CircuitSweep(make(lambda mode=0, a=1.0: (a if mode else 50.0)), ProductSweep(mode=[0, 1], a=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]))
    _, _, vals = cs._batch(0, 12)
    assert np.array_equal(vals[0], [(p["a"] if p["mode"] else 50.0) for p in cs])
    # a map that is not affine in its variable (1/g): one build per distinct value, still exact
    gs = [1e-3 * (i + 1) for i in range(12)]
    cs = CircuitSweep(make(lambda g=1e-3, k=1.0: 1.0 / g), ProductSweep(g=gs, k=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]))
    _, _, vals = cs._batch(0, 72)
    assert np.array_equal(vals[0], [1.0 / p["g"] for p in cs]) and cs.setup["circuit_builds"] < 72


def test_sweep_batch_catches_clipped_and_gated_entries():
    """What scripts/extended_fuzz_sweepmap.py found (2 of 1 500 random builders, silently wrong values): an entry that is affine on the
    three fitted values of its variable and clipped beyond them, and an entry that follows one variable only while another is above a
    threshold.  The validation now includes, for every fitted variable, the points that hold its extremes with the most other
    variables away from the base point."""
    from cedarsim_jl_amd import Circuit, CircuitSweep

    def build(a=2.2, b=2.9):
        c = Circuit()
        c.V("V", "vcc", 0, dc=1.0)
        c.R("R1", "vcc", "mid", a)
        c.R("R2", "mid", 0, max(b, 2.0) * 1.8)          # clipped below b = 2
        c.R("R3", "mid", 0, b if a > 2.0 else 50.0)      # gated by the other variable
        return c
    rng = np.random.default_rng(36)
    npts = 32
    cs = CircuitSweep(build, TandemSweep(a=[float(x) for x in rng.uniform(0.5, 4.0, npts)], b=[float(x) for x in rng.uniform(0.5, 4.0, npts)]))
    base, ids, vals = cs._batch(0, npts)
    for r in range(npts):
        c = build(**cs.points[r])
        for i, sl in enumerate(base.slots):
            assert vals[i][r] == c.dev_par[sl[1]][sl[2]], (r, sl, cs.setup["how"])
    cs = CircuitSweep(build, ProductSweep(a=[0.855, 1.504, 1.971, 1.894, 3.994, 1.111], b=[1.778, 3.762, 3.168, 2.994, 1.996]))
    base, ids, vals = cs._batch(0, 30)
    for r in range(30):
        c = build(**cs.points[r])
        for i, sl in enumerate(base.slots):
            assert vals[i][r] == c.dev_par[sl[1]][sl[2]], (r, sl, cs.setup["how"])


def test_monte_carlo_tandem_sweep_needs_a_handful_of_builds():
    """process-variation samples enter as an explicit TandemSweep (src/sweeps.jl:278-290) with as many
    distinct values as points.  The name -> table-entry map is learned from three builds per variable (identity /
    proportional / affine), not one per point; the table equals the per-point builds bit for bit."""
    from cedarsim_jl_amd import CircuitSweep
    from cedarsim_jl_amd import bsim4_params as B4
    from cedarsim_jl_amd.workloads import dff_mc_builder, mc_tandem_sweep
    S = 256
    build, names = dff_mc_builder()
    cs = CircuitSweep(build, mc_tandem_sweep(S))
    base, ids, vals = cs._batch(0, S)
    assert cs.setup["circuit_builds"] <= 1 + 4 * len(names) + 4 and vals.shape[1] == S and cs.setup["how"].startswith("learned")
    assert len(base.slots) == 6 + 2 * 30   # six card entries, W and L of the thirty MOSFETs
    for r in (1, 17, 200, S - 1):   # against the per-point build
        c = build(**cs.points[r])
        for i, sl in enumerate(base.slots):
            if sl[0] == 2:     # SLOT_MODEL_PAR: proportional map, the builder's own product
                assert vals[i, r] == c.models[sl[1]][sl[2]]
            else:              # SLOT_DEV_PAR (W + dw, L + dl): affine map, equal to rounding
                assert sl[0] == 1 and abs(vals[i, r] - c.dev_par[sl[1]][sl[2]]) <= 1e-13 * abs(vals[i, r])


def test_sweep_map_reproduces_the_recorded_trace_of_300_random_builders():
    """tests/golden/sweepmap_trace.json holds, for seeds 0..299 of sweepmap_cases.random_case, what `CircuitSweep._batch` did
    before the learner moved to sweepmap.py (tests/golden/make_sweepmap_trace.py): which way it went, how many circuits it
    built, the slots, and a digest of the float64 value table.  The moved code must do exactly that — same builds, same bits —
    and, independently of the trace, every slotted entry must equal the per-point build and every other `dev_par` entry the base
    build's (the check of scripts/extended_fuzz_sweepmap.py)."""
    import hashlib
    import json
    from cedarsim_jl_amd import CircuitSweep
    from sweepmap_cases import random_case, table_mismatch
    trace = json.load(open(os.path.join(GOLD, "sweepmap_trace.json")))
    assert len(trace) == 300 and sum(row["how"] == "learned map" for row in trace) >= 50   # not a test of the fall-back alone
    for seed, want in enumerate(trace):
        build, sweep = random_case(seed)
        cs = CircuitSweep(build, sweep)
        base, ids, vals = cs._batch(0, len(cs.points))
        got = {"how": cs.setup["how"].split(" (")[0], "circuit_builds": cs.setup["circuit_builds"],
               "slots": [[int(x) for x in s] for s in base.slots],
               "vals_sha256_16": hashlib.sha256(np.ascontiguousarray(vals, np.float64).tobytes()).hexdigest()[:16]}
        assert got == want, seed
        assert ids == list(range(len(base.slots))) and vals.dtype == np.float64 and vals.shape == (len(base.slots), len(cs.points))
        assert table_mismatch(build, cs.points, base, vals) is None, seed


SWEEPMAP_ALONE = r'''
import importlib, os, sys, types
pkg = types.ModuleType("cedarsim_jl_amd")          # the package WITHOUT its __init__ (which imports api, and api the GPU binding):
pkg.__path__ = [os.path.join(sys.argv[1], "cedarsim.jl_amd")]   # submodules load from their files, each with its own imports only
sys.modules["cedarsim_jl_amd"] = pkg
sweepmap = importlib.import_module("cedarsim_jl_amd.sweepmap")
from cedarsim_jl_amd.circuit import Circuit
from cedarsim_jl_amd.sweeps import ProductSweep, frange


def two_resistor(R1=100.0, R2=100.0):
    c = Circuit()
    c.V("V", "vcc", 0, dc=1.0)
    c.R("R1", "vcc", "mid", R1)
    c.R("R2", "mid", 0, R2)
    return c


points = [dict(p) for p in ProductSweep(R1=frange(100.0, 100.0, 2000.0), R2=frange(100.0, 100.0, 2000.0))]
base, ids, vals, setup = sweepmap.learn_batch(two_resistor, points)
assert setup["how"].startswith("learned map") and setup["circuit_builds"] <= 13 and vals.shape == (2, 400), setup
assert [vals[i][399] for i in ids] == [2000.0, 2000.0] and len(base.slots) == 2
assert "cedarsim_jl_amd.engine" not in sys.modules and "cedarsim_jl_amd.api" not in sys.modules, sorted(m for m in sys.modules if "cedar" in m)
assert "libcedarhip" not in open("/proc/self/maps").read()
print("SWEEPMAP_HOST_ONLY_OK")
'''


def test_sweepmap_module_is_host_only():
    # The learner runs without the GPU binding.  The package `__init__` imports `api`, and `api` imports `engine`, so a plain
    # `import cedarsim_jl_amd.sweepmap` always brings the binding along; the child process therefore imports the module FILE
    # directly (a bare package object whose `__path__` is the source directory, `__init__` not executed), runs `learn_batch` on
    # the two-resistor product sweep, and then finds neither `engine` in `sys.modules` nor libcedarhip.so mapped.
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", SWEEPMAP_ALONE, root], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SWEEPMAP_HOST_ONLY_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
