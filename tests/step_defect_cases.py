"""Circuits and run options of the step-defect tests (tests/test_step_defect_reference.py on the CPU oracle,
tests/test_gpu_step_defect.py on the engine), and `dense_mesh`, which tests/test_gpu_parity.py shares.  HIP-free; no test collection.

Every transient case is a LINEAR circuit with continuous sources (SIN, PULSE with finite edges, PWL), run without `saveat` so that
every accepted step is a row, at deliberately loose tolerances with a `dtmax` of about an eighth of the fastest source period: the
corrections are then the size of the signals, and a linear solve wrong by a relative eps shows as eps, not as eps times a
tolerance-sized correction."""
import numpy as np

from cedarsim_jl_amd import PWL, SIN, Circuit
from cedarsim_jl_amd.circuit import DEV_V
from cedarsim_jl_amd.workloads import rc_ladder

LOOSE = dict(abstol=1e-1, reltol=1e-1)


def dense_mesh(n_nodes, rng, n_cg=None, n_mos=None, reach=None):
    """Every pair of nodes joined by a resistor, every node with a capacitor to ground, a handful of MOSFETs and a PWL
    supply behind a resistor: ONE block of n_nodes unknowns whose gather lists are as long as the block size allows.
    reach: join only nodes at most `reach` apart in the numbering, and those half the mesh apart (None: every pair)."""
    from cedarsim_jl_amd.workloads import gf180_models
    c = Circuit(gmin=1e-12)
    m = gf180_models()
    mn, mp = c.add_model(*m["nfet_06v0"]), c.add_model(*m["pfet_06v0"])
    names = ["n%d" % i for i in range(1, n_nodes + 1)]
    c.V("vdd", "vdd", 0, dc=5.0, tran=PWL([0.0, 5.0, 2e-7, 2.0, 5e-7, 2.0, 6e-7, 5.0, 1.0, 5.0]))
    for i, a in enumerate(names):
        c.R("rs%d" % i, "vdd" if i % 3 == 0 else 0, a, float(10 ** rng.uniform(3, 4)))
        if n_cg is None or i < n_cg:
            c.C("cg%d" % i, a, 0, float(10 ** rng.uniform(-13, -12)))
        for j in range(i + 1, n_nodes):
            if reach is None or j - i <= reach or j - i == n_nodes // 2:
                c.R("r%d_%d" % (i, j), a, names[j], float(10 ** rng.uniform(3, 5)))
    for k in range(min(6, n_nodes // 2) if n_mos is None else n_mos):
        d, g, s = names[(3 * k) % n_nodes], names[(3 * k + 1) % n_nodes], names[(3 * k + 2) % n_nodes]
        if k % 2 == 0:
            c.M("mn%d" % k, d, g, s, 0, mn, 1e-6, 6e-7)
        else:
            c.M("mp%d" % k, d, g, s, "vdd", mp, 1e-6, 6e-7)
    c.observe_all_nodes()
    return c


def set_wave(c, name, dc, wave):
    c.sources[c.dev_ipar[c.dev_names.index(name)][0]] = (float(dc), wave)


def mesh_shape(n):
    """dict(reach, n_cg) of a mesh of n unknowns that stays on the fused path.  The fused kernel keeps, per block, one stamp record
    of 41 doubles per device and 2 n^2 + 13 n doubles of matrices and vectors in LDS, and a block that needs more than 150 KB takes
    the sparse path whatever its size: the full mesh (n (n + 3) / 2 devices) does from about 28 unknowns on.  A mesh that does not
    fit is thinned to the devices a 135 KB budget holds: links within `reach`, one link per node across half the mesh (fill-in
    over the whole matrix) and, where even that is too much, capacitors on a quarter of the nodes only.  Above 64 unknowns
    (sparse path in any case) the mesh is full again."""
    budget = (135000 - 8 * (2 * n * n + 13 * n)) // 340
    if n > 64 or n * (n + 3) // 2 <= budget:
        return dict(reach=None, n_cg=None)
    far = n // 2 + 1
    n_cg = n if budget - 2 * n - far >= n else max(1, n // 4)
    return dict(reach=max(1, (budget - n - n_cg - far) // n), n_cg=n_cg)


def linear_mesh(n):
    """`dense_mesh` without its MOSFETs, its supply a sine of period 200 ns around 3.5 V: one linear block of n unknowns."""
    c = dense_mesh(n, np.random.default_rng(1000 + n), n_mos=0, **mesh_shape(n))
    set_wave(c, "vdd", 3.5, SIN(3.5, 1.5, 5e6))
    return c


def mixed_linear():
    """Two RC poles, an inductor branch, a VCCS stage, a VCVS stage and a floating source (the two_pole circuit of
    tests/test_gpu_tran_sens.py and two more stages): every linear element kind, three kept branch currents."""
    c = Circuit(gmin=1e-9)
    c.V("v1", "in", 0, dc=0.5, tran=SIN(0.5, 0.4, 5e5))
    c.R("r1", "in", "a", 1e3)
    c.C("c1", "a", 0, 2e-10)
    c.R("r2", "a", "b", 2e3)
    c.C("c2", "b", 0, 1e-10)
    c.L("l1", "b", "d", 1e-4)
    c.R("r3", "d", 0, 5e2)
    c.G("g1", "e", 0, "a", 0, gain=1e-3)
    c.R("r4", "e", 0, 1e3)
    c.C("c3", "e", 0, 1e-10)
    c.E("e1", "f", 0, "b", 0, gain=2.0)
    c.R("r5", "f", "g", 1e3)
    c.C("c4", "g", 0, 1e-10)
    c.V("vf", "g", "h", dc=0.3, tran=SIN(0.3, 0.2, 1e6))
    c.R("r6", "h", 0, 2e3)
    c.observe_all_nodes()
    for b in ("l1", "e1", "vf"):
        c.observe_branch(b)
    return c


def lockstep_blocks(size, n_blocks):
    """n_blocks independent blocks of `size` unknowns, structurally identical and differently valued, each behind its own grounded
    sine source: a resistor chain with a capacitor on every node, a resistor across every third pair of next-but-one nodes (fill-in)
    and a VCCS from the first node onto the last (an unsymmetric matrix)."""
    c = Circuit()
    for k in range(n_blocks):
        f = 1.0 + 0.07 * k
        nm = lambda i, k=k: "in%d" % k if i == 0 else "b%d_%d" % (k, i)   # noqa: E731
        c.V("v%d" % k, nm(0), 0, dc=0.5, tran=SIN(0.5, 0.4 / f, 2e7))
        for i in range(1, size + 1):
            c.R("r%d_%d" % (k, i), nm(i - 1), nm(i), 1e3 * f * (1.0 + 0.03 * ((5 * i) % 7)))
            c.C("c%d_%d" % (k, i), nm(i), 0, 1e-12 / f * (1.0 + 0.05 * ((3 * i) % 5)))
        for i in range(1, size - 1, 3):
            c.R("x%d_%d" % (k, i), nm(i), nm(i + 2), 3e3 * f)
        if size > 1:
            c.G("g%d" % k, nm(size), 0, nm(1), 0, gain=2e-4 * f)
    c.observe_all_nodes()
    return c


def observe_all(c):
    c.observe_all_nodes()
    return c


def sine_tiles(n):
    """`rc_tiles(n)` of tests/test_gpu_torn.py (n RC tiles on one rail behind a resistor: torn at the rail, a border of one unknown)
    with every node observed and the rail's source a 100 MHz sine around 0.5 V: every step moves every tile, and the operating
    point is not zero."""
    from test_gpu_torn import rc_tiles
    c = observe_all(rc_tiles(n))
    set_wave(c, "vs", 0.5, SIN(0.5, 0.5, 1e8))
    return c


def two_rail_tiles(n):
    """n tiles between a `vdd` rail and a `vss` rail, each rail behind its own resistor and sine source: every tile a resistor from
    vdd to its node and a capacitor and a leak resistor from there to vss.  Torn at the rails: a border of two unknowns; the
    operating point is not zero (0.8 V above, 0.1 V below, the leaks carry current)."""
    c = Circuit()
    c.V("vhi", "hsrc", 0, dc=0.8, tran=SIN(0.8, 0.3, 1e8))
    c.R("rhi", "hsrc", "vdd", 20.0)
    c.C("chi", "vdd", 0, 5e-13)
    c.V("vlo", "lsrc", 0, dc=0.1, tran=SIN(0.1, 0.05, 2.5e7))
    c.R("rlo", "lsrc", "vss", 30.0)
    c.C("clo", "vss", 0, 4e-13)
    for i in range(n):
        c.R("r%d" % i, "vdd", "a%d" % i, 1e3 * (1.0 + 0.01 * i))
        c.C("c%d" % i, "a%d" % i, "vss", 1e-12 * (1.0 + 0.02 * (i % 7)))
        c.R("k%d" % i, "a%d" % i, "vss", 2e4 * (1.0 + 0.03 * (i % 5)))
    return observe_all(c)


def hub_ladder(n, n_spokes):
    """`hub_ladder` of tests/sparse_path_cases.py with every node observed."""
    c = rc_ladder(n)
    step = n // n_spokes
    for k in range(n_spokes):
        c.R("rh%d" % k, "hub", "n%d" % (1 + k * step), 5e3 * (1.0 + 0.01 * (k % 11)))
    c.C("chub", "hub", 0, 2e-12)
    return observe_all(c)


def hub_ladder_matrices(n, n_spokes, r=1e3, cap=1e-12, vstep=1.0, trise=1e-9):
    """G, C (scipy.sparse, full MNA: nodes n0 .. n_n, hub, then the source's branch) and s(t) of `hub_ladder(n, n_spokes)`, written
    down by hand: the oracle's dense evaluation does not scale to 4200 unknowns.  Held to `linear_parts` at n = 40 on the CPU."""
    import scipy.sparse as sp
    N = n + 3
    hub, br = n + 1, n + 2
    i, j, v = [], [], []

    def cond(a, b, g):
        i.extend([a, b, a, b]); j.extend([a, b, b, a]); v.extend([g, g, -g, -g])   # noqa: E702

    for k in range(n):
        cond(k, k + 1, 1.0 / r)
    step = n // n_spokes
    for k in range(n_spokes):
        cond(hub, 1 + k * step, 1.0 / (5e3 * (1.0 + 0.01 * (k % 11))))
    # the source: its current leaves node n0 through the branch unknown; its row is v(n0) = V(t)
    i.extend([0, br]); j.extend([br, 0]); v.extend([1.0, 1.0])   # noqa: E702
    G = sp.csr_matrix((v, (i, j)), shape=(N, N))
    cd = np.zeros(N)
    cd[1:n + 1] = cap
    cd[hub] = 2e-12
    C = sp.diags(cd).tocsr()

    def s(t, mode=1):
        out = np.zeros(N)
        out[br] = vstep * min(max(t / trise, 0.0), 1.0) if mode else 0.0
        return out
    return G, C, s


def obs_mna(c):
    """MNA index of every observable, in the order of the result rows."""
    return [o[1] - 1 if o[0] == "v" else c.mna_index("i", c.dev_names[o[1]]) for o in c.obs]


def rows_to_mna(c, v):
    """Result rows v[n_obs][nt] -> X[nt][n_mna], NaN where an MNA entry is not observed."""
    X = np.full((v.shape[1], c.n_mna), np.nan)
    X[:, obs_mna(c)] = np.asarray(v).T
    return X


def unknown_columns(c):
    """MNA columns of the excitation condition: every observed entry but the nodes a voltage source ties to ground (the engine
    holds those as known values, not as unknowns)."""
    known = set()
    for k, kind in enumerate(c.dev_kind):
        if kind == DEV_V:
            a, b = c.dev_node[k][0], c.dev_node[k][1]
            if a == 0 or b == 0:
                known.add(max(a, b) - 1)
    return np.array([m for m in obs_mna(c) if m not in known], int)


SPARSE = {"CEDARHIP_FORCE_SPARSE": "1"}
NO_TEAR = {"CEDARHIP_NO_TEAR": "1"}
NO_SUBTREE = {"CEDARHIP_NO_TEAR": "1", "CEDARHIP_SPARSE_NO_SUBTREE": "1"}
NOPAIR = {"CEDARHIP_PERSIST_NOPAIR": "1"}
MESH_SIZES = (1, 7, 8, 9, 12, 13, 16, 17, 32, 33, 40, 64)
HOST, DEVICE = 1, 2
LOCKSTEP, BORDERED = 1, 3


def _case(build, span, dtmax, path, stepper, mode, env=None, force=None, **tol):
    """One transient case: circuit builder, (t0, t1), dtmax, the path / stepper / stepper mode that must have run, the environment
    switches around the engine, the `stepper` option (None: the engine's choice) and the tolerances (default LOOSE)."""
    kw = dict(LOOSE)
    kw.update(tol)
    return dict(build=build, span=span, dtmax=dtmax, path=path, stepper=stepper, mode=mode, env=env or {}, force=force, tol=kw)


# name -> case.  The sizes are the smallest at which each solver is a different piece of code.
TRAN_CASES = {}
for _n in MESH_SIZES:        # fused kernel on the host stepper: both sides of every lu_variant edge (8 / 12 / 16 / 32, LDS above) and the cap of 64
    TRAN_CASES["mesh%d" % _n] = _case(lambda n=_n: linear_mesh(n), (0.0, 4e-7), 2.5e-8, 1, HOST, 0, force="host")
TRAN_CASES["mixed"] = _case(mixed_linear, (0.0, 4e-6), 1.25e-7, 1, HOST, 0, force="host")
for _n in (7, 12, 13, 16):   # device stepper, lock-step: a lone block per workgroup; 7 is padded to 12, 13 to 16
    TRAN_CASES["lockstep%d" % _n] = _case(lambda n=_n: lockstep_blocks(n, 5), (0.0, 1e-7), 6e-9, 1, DEVICE, LOCKSTEP, force="device")
TRAN_CASES["lockstep7_nopair"] = _case(lambda: lockstep_blocks(7, 5), (0.0, 1e-7), 6e-9, 1, DEVICE, LOCKSTEP, env=NOPAIR, force="device")
TRAN_CASES["lockstep13_two_blocks"] = _case(lambda: lockstep_blocks(13, 2), (0.0, 1e-7), 6e-9, 1, DEVICE, LOCKSTEP, force="device")
TRAN_CASES["tiles80"] = _case(lambda: sine_tiles(80), (0.0, 2e-8), 1.25e-9, 2, DEVICE, BORDERED)
# (72 tiles: up to 64 unknowns the whole array is one block of the fused kernel and is never torn)
TRAN_CASES["two_rail72"] = _case(lambda: two_rail_tiles(72), (0.0, 2e-8), 1.25e-9, 2, DEVICE, BORDERED)
TRAN_CASES["ladder40_sparse"] = _case(lambda: observe_all(rc_ladder(40)), (0.0, 2e-7), 2e-8, 2, HOST, 0, env=SPARSE)
TRAN_CASES["mesh65"] = _case(lambda: linear_mesh(65), (0.0, 4e-7), 2.5e-8, 2, HOST, 0)
TRAN_CASES["two_rail72_subtree"] = _case(lambda: two_rail_tiles(72), (0.0, 2e-8), 1.25e-9, 2, HOST, 0, env=NO_TEAR)
TRAN_CASES["two_rail72_levels"] = _case(lambda: two_rail_tiles(72), (0.0, 2e-8), 1.25e-9, 2, HOST, 0, env=NO_SUBTREE)

# nonlinear operating points: dense_mesh with its MOSFETs
DC_MESH_SIZES = (7, 12, 16, 28, 40, 70)
DC_ABSTOL = 1e-12
DC_SEED_VOLTS = 1e-2


def mos_mesh(n):
    return dense_mesh(n, np.random.default_rng(2000 + n), **mesh_shape(n))


def perturbed_start(c, x_op, node_is_unknown):
    """The oracle's operating point plus a seeded 1e-2 V perturbation of the unknown nodes (node_is_unknown[node id], 1-based)."""
    rng = np.random.default_rng(5)
    x = np.array(x_op, float)
    d = DC_SEED_VOLTS * rng.standard_normal(c.n_nodes)
    for n in range(1, c.n_nodes + 1):
        if node_is_unknown[n]:
            x[n - 1] += d[n - 1]
    return x
