"""Linear circuits at the shape edges of the small-signal and sensitivity solvers (`ac_block_kernel`, `sens_block_kernel`),
shared by the CPU test that pins the reference (test_smallsignal_reference.py) and the GPU tests
(test_gpu_smallsignal_shapes.py).  Every builder is seeded and deterministic.  `ac_reference` computes the refined
solution of a case once per process, together with `e_cpu`, the error two CPU double-precision solvers (the oracle, LAPACK)
make on the same system: the yardstick the GPU tolerance is derived from."""
import copy

import numpy as np

import smallsignal_reference as ref
from cedarsim_jl_amd import Circuit
from cedarsim_jl_amd.circuit import DEV_R, DEV_VCCS, SLOT_DEV_PAR, SLOT_SRC_DC

FREQS = np.array([0.0, 1e-3, 1e3, 1e6, 3.3e8, 1e10, 1e12])
FREQS_LARGE = np.array([0.0, 1e6, 1e12])          # from 255 unknowns up: three frequencies keep the reference and the oracle's dense LU cheap
LADDER_SIZES = [1, 2, 63, 64, 65, 96, 97, 255, 256, 257]
SENS_SIZES = [64, 65, 96, 97]
TOL_FLOOR, TOL_FACTOR, TOL_CEILING, E_CPU_MAX = 1e-12, 32.0, 1e-10, 1e-11


def ladder_freqs(n):
    return FREQS if n <= 97 else FREQS_LARGE


def _logu(rng, lo, hi):
    return float(10.0 ** rng.uniform(np.log10(lo), np.log10(hi)))


def _rlc_sections(c, rng, prefix, start, k, trailing, series=(1e2, 1e4), shunt=(1e4, 1e6)):
    """k sections `series R - series L - (shunt C, shunt R)` from node `start` on, 3 unknowns each (two nodes and the
    inductor current), then `trailing` RC sections of one unknown each; a quarter as many VCCS as sections between random
    section nodes, so that the matrix is not banded.  Returns the list of section end nodes."""
    ends, at = [], start
    for i in range(1, k + 1):
        mid, end = "%sm%d" % (prefix, i), "%sn%d" % (prefix, i)
        c.R("%srs%d" % (prefix, i), at, mid, _logu(rng, *series))
        c.L("%sl%d" % (prefix, i), mid, end, _logu(rng, 1e-7, 1e-5))
        c.C("%sc%d" % (prefix, i), end, 0, _logu(rng, 1e-13, 1e-11))
        c.R("%srp%d" % (prefix, i), end, 0, _logu(rng, *shunt))
        ends.append(end)
        at = end
    for i in range(1, trailing + 1):
        end = "%st%d" % (prefix, i)
        c.R("%srt%d" % (prefix, i), at, end, _logu(rng, *series))
        c.C("%sct%d" % (prefix, i), end, 0, _logu(rng, 1e-13, 1e-11))
        ends.append(end)
        at = end
    if len(ends) >= 4:
        for i in range(1, k // 4 + 1):
            a, b, p, q = (ends[j] for j in rng.choice(len(ends), 4, replace=False))
            c.G("%sg%d" % (prefix, i), a, b, p, q, gain=_logu(rng, 1e-6, 1e-4) * (1.0 if rng.uniform() < 0.5 else -1.0))
    return ends


def ladder(n, dc=0.0):
    """A non-uniform R-L-C ladder with exactly n engine unknowns when built with small_signal=True: the AC voltage source
    keeps its node and its branch (2), every section adds 3, one or two trailing RC sections add the remainder.  n = 1 and
    n = 2 have no room for a source branch: an AC current source drives R || C (n = 1) or R || C - R - R || C (n = 2).
    dc: the DC value of the source (the sensitivity tests use 1; the far node then stays between 8.6e-3 and 6.9 of the
    source at 64, 65, 96 and 97 unknowns, so the ladder is used as it is).
    Returns the circuit; `c.far` is the last node, `c.mid_l` a mid-ladder inductor (or None)."""
    c = Circuit()
    rng = np.random.default_rng(1000 + n)
    c.mid_l = None
    if n <= 2:
        c.I("iin", 0, "n0", dc=dc, ac=1.0)
        c.R("rp0", "n0", 0, _logu(rng, 1e2, 1e4))
        c.C("c0", "n0", 0, _logu(rng, 1e-13, 1e-11))
        c.far = "n0"
        if n == 2:
            c.R("rs1", "n0", "n1", _logu(rng, 1e2, 1e4))
            c.R("rp1", "n1", 0, _logu(rng, 1e4, 1e6))
            c.C("c1", "n1", 0, _logu(rng, 1e-13, 1e-11))
            c.far = "n1"
        return c
    c.V("vin", "n0", 0, dc=dc, ac=1.0)
    k, trailing = (n - 2) // 3, (n - 2) % 3
    ends = _rlc_sections(c, rng, "", "n0", k, trailing)
    c.far = ends[-1]
    c.mid_l = "l%d" % ((k + 1) // 2)
    return c


def pivot_torture():
    """15 unknowns in one block whose diagonal is of no use: a floating voltage source between two unknown nodes, two VCVS in
    a chain, a gyrator (two VCCS of opposite sign) loaded by capacitors only, and a loop of two inductors closed by a
    resistor.  At f = 0 the rows of the four sources, of both inductors and of one gyrator node have an exactly zero diagonal;
    at 1 mHz the inductor diagonals are w L = 6e-9 .. 6e-8 beside column entries of 1."""
    c = Circuit()
    c.V("vin", "a", 0, dc=0.0, ac=1.0)
    c.R("r1", "a", "b", 1.3e3)
    c.V("vf", "b", "c", dc=0.5)                       # floating and not 0 V: neither folded into a known node nor merged
    c.R("rc", "c", 0, 4.7e3)
    c.C("cc", "c", 0, 2e-12)
    c.E("e1", "d", 0, "c", 0, gain=3.0)
    c.R("rd", "d", 0, 2.2e3)
    c.E("e2", "e", 0, "d", 0, gain=-2.0)
    c.R("re", "e", "p", 820.0)
    c.G("gy1", "p", 0, "q", 0, gain=1e-3)
    c.G("gy2", "q", 0, "p", 0, gain=-1e-3)
    c.C("cp", "p", 0, 1e-11)
    c.C("cq", "q", 0, 3e-11)
    c.L("la", "e", "m1", 1e-6)
    c.L("lb", "m1", "m2", 1e-5)
    c.R("rl", "m2", "e", 150.0)
    c.R("rm", "m1", 0, 3.3e4)
    return c


BLOCK_SIZES = [1, 2, 3, 17, 64]


def blocks():
    """Five independent components on the fused path, 1, 2, 3, 17 and 64 unknowns in this order.  The first has no source
    at all; the three middle ones are driven by AC current sources of different magnitudes (with DC values, so that DC
    sensitivities are not identically zero); the last by an AC voltage source with dc = 5.  `c.block_nodes[k]` lists the
    node names of component k, `c.sweep` the two swept slots (a resistor of the 17-block, a capacitor of the 64-block) and
    their S = 3 values."""
    c = Circuit()
    rng = np.random.default_rng(78)
    c.R("ur", "u1", 0, 2.7e3)
    c.C("uc", "u1", 0, 1.5e-12)
    c.I("vi", 0, "v1", dc=1e-4, ac=1e-3)
    c.C("vc1", "v1", 0, 1e-12)
    c.R("vr1", "v1", "v2", 1.8e3)
    c.R("vr2", "v2", 0, 5.6e3)
    c.C("vc2", "v2", 0, 3e-12)
    c.I("wi", 0, "w1", dc=2e-3, ac=2.0)
    c.R("wr1", "w1", 0, 680.0)
    c.L("wl", "w1", "w2", 2e-6)
    c.R("wr2", "w2", 0, 1.2e3)
    c.C("wc", "w2", 0, 4e-12)
    c.I("xi", 0, "x0", dc=5e-4, ac=0.3)
    c.R("xr0", "x0", 0, 3.9e3)
    xe = _rlc_sections(c, rng, "x", "x0", 5, 1)
    c.V("yv", "y0", 0, dc=5.0, ac=1.0)
    ye = _rlc_sections(c, rng, "y", "y0", 20, 2)
    names = {0: ["u1"], 1: ["v1", "v2"], 2: ["w1", "w2"], 3: ["x0"], 4: ["y0"]}
    for k, pre, n_sec in ((3, "x", 5), (4, "y", 20)):
        names[k] += ["%sm%d" % (pre, i) for i in range(1, n_sec + 1)]
    names[3] += xe
    names[4] += ye
    c.block_nodes = names
    c.block_branches = {0: [], 1: [], 2: ["wl"], 3: ["xl%d" % i for i in range(1, 6)], 4: ["yv"] + ["yl%d" % i for i in range(1, 21)]}
    r17, c64 = c.slot("xrs3"), c.slot("yc7")
    c.sweep = ([r17, c64], [[base_value(c, r17) * f for f in (1.0, 0.4, 2.5)], [base_value(c, c64) * f for f in (1.0, 3.0, 0.2)]])
    return c


def block_groups(c):
    """MNA rows of every component, node voltages and branch currents apart: the groups `scaled_error` scales by."""
    out = []
    for k in range(len(BLOCK_SIZES)):
        out.append([c.mna_index("v", nm) for nm in c.block_nodes[k]])
        out.append([c.mna_index("i", nm) for nm in c.block_branches[k]])
    return out


def offset_source():
    """The RC cell driven by a voltage source with dc = 5 and ac = 1e-3: the AC right-hand side is the difference of two
    residuals whose source values are 5 and 5 + 1e-3."""
    c = Circuit()
    c.V("vin", "a", 0, dc=5.0, ac=1e-3)
    c.R("r1", "a", "b", 1e3)
    c.C("c1", "b", 0, 1e-9)
    c.rc = 1e3 * 1e-9
    return c


def offset_groups(c):
    """Node voltages only.  At 1 mHz the source current is w C |ac| = 6e-15 A, formed from two node voltages that differ
    by w R C = 6e-9 of themselves: its real part lies below the rounding of those voltages in ANY double-precision MNA solve
    (LAPACK and the oracle both lose it), so it says nothing about a solver."""
    return [list(range(c.n_nodes))]


CHUNK_SECTIONS, CHUNK_SAMPLES, CHUNK_NFREQ = 300, 2, 400


def chunk_ladder():
    """A non-uniform RC ladder of 300 sections: 302 unknowns with the AC source's node and branch.  With S = 2 samples and
    400 frequencies the global workspace of the complex LU exceeds its cap and the sweep takes two launches.  `c.rs`, `c.cs`
    are the element values, `c.sweep` the swept slot (one resistor) and its two values."""
    c = Circuit()
    rng = np.random.default_rng(302)
    c.V("vin", "n0", 0, dc=0.0, ac=1.0)
    c.rs = [float(rng.uniform(0.5e3, 2e3)) for _ in range(CHUNK_SECTIONS)]
    c.cs = [float(rng.uniform(0.5e-12, 2e-12)) for _ in range(CHUNK_SECTIONS)]
    for i in range(CHUNK_SECTIONS):
        c.R("r%d" % (i + 1), "n%d" % i, "n%d" % (i + 1), c.rs[i])
        c.C("c%d" % (i + 1), "n%d" % (i + 1), 0, c.cs[i])
    c.sweep = (c.slot("r8"), [c.rs[7], 2.5 * c.rs[7]])
    c.freqs = np.logspace(4.0, 8.0, CHUNK_NFREQ)    # from 10 kHz: below, the matrix nears the bare Laplacian of condition N^2 = 9e4
    c.out = 40                                      # noise output: ladder node n40
    return c


def chunk_values(c, sample):
    rs = list(c.rs)
    rs[7] = c.sweep[1][sample]
    return rs, c.cs


def sens_slot_names(c, n):
    """Ten resistors spread over the ladder, the source and one VCCS gain; then (used at 96 unknowns only) every other
    resistor and VCCS and every capacitor and inductor, whose rows are exactly zero at DC."""
    res = [nm for nm, k in zip(c.dev_names, c.dev_kind) if k == DEV_R]
    spread = [res[int(round(j))] for j in np.linspace(0, len(res) - 1, 10)]
    first = spread + ["vin", "g1"]
    return first + [nm for nm in c.dev_names if nm not in first]


def carries_no_dc_current(c, name):
    """The series resistor rt<i> of a trailing RC section feeds capacitors alone — unless a VCCS drives its current into one of
    the trailing nodes t<i>, t<i+1>, ...  Without such a VCCS no DC current flows and dx/dR is identically zero: what a solver
    returns for it is rounding noise (1e-52 in the reference), which no relative tolerance can be scaled by."""
    if not name.startswith("rt"):
        return False
    down = {c._n("t%d" % j) for j in range(int(name[2:]), 3) if ("t%d" % j) in c._node_ix}
    return not any(k == DEV_VCCS and (nd[0] in down or nd[1] in down) for k, nd in zip(c.dev_kind, c.dev_node))


def zero_slot_bound(c, names, want):
    """Absolute bound for a slot whose derivative is identically zero: 1e-8 (the atol factor of the other slots) of the
    SMALLEST max|dx/dp_k| among the ladder's requested resistors that do carry current, taken from the reference."""
    return 1e-8 * min(np.max(np.abs(want[k])) for k, nm in enumerate(names) if nm[0] == "r" and not carries_no_dc_current(c, nm))


# ---- parameters ----
def base_value(c, slot):
    kind, a, b = c.slots[slot]
    return c.dev_par[a][b] if kind == SLOT_DEV_PAR else c.sources[a][0]


def at_params(c, values):
    """A copy of the circuit with {slot: value} written into its record (device parameters and source DC values)."""
    d = copy.deepcopy(c)
    for slot, v in values.items():
        kind, a, b = d.slots[slot]
        if kind == SLOT_DEV_PAR:
            d.dev_par[a][b] = float(v)
        elif kind == SLOT_SRC_DC:
            d.sources[a] = (float(v), d.sources[a][1])
        else:
            raise ValueError("at_params: slot kind %d" % kind)
    return d


# ---- references, computed once per process ----
_CACHE = {}


def tolerance(e_cpu):
    """max(1e-12, 32 e_cpu) on the scale of `scaled_error`.  32: the kernel pivots on |re| + |im| instead of the modulus
    and may take another pivot order, and its G, C are the engine's own stamps of 1/R — each worth a few roundings, not
    orders of magnitude.  A case whose tolerance would exceed 1e-10 is mis-designed (the closed-form AC bound of
    test_gpu_ac_noise.py is 1e-9)."""
    tol = max(TOL_FLOOR, TOL_FACTOR * e_cpu)
    assert tol <= TOL_CEILING, "mis-designed case: e_cpu = %.3e" % e_cpu
    return tol


def ac_reference(key, circuit, freqs, Oracle, groups=None):
    """{x: refined phasors [n_freq][n_mna], e_lapack, e_oracle, e_cpu (per case: the worst frequency), tol, xo} of a case,
    cached under `key` together with the frequencies, the size and the groups, so that a reused name cannot return another
    case's data.  Errors are `scaled_error`s against the refined solution."""
    groups = groups or ref.unit_groups(circuit)
    key = (key, "ac", tuple(float(f) for f in freqs), circuit.n_mna, tuple(tuple(int(i) for i in g) for g in groups))
    if key in _CACHE:
        return _CACHE[key]
    rc, xo = Oracle(circuit).ac(freqs)
    assert rc == 0
    xs, e_lapack, e_oracle = [], [], []
    for k, f in enumerate(freqs):
        Y, b = ref.mna(circuit, 2.0 * np.pi * f)
        x, _, _ = ref.solve(Y, b)
        xs.append(x)
        e_lapack.append(ref.scaled_error(np.linalg.solve(Y, b), x, groups))
        e_oracle.append(ref.scaled_error(xo[k], x, groups))
    e_cpu = max(max(e_lapack), max(e_oracle))
    out = dict(x=np.array(xs), xo=xo, e_lapack=np.array(e_lapack), e_oracle=np.array(e_oracle), e_cpu=e_cpu, groups=groups)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = out
    return out


def noise_reference(key, circuit, out_index, freqs):
    """Refined adjoint PSD [n_freq] at MNA row `out_index`, cached."""
    key = (key, "noise", int(out_index), tuple(float(f) for f in freqs), circuit.n_mna)
    if key not in _CACHE:
        p = np.array([ref.noise_psd(circuit, out_index, 2.0 * np.pi * f) for f in freqs])
        p.setflags(write=False)
        _CACHE[key] = p
    return _CACHE[key]


def chunk_reference(c, launch_chunk, Oracle):
    """Thomas solves of the chunking ladder for every (sample, frequency) and the 40-digit recurrence at four frequencies: the
    first, the last of the first launch, the first of the second launch and the last.
    e_cpu differs from the other cases': 800 systems of 302 unknowns are too many for 40 digits, so it is measured at those
    four frequencies only (both samples) — the larger of the Thomas solve's and the oracle's error against the recurrence,
    node voltages and the source current scaled apart, the PSD relative.  The other 396 frequencies are judged by the Thomas
    solve, whose own error is what e_cpu bounds at the four."""
    key = ("chunk", launch_chunk, tuple(c.freqs))
    if key in _CACHE:
        return _CACHE[key]
    nodes = [c.mna_index("v", "n%d" % k) for k in range(1, CHUNK_SECTIONS + 1)]
    iv, o = c.mna_index("i", "vin"), Oracle(c)
    w = 2.0 * np.pi * c.freqs
    check = [0, launch_chunk - 1, launch_chunk, len(c.freqs) - 1]
    v, i, psd, vmp, pmp, e, e_oracle = [], [], [], {}, {}, 0.0, 0.0
    for s in range(CHUNK_SAMPLES):
        rs, cs = chunk_values(c, s)
        o.set_param(c.sweep[0], c.sweep[1][s])
        rc, xo = o.ac(c.freqs[check])
        rcn, po = o.noise(c.mna_index("v", "n%d" % c.out), c.freqs[check])
        assert rc == 0 and rcn == 0
        vs, is_ = ref.rc_ladder_ac(rs, cs, w)
        v.append(vs)
        i.append(is_)
        psd.append(ref.rc_ladder_noise(rs, cs, w, c.out, c.temp))
        for k in check:
            vm, im = ref.rc_ladder_mp(rs, cs, w[k])
            vmp[s, k] = (vm, im)
            pmp[s, k] = ref.rc_ladder_noise_mp(rs, cs, w[k], c.out, c.temp)
            e = max(e, np.max(np.abs(vs[k] - vm)) / np.max(np.abs(vm)), abs(is_[k] - im) / abs(im), abs(psd[s][k] - pmp[s, k]) / pmp[s, k])
            j = check.index(k)
            e_oracle = max(e_oracle, np.max(np.abs(xo[j][nodes] - vm)) / np.max(np.abs(vm)), abs(xo[j][iv] - im) / abs(im),
                           abs(po[j] - pmp[s, k]) / (2.0 * pmp[s, k]))
    out = dict(v=np.array(v), i=np.array(i), psd=np.array(psd), check=check, v_mp=vmp, psd_mp=pmp, e_thomas=float(e),
               e_oracle=float(e_oracle), e_cpu=float(max(e, e_oracle)))
    _CACHE[key] = out
    return out
