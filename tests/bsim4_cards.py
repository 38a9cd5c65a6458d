"""BSIM4 card variants, the bias set and the per-row error scale shared by test_bsim4_oracle.py (CPU) and
test_gpu_bsim4_cards.py (GPU).  A plain helper module: no fixtures, no test collection.

Every variant is a set of overrides applied to BOTH GF180 cards (nfet_06v0, pfet_06v0); the instances are those of
test_bsim4_oracle.two_fets.  The variants walk the branches of the model that the GF180 cards themselves never take
(mobmod 1/2 and their defaults, capmod 0, the three charge partitions and xpart < 0, the poly-depletion window, impact
ionisation, GIDL/GISL, k1ox == 0, dead junctions, the output-resistance and pocket terms, the diffusion geometry)."""
import numpy as np

from cedarsim_jl_amd import PULSE, Circuit
from cedarsim_jl_amd.workloads import gf180_models

REMOVED = None   # an override of REMOVED takes the parameter off the card: both sides then use their default

_NOMOB = dict(ua=0.0, ub=0.0, uc=0.0, ua1=0.0, ub1=0.0, uc1=0.0)

# name -> (card overrides, instance keyword arguments)
VARIANTS = {
    "base": ({}, {}),
    "mob1": (dict(mobmod=1, ua=1e-9, uc=-0.0465), {}),
    "mob2": (dict(mobmod=2, ua=1e-15, uc=-0.0465e-9, eu=1.67), {}),
    "mob1_dflt": (dict(mobmod=1, ua=REMOVED, uc=REMOVED, uc1=REMOVED, eu=REMOVED), {}),
    "mob2_dflt": (dict(mobmod=2, ua=REMOVED, uc=REMOVED, uc1=REMOVED, eu=REMOVED), {}),
    "cap0": (dict(capmod=0), {}),
    "xp05": (dict(xpart=0.5), {}),
    "xp1": (dict(xpart=1.0), {}),
    "xpneg": (dict(xpart=-1.0), {}),
    "ngate0": (dict(ngate=0.0), {}),
    "ngate_hi": (dict(ngate=1e26), {}),
    "isub": (dict(alpha0=1e-6, beta0=20.0), {}),
    "isub0": (dict(alpha0=0.0, beta0=20.0), {}),
    "gidl": (dict(agidl=1e-9), {}),
    "gidl0": (dict(agidl=0.0), {}),
    "k1zero": (dict(k1=0.0, k2=0.0), {}),
    "nojn": (dict(jss=0.0, jsws=0.0, jswgs=0.0, cjs=0.0, cjsws=0.0, cjswgs=0.0), {}),
    "rout": (dict(pdits=0.5, pditsd=0.3, fprout=1.0, pvag=0.5), {}),
    "minv": (dict(minv=0.3, dvtp0=1e-7, dvtp1=0.1), {}),
    "geom": (dict(permod=0), dict(nf=2, as_=2.0e-13, ad=1.5e-13, ps=1.6e-6, pd=1.3e-6)),
}
NAMES = list(VARIANTS)
# the variants of the issue's circuit-level tests (assembled Jacobian, steppers)
CIRCUIT_NAMES = ["mob1", "mob2", "xp05", "xp1", "cap0", "isub", "gidl", "geom"]

# model selectors of sub-models that neither side implements: both must refuse the card (CH_ERR_UNSUPPORTED)
UNSUPPORTED_SELECTORS = [("rdsmod", 1), ("rgatemod", 1), ("rbodymod", 1), ("igcmod", 1), ("igbmod", 1), ("trnqsmod", 1),
                         ("geomod", 1), ("diomod", 0), ("diomod", 2), ("capmod", 1), ("mobmod", 3)]

WN, LN, WP, LP = 3.6e-7, 6e-7, 4.95e-7, 5e-7   # test_bsim4_oracle.two_fets


def cards(overrides):
    """The two GF180 cards with `overrides` applied: (name, type, params) for nfet_06v0 and pfet_06v0."""
    out = []
    for nm in ("nfet_06v0", "pfet_06v0"):
        name, mtype, params = gf180_models()[nm]
        p = {k.lower(): v for k, v in params.items()}
        for k, v in overrides.items():
            if v is REMOVED:
                p.pop(k, None)
            else:
                p[k] = v
        out.append((name, mtype, p))
    return out


def resolve(variant):
    """variant: a name of VARIANTS, or a dict of card overrides -> (overrides, instance kwargs)."""
    return VARIANTS[variant] if isinstance(variant, str) else (dict(variant), {})


def two_fets(variant="base", rows=1, mirror=False, **kw):
    """`rows` copies of the (mn, mp) pair of test_bsim4_oracle.two_fets on the cards of `variant`; MOS instance 2r is the
    NMOS and 2r+1 the PMOS of copy r.  The `temp` slot is declared, so one circuit serves every temperature.
    mirror=True exchanges the source and drain diffusions (as/ad, ps/pd) of the instances."""
    ov, inst = resolve(variant)
    if mirror and inst:
        inst = dict(inst, as_=inst["ad"], ad=inst["as_"], ps=inst["pd"], pd=inst["ps"])
    c = Circuit(**kw)
    (nn, nt, npar), (pn, pt, ppar) = cards(ov)
    n, p = c.add_model(nn, nt, npar), c.add_model(pn, pt, ppar)
    for r in range(rows):
        c.M("mn%d" % r, "d", "g", "s", "b", n, WN, LN, **inst)
        c.M("mp%d" % r, "d", "g", "s", "b", p, WP, LP, **inst)
    c.slot("temp")
    return c


def fet_bank(variant, rows):
    """two_fets(rows=...) with every terminal driven through a resistor, as the engine wants a circuit it could solve; the
    stand-alone device evaluations (mos_eval) take their voltages from the caller and ignore the nets."""
    c = two_fets(variant, rows=rows)
    for k, nd in enumerate("dgsb"):
        c.V("v" + nd, "x" + nd, 0, dc=0.0)
        c.R("r" + nd, "x" + nd, nd, 1e3)
    return c


def bias_rows():
    """The bias set, one row (vd, vg, vs, vb) per NMOS evaluation: the three random boxes of the existing stamp test
    (test_gpu_parity.test_bsim4_stamps_match_oracle), 30 rows each, and the fixed edge rows."""
    rng = np.random.default_rng(0)
    rows = [lo + scale * rng.random((30, 4)) for scale, lo in ((6.5, -0.75), (0.2, 2.4), (12.0, -3.0))]
    edge = [[2, 3, 2, 0],        # vds = 0 exactly, channel on
            [0.5, 3, 4, 0],      # reverse mode
            [0, 5, 0, 0.9],      # both junctions forward biased, vds = 0
            [5, -2, 0, 0],       # accumulation, GIDL
            [1, 1, 1, 1],        # every branch voltage zero
            [0, 0, 0, 0],
            [5, 0.3, 0, 0],      # deep subthreshold
            [1e-9, 3, 0, 0],     # a nanovolt into forward mode
            [0, 3, 1e-9, 0],     # a nanovolt into reverse mode
            [5, 5, 0, -3],       # saturation with body bias
            [0.05, 0.6, 0, 0]]   # linear region near threshold
    rows.append(np.array(edge, dtype=np.float64))
    return np.vstack(rows)


FAR_SCALES = (20.0, 40.0)
# rows of far_bias_rows() on which rounding of the INPUT alone moves the oracle by more than 2e-11 of the row scale on some variant
# (test_bsim4_oracle.test_far_bias_rows_are_finite_and_well_conditioned measures it): left out of the GPU comparison, by index.
#    2  [ 11.88,  -1.28,  -7.88,  -8.86]   9.3e-11 (mob2, mob2_dflt)        52  [ 21.12,  25.22,  18.40, -30.94]   5.2e-11 (mob2)
#   19  [ 17.80,  16.16,   2.79, -14.18]   4.1e-11 (mob2_dflt)              60  [ 40, 40, 0, -40] body far negative at 40 V: 3.7e-11 (17 variants)
FAR_ILL_CONDITIONED = (2, 19, 52, 60)


def far_bias_rows():
    """Where the Newton iterates of a cold start go and bias_rows() does not: for each of 20 V and 40 V, 24 seeded rows
    (vd, vg, vs, vb) uniform in +-scale and eight edge rows at the scale."""
    rng = np.random.default_rng(7)
    edge = np.array([[1, 1, 0, 0],        # all on
                     [1, -1, 0, 0],       # gate far negative
                     [0, 0, 0, 1],        # both junctions far forward
                     [-1, 1, 0, 0],       # drain far negative
                     [1, 1, 0, -1],       # body far negative
                     [1, 1, 1, 1],        # all four terminals equal
                     [0, 1, 1, 0],        # all on in reverse mode
                     [0.5, -1, 0, -1]],   # gate and body far negative
                    dtype=np.float64)
    rows = []
    for scale in FAR_SCALES:
        rows.append(scale * (2 * rng.random((24, 4)) - 1))
        rows.append(scale * edge)
    return np.vstack(rows)


def far_admitted_rows():
    """far_bias_rows() without the rows named in FAR_ILL_CONDITIONED"""
    rows = far_bias_rows()
    return rows[[i for i in range(len(rows)) if i not in FAR_ILL_CONDITIONED]]


def bank_voltages(rows):
    """Voltages for two_fets(rows=len(rows)): the PMOS of each pair gets the negated row."""
    v = np.empty((2 * len(rows), 4))
    v[0::2] = rows
    v[1::2] = -rows
    return v


def row_scales(ref):
    """Per instance row of the 40-slot record [I(4) | Q(4) | G(16) | C(16)]: the magnitude an error in each slot is judged
    against.  Conductances and capacitances by the row's own largest; currents and charges by the row's own largest, or by what
    1 mV across that conductance / capacitance moves, whichever is larger (keeps the rows whose currents are all zero
    defined)."""
    ref = np.atleast_2d(ref)
    sG = np.abs(ref[:, 8:24]).max(axis=1)
    sC = np.abs(ref[:, 24:40]).max(axis=1)
    sI = np.maximum(np.abs(ref[:, 0:4]).max(axis=1), 1e-3 * sG)
    sQ = np.maximum(np.abs(ref[:, 4:8]).max(axis=1), 1e-3 * sC)
    sc = np.empty_like(ref)
    sc[:, 0:4], sc[:, 4:8], sc[:, 8:24], sc[:, 24:40] = sI[:, None], sQ[:, None], sG[:, None], sC[:, None]
    return np.maximum(sc, 1e-300)


SLOT_NAMES = (["I%s" % t for t in "dgsb"] + ["Q%s" % t for t in "dgsb"] +
              ["G%s%s" % (a, b) for a in "dgsb" for b in "dgsb"] + ["C%s%s" % (a, b) for a in "dgsb" for b in "dgsb"])


def worst(a, b):
    """(error, row, slot) of the largest row-scaled difference of two record arrays; b is the reference."""
    err = np.abs(a - b) / row_scales(b)
    err = np.where(np.isfinite(err), err, np.inf)   # a NaN in either side is the worst error there is
    r, s = np.unravel_index(np.argmax(err), err.shape)
    return float(err[r, s]), int(r), int(s)


def inverter_chain(variant):
    """Two inverters in a row on the cards of `variant`, a load capacitor on each output, the input on a pulse: the smallest
    circuit in which the model runs inside the assembled Jacobian and the steppers (2 NMOS + 2 PMOS + 2 C, two unknowns)."""
    ov, inst = resolve(variant)
    c = Circuit(gmin=1e-15)
    (nn, nt, npar), (pn, pt, ppar) = cards(ov)
    n, p = c.add_model(nn, nt, npar), c.add_model(pn, pt, ppar)
    c.V("vdd", "vdd", 0, dc=5.0)
    c.V("vin", "in", 0, dc=0.0, tran=PULSE(0.0, 5.0, 1e-9, 1e-9, 1e-9, 4e-9, 2e-8))
    for k, (a, b) in enumerate((("in", "o1"), ("o1", "o2"))):
        c.M("mn%d" % k, b, a, 0, 0, n, WN, LN, **inst)
        c.M("mp%d" % k, b, a, "vdd", "vdd", p, WP, LP, **inst)
        c.C("c%d" % k, b, 0, 2e-14)
    c.observe_node("o1")
    c.observe_node("o2")
    return c


CHAIN_TSPAN = (0.0, 1e-8)
# six points over the rise (1..2 ns) and the fall (6..7 ns) of the input
CHAIN_SAVEAT = np.array([1.5e-9, 2.0e-9, 2.6e-9, 6.5e-9, 7.0e-9, 1e-8])
