"""The swept-name -> table-entry map of a `CircuitSweep`, learned on the host from a few netlist builds.

The reference rebuilds nothing per point: `remake(prob, p=sim)` swaps a parameter struct (src/sweeps.jl:278-290, 473-480).
Here the netlist is rebuilt only as often as needed to LEARN which table entries every swept name moves, and how:
  * a variable with at most four distinct values: one build per value (exact look-up);
  * any other variable (the Monte-Carlo shape: a TandemSweep with as many distinct values as points): three builds —
    two determine an identity / proportional / affine map for every entry the variable moves, the third checks it;
  * the assembled table is then VALIDATED against full builds of the point with the most variables away from the
    base point and of a few seeded random points: an entry that answers to two variables (r = a*b with a base of
    a = 0, a conditional) is not visible from single-axis builds around one point.
Any failed check (an entry moved by two variables, a non-affine map, a validation mismatch) falls back to one build
per point, which is always correct.

Host only: numpy and the circuit tables, nothing of the GPU binding.  Fuzzed by scripts/extended_fuzz_sweepmap.py.
"""
import copy
import time

import numpy as np

from .circuit import (SLOT_DEV_MULT, SLOT_DEV_PAR, SLOT_GMIN, SLOT_MODEL_PAR, SLOT_SRC_DC, SLOT_SRC_PAR, SLOT_TEMP, SLOT_VA_PAR,
                      CedarError)


def differs(x, y):
    return (x != y) & ~(np.isnan(x) & np.isnan(y))


def close(x, y):
    return np.all((x == y) | (np.isnan(x) & np.isnan(y)) | (np.abs(x - y) <= 1e-13 * np.maximum(np.abs(x), np.abs(y))))


def numeric(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def flat_table(c):
    """Every sweepable entry of a circuit's tables as one vector, with the engine slot (kind, a, b) of each position."""
    vals, keys = [], []
    par = np.array(c.dev_par, float).reshape(len(c.dev_par), -1) if len(c.dev_par) else np.zeros((0, 8))
    for d in range(par.shape[0]):
        vals.extend(par[d]); keys.extend((SLOT_DEV_PAR, d, k) for k in range(par.shape[1]))
    vals.extend(float(m) for m in c.dev_mult); keys.extend((SLOT_DEV_MULT, d, 0) for d in range(len(c.dev_mult)))
    for i, sv in enumerate(c.sources):
        vals.append(float(sv[0])); keys.append((SLOT_SRC_DC, i, 0))
        pr = list(sv[1].par) + [0.0] * (8 - len(sv[1].par))
        vals.extend(float(x) for x in pr); keys.extend((SLOT_SRC_PAR, i, k) for k in range(8))
    for m, card in enumerate(c.models):
        vals.extend(float(x) for x in card); keys.extend((SLOT_MODEL_PAR, m, k) for k in range(len(card)))
    vals.extend(float(x) for x in c.va_par); keys.extend((SLOT_VA_PAR, i, 0) for i in range(len(c.va_par)))
    vals.append(float(c.temp)); keys.append((SLOT_TEMP, 0, 0))
    vals.append(float(c.gmin)); keys.append((SLOT_GMIN, 0, 0))
    return np.array(vals, float), keys


def _learn_table(pts, names, distinct, v0, flat_of):
    """Per-point flat tables from single-axis builds around pts[0]; None when the sweep is not separable that way."""
    owner = np.full(len(v0), -1)
    table = np.tile(v0, (len(pts), 1))
    for ki, k in enumerate(names):
        vals = distinct[k]
        x0 = pts[0][k]
        others = [v for v in vals if v != x0]
        if not others:
            continue
        cols = {x0: v0}

        def lookup():
            moved = np.zeros(len(v0), bool)
            for val in others:
                if val not in cols:
                    cols[val] = flat_of(dict(pts[0], **{k: val}))
                moved |= differs(cols[val], v0)
            if np.any(moved & (owner >= 0) & (owner != ki)):
                return False
            owner[moved] = ki
            idx = np.nonzero(moved)[0]
            for r, p in enumerate(pts):
                table[r, idx] = cols[p[k]][idx]
            return True

        if len(others) <= 3 or not all(numeric(v) for v in vals):
            if not lookup():
                return None
            continue
        # many distinct numeric values: every entry the variable moves must be an affine function of it
        x1 = max(others, key=lambda v: abs(v - x0))
        x2 = min((v for v in others if v != x1), key=lambda v: abs(v - 0.5 * (x0 + x1)))
        v1, v2 = flat_of(dict(pts[0], **{k: x1})), flat_of(dict(pts[0], **{k: x2}))
        cols[x1], cols[x2] = v1, v2
        moved = differs(v1, v0) | differs(v2, v0)
        if np.any(moved & (owner >= 0)):
            return None
        idx = np.nonzero(moved)[0]
        if not len(idx):
            continue
        xs = np.array([float(p[k]) for p in pts])
        a0, a1, a2 = v0[idx], v1[idx], v2[idx]
        ident = (a0 == x0) & (a1 == x1) & (a2 == x2)
        with np.errstate(all="ignore"):
            cprop = a1 / x1 if x1 != 0 else np.full(len(idx), np.nan)
            prop = ~ident & (cprop * x0 == a0) & (cprop * x2 == a2)
            slope = (a1 - a0) / (float(x1) - float(x0))
            pred2 = a0 + slope * (float(x2) - float(x0))
        if not close(np.where(ident | prop, a2, pred2), a2):
            # not affine in the swept variable (1/x, x^2, a table look-up ...): one build per distinct value, if that is
            # still cheaper than one per point
            if 2 * len(vals) < len(pts) and lookup():
                continue
            return None
        owner[moved] = ki
        col = a0[None, :] + slope[None, :] * (xs[:, None] - float(x0))
        col = np.where(prop[None, :], cprop[None, :] * xs[:, None], col)   # the builder's own product, bit for bit
        col = np.where(ident[None, :], xs[:, None], col)
        table[:, idx] = col
    return table


def validation_points(pts, names, fitted, n_check):
    """Indices of the points whose full builds the assembled table is checked against, ascending; never the base point."""
    # the point farthest from the base point (most variables changed) + seeded random points
    def away(r):
        return sum(pts[r][j] != pts[0][j] for j in names)

    far = max(range(1, len(pts)), key=away)
    rng = np.random.default_rng(len(pts))
    picks = {far, len(pts) - 1} | {int(r) for r in rng.integers(1, len(pts), size=max(0, n_check - 2))}
    # ... and, for every variable whose map was FITTED from three values, the points that hold its smallest and its
    # largest value: a clipped or saturating entry (max(x, lower bound), a model card's limits) is affine on the
    # three fitted values and wrong beyond the kink (scripts/extended_fuzz_sweepmap.py, 2 of 1 500 random builders)
    # Among the points that hold such an extreme, the one with the most OTHER variables away from the base point: an
    # entry that follows one variable only while another is beyond a threshold shows there and nowhere on the axes.
    for k in fitted:
        for ext in (min(p[k] for p in pts), max(p[k] for p in pts)):
            picks.add(max((r for r in range(len(pts)) if pts[r][k] == ext), key=lambda r: (away(r), r)))
    picks.discard(0)
    return sorted(picks)


def learn_batch(build, points):
    """Base circuit + slots + per-sample values for `points`, found by diffing the flat tables of built circuits (see the module
    text).  Returns (base, slot_ids, values[slot][point], setup); `base.slots` / `base.slot_names` are set, and `setup` records
    what was done (points, circuit_builds, seconds, how, slots)."""
    t_setup = time.perf_counter()
    pts = points
    base = build(**pts[0])
    v0, keys = flat_table(base)
    n_builds = [1]

    def flat_of(point):
        c = build(**point)
        n_builds[0] += 1
        if c.dev_kind != base.dev_kind or c.dev_node != base.dev_node or c.dev_ipar != base.dev_ipar:
            raise CedarError("sweep points must not change the circuit topology")
        vv, _ = flat_table(c)
        if len(vv) != len(v0):
            raise CedarError("sweep points must not change the circuit topology")
        return vv

    table, how = None, "one build per point"
    names = sorted({k for p in pts for k in p})
    if names and len(pts) > 1 and all(set(p) == set(names) for p in pts):
        distinct = {k: list(dict.fromkeys(p[k] for p in pts)) for k in names}
        n_check = min(4, len(pts) - 1)
        fitted = [k for k in names if len(distinct[k]) > 4 and all(numeric(x) for x in distinct[k])]   # variables whose map is fitted, not looked up
        cost = 1 + sum(min(len(v) - 1, 2) if all(numeric(x) for x in v) else len(v) - 1 for v in distinct.values()) + n_check + 2 * len(fitted)
        if cost < len(pts):
            table = _learn_table(pts, names, distinct, v0, flat_of)
            if table is not None and not all(close(flat_of(pts[r]), table[r]) for r in validation_points(pts, names, fitted, n_check)):
                table = None   # e.g. an entry that depends on two swept variables
            if table is not None:
                how = "learned map (%d builds for %d points)" % (n_builds[0], len(pts))
    if table is None:
        table = np.array([v0] + [flat_of(p) for p in pts[1:]])
    ch = np.nonzero(np.any(differs(table, table[0:1]), axis=0))[0]
    slots = [keys[i] for i in ch]
    # a constant source whose dc is swept: SRC_DC already updates the transient value
    drop = {i for i in ch if keys[i][0] == SLOT_SRC_PAR and keys[i][2] == 0 and base.sources[keys[i][1]][1].kind == 0 and (SLOT_SRC_DC, keys[i][1], 0) in slots}
    ch = [i for i in ch if i not in drop]
    slots = [keys[i] for i in ch]
    base.slots = list(slots)
    base.slot_names = [("slot%d" % i, None) for i in range(len(slots))]
    setup = {"points": len(pts), "circuit_builds": n_builds[0], "seconds": time.perf_counter() - t_setup, "how": how, "slots": len(slots)}
    return base, list(range(len(slots))), np.ascontiguousarray(table[:, ch].T, float).reshape(len(slots), len(pts)), setup


def sample_view(ckt, values, s):
    """Shallow per-sample view of `ckt` so that post-processing (e.g. R.I = V/r) uses the values of sample `s`."""
    c = copy.copy(ckt)
    c.dev_par = [list(p) for p in ckt.dev_par]
    for i, sl in enumerate(ckt.slots):
        if sl[0] == SLOT_DEV_PAR:
            c.dev_par[sl[1]][sl[2]] = float(values[i][s])
    return c
