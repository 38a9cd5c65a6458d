"""What a result is: the solution classes of the analyses in api.py and the host-side post-processing behind them — symbols to rows of
an MNA vector, parameter names to columns, dense output.  Pure numpy: the classes that sample on demand are handed their engine circuit
from outside, and nothing here loads the GPU binding."""
import math
import re
from types import MappingProxyType
from typing import NamedTuple

import numpy as np

from .circuit import (DEV_C, DEV_L, DEV_MOS, DEV_R, DEV_V, DEV_VCVS, RETCODES, SLOT_DEV_MULT, SLOT_DEV_PAR, SLOT_GMIN, SLOT_MODEL_PAR, SLOT_SRC_DC,
                      SLOT_SRC_PAR, SLOT_TEMP, SLOT_VA_PAR, CedarError, dc_opts)


def _split_sym(ckt, sym):
    """'node_q' / 'q' -> (node name, None, None); 'r1.i' / 'r1.v' -> (None, device index, 'i' / 'v'); anything else is a KeyError."""
    nm = str(sym).lower()
    if nm.startswith("node_"):
        nm = nm[5:]
    if nm in ckt._node_ix:
        return nm, None, None
    if "." in nm:
        dev, fld = nm.rsplit(".", 1)
        if dev in ckt.dev_names and fld in ("i", "v"):
            return None, ckt.dev_names.index(dev), fld
    raise KeyError(sym)


def _resolve_sym(ckt, sym):
    """'node_vout' / 'vout' → ('v', node id); 'l3.i' → ('i', device index); 'l3.v' → ('dv', a, b)."""
    node, i, fld = _split_sym(ckt, sym)
    if node is not None:
        return ("v", ckt._n(node))
    if fld == "v":
        return ("dv", ckt.dev_node[i][0], ckt.dev_node[i][1])
    if ckt.dev_kind[i] in (DEV_V, DEV_L, DEV_VCVS):
        return ("i", i)
    raise KeyError(sym)


def _pick(ckt, r, sym, x, nan_is_error):
    """The resolved symbol `r` out of MNA values x[..., n_mna] — one real row, or complex phasors [n_freq][n_mna]: a node (ground is
    zero), the difference across a device, or a branch current.  The row of an eliminated branch is NaN, and `nan_is_error` says
    whether that raises: the complex results always do; a real row does while its operating point converged (a failed sample's
    row is NaN throughout, and is handed out as it is)."""
    def node(n):
        return np.zeros(x.shape[:-1], x.dtype) if n == 0 else x[..., n - 1]

    if r[0] == "v":
        return node(r[1])
    if r[0] == "dv":
        return node(r[1]) - node(r[2])
    v = x[..., ckt.mna_index("i", ckt.dev_names[r[1]])]
    if nan_is_error and np.any(np.isnan(v)):
        raise KeyError("branch current of '%s' was eliminated: observe it when building the circuit" % sym)
    return v


def _param_key(name):
    return tuple(str(x).lower() for x in name) if isinstance(name, (tuple, list)) else (str(name).lower(), None)


def _param_columns(params):
    return {_param_key(p): k for k, p in enumerate(params)}


def _param_column(cols, par):
    """Column of parameter `par` among the requested ones; a bare source name ("v1") also finds ("v1", "dc")."""
    pk = _param_key(par)
    if pk not in cols and pk[1:] == (None,):
        pk = (pk[0], "dc")
    if pk not in cols:
        raise KeyError("no sensitivity with respect to %r was requested" % (par,))
    return cols[pk]


def _nothing_to_hand_out(rc, status):
    """A batched solve failed altogether: anything but "some operating points failed" (-3 with at least one good sample)."""
    return rc != 0 and (rc != -3 or np.all(status != 0))


def _failure(what, rc, eng):
    return CedarError("%s failed (%s): %s" % (what, RETCODES.get(rc, rc), eng.ctx.last_error()))


def need_ac_source(ckt):
    if not any(ckt.source_ac):
        raise CedarError("AC analysis needs at least one source with an `ac` magnitude")


def _dense_eval(tt, pts, y, tq):
    """The BDF dense-output polynomials of a run at times `tq`: the step that ended at saved row i runs through its pts[i] newest rows."""
    y = np.asarray(y, float)
    out = np.empty(len(tq))
    for q, x in enumerate(tq):
        if x <= tt[0] or x >= tt[-1]:
            out[q] = y[0] if x <= tt[0] else y[-1]
            continue
        i = int(np.searchsorted(tt, x, side="left"))          # tt[i-1] < x <= tt[i]: the step that ended at row i covers x
        m = min(int(pts[i]), i + 1)
        rows = list(range(i - m + 1, i + 1))
        if m < 2 or len(set(tt[rows])) < m:
            out[q] = np.interp(x, tt[i - 1:i + 1], y[i - 1:i + 1]) if tt[i] > tt[i - 1] else y[i]
            continue
        acc = 0.0
        for a in rows:
            w = 1.0
            for b in rows:
                if b != a:
                    w *= (x - tt[b]) / (tt[a] - tt[b])
            acc += w * y[a]
        out[q] = acc
    return out


def _pchip_eval(tt, y, tq):
    """Shape-preserving cubic (PCHIP) through the saved rows at times `tq`, clipped to the run's span."""
    y = np.asarray(y, float)
    uniq = np.concatenate(([True], np.diff(tt) > 0)) if len(tt) > 1 else np.ones(len(tt), bool)   # restart steps repeat a time
    if uniq.sum() < 3:
        return np.interp(tq, tt, y)
    from scipy.interpolate import PchipInterpolator
    return PchipInterpolator(tt[uniq], y[uniq], extrapolate=False)(np.clip(tq, tt[0], tt[-1]))


class MeasureSens:
    """`sol.measure_sens` / the `sens` of `Solution.measure`: `ms["tpd", ("m1", "w")]` is d(measure)/d(parameter); `ms.array` the raw
    [n_meas][n_par] values in the order of `ms.names` and of the requested parameters."""

    def __init__(self, names, cols, array):
        self.names, self._cols, self.array = list(names), cols, np.asarray(array)

    def __getitem__(self, key):
        name, par = key
        if name not in self.names:
            raise KeyError("no measure named %r" % (name,))
        return float(self.array[self.names.index(name), _param_column(self._cols, par)])


class Measured(NamedTuple):
    """What `Solution.measure` returns: {name: value}, {name: status} (measure.STATUS) and a MeasureSens or None."""
    values: dict
    status: dict
    sens: object = None


class Solution:
    """Solution of one sample: time points, observables by name, retcode and stats.  A transient run with `measures=` also carries
    `measures[name]` and `measure_status[name]` (measure.py)."""
    measures = MappingProxyType({})          # (class-level, read-only empties: a run without measures= adds nothing to its solutions)
    measure_status = MappingProxyType({})

    def __init__(self, circuit, t, cols, x_final, rc, stats, params=None):
        self.circuit, self.t, self._cols, self.x_final = circuit, np.asarray(t), cols, x_final
        self.retcode = RETCODES.get(rc, str(rc))
        self.rc = rc
        self.stats = stats
        self.params = params or {}

    # -- symbolic indexing: "node_q" / "q" (node voltage), "r1.i" / "r1.v" (device current / voltage) --
    def _node_series(self, node):
        c = self.circuit
        n = c._n(node) if not isinstance(node, (int, np.integer)) else int(node)
        if n == 0:
            return np.zeros(len(self.t))
        key = ("v", n)
        if key in self._cols:
            return self._cols[key]
        if len(self.t) == 1 and self.x_final is not None:
            return np.array([self.x_final[n - 1]])
        raise KeyError("node '%s' was not observed" % node)

    def __getitem__(self, name):
        c = self.circuit
        node, i, fld = _split_sym(c, name)
        if node is not None:
            return self._node_series(node)
        v = self._node_series(c.dev_node[i][0]) - self._node_series(c.dev_node[i][1])
        if fld == "v":
            return v
        k = c.dev_kind[i]
        if k == DEV_R:
            return v / c.dev_par[i][0]
        if k in (DEV_V, DEV_L, DEV_VCVS):
            if ("i", i) in self._cols:
                return self._cols[("i", i)]
            if len(self.t) == 1 and self.x_final is not None:
                return np.array([self.x_final[c.mna_index("i", c.dev_names[i])]])
            raise KeyError("branch current of '%s' was not observed" % c.dev_names[i])
        if k == DEV_C:
            if len(self.t) < 2:
                return np.zeros(len(self.t))
            return c.dev_par[i][0] * np.gradient(v, self.t)  # post-processed derivative
        raise KeyError(name)

    def op(self, dev_name, index=-1, ctx=None):
        """Operating-point observables of a compiled Verilog-A instance at saved point `index` — `sol[sys.x1.gm]` for the
        variables a module declares with (* desc *) (src/vasim.jl:742-753).  Evaluated on the GPU from the node voltages."""
        c = self.circuit
        name = str(dev_name).lower()
        if name not in getattr(c, "va_instances", {}):
            raise KeyError("'%s' is not a compiled Verilog-A instance" % dev_name)
        i = c.dev_names.index(name)
        mid, ofs = c.dev_ipar[i]
        mod, _ = c.va_instances[name]
        v = [float(self._node_series(n)[index]) for n in c.dev_node[i][:len(mod.nodes)]]
        par = c.va_par[ofs:ofs + 2 * len(mod.params)]
        if ctx is None:
            from .engine import default_context   # the one place a result reaches for the GPU by itself, and only when asked to
            ctx = default_context()
        return ctx.va_opvars(mid, par, v, c.temp + 273.15, c.gmin)

    def default_name_map(self):
        """{solution key: column name} for every observed top-level node voltage — default_name_map (src/util.jl:239-260):
        the `node_` prefix is dropped and ground aliases are left out."""
        c = self.circuit
        out = {}
        for kind, idx in self._cols:
            if kind != "v":
                continue
            name = c.node_names[idx]
            if "." in name or name in ("0", "gnd"):
                continue
            out["node_" + name] = name
        return out

    def write_csv(self, path, name_map=None):
        """CSV.write(file, sol; name_map) (ext/CedarSimCSVExt.jl:13-19): column `t` then one column per mapped probe."""
        name_map = name_map or self.default_name_map()
        cols = [("t", self.t)] + [(name, self[key]) for key, name in name_map.items()]
        with open(path, "w") as f:
            f.write(",".join(n for n, _ in cols) + "\n")
            for i in range(len(self.t)):
                f.write(",".join(repr(float(v[i])) for _, v in cols) + "\n")
        return path

    def __call__(self, t, idxs=None):
        """`sol(t, idxs=…)` (test/gf180_dff.jl:29-33).  A run without a `saveat` grid carries, per accepted step, the number of
        newest saved points its BDF dense-output polynomial runs through (`ch_result_dense_points`): `sol(t)` evaluates exactly
        that polynomial — the value a `saveat` grid would have returned at t.  Results that are already on a `saveat` grid are
        interpolated between grid points by a shape-preserving cubic (PCHIP)."""
        names = idxs if isinstance(idxs, (list, tuple)) else [idxs]
        out = self._sample([self[n] for n in names], t)
        return out if isinstance(idxs, (list, tuple)) else out[0]

    def _sens_rows(self):
        """(parameters, {observable: rows[n_par][n_times]}) of a solution that carries sensitivity rows, else ((), None)."""
        return (), None

    def measure(self, measures, ctx=None):
        """Waveform measurements after the fact (measure.py: `when`, `delay`, ..., `parse_measure`) on this solution's own rows and
        dense points, on the GPU (ch_measure_rows): a `Measured` of {name: value}, {name: status} and, for a TranSensSolution, the
        measures' derivatives.  Needs every observable of the run (a Solution built by `tran`)."""
        from .measure import resolve_measures   # (measure imports this module)
        c = self.circuit
        params, srows = self._sens_rows()
        names, specs = resolve_measures(c, measures, None, bool(params))
        missing = [o for o in c.obs if o not in self._cols]
        if missing or not c.obs:
            raise CedarError("Solution.measure needs the rows of every observable of the run")
        values = np.stack([np.asarray(self._cols[o], float) for o in c.obs])[:, :, None]
        sens = np.stack([np.asarray(srows[o], float) for o in c.obs])[:, :, :, None] if params else None
        pts = self.stats.get("dense_points") if isinstance(self.stats, dict) else None
        if ctx is None:
            from .engine import default_context
            ctx = default_context()
        val, status, ds = ctx.measure_rows(self.t, values, specs, len(names), pts if pts is not None and len(pts) == len(self.t) else None, sens)
        return Measured({n: float(val[k, 0]) for k, n in enumerate(names)}, {n: int(status[k, 0]) for k, n in enumerate(names)},
                        MeasureSens(names, _param_columns(params), ds[:, :, 0]) if params else None)

    def _sample(self, rows, t):
        """Rows over self.t at the time(s) t: the dense-output polynomials where the run carries them, else PCHIP between grid points."""
        tt = np.asarray(self.t, float)
        tq = np.atleast_1d(np.asarray(t, float))
        pts = self.stats.get("dense_points") if isinstance(self.stats, dict) else None
        if pts is not None and len(pts) == len(tt) and np.any(np.asarray(pts) >= 2):
            out = [_dense_eval(tt, pts, y, tq) for y in rows]
        else:
            out = [_pchip_eval(tt, y, tq) for y in rows]
        if not np.ndim(t):
            out = [float(o[0]) for o in out]
        return out


class _SensRows:
    """`sol.sens` of a TranSensSolution: `sens["node_out", ("m1", "w")]` is the row of d(symbol)/d(parameter) over `sol.t`, and
    `sens(t, idxs=…, par=…)` samples it with the interpolation `Solution.__call__` uses for the states."""

    def __init__(self, sol, params, rows):
        self._sol, self.params, self._rows, self._col = sol, list(params), rows, _param_columns(params)

    def _row(self, key, k):
        if key not in self._rows:
            raise KeyError("%s was not observed" % (key,))
        return self._rows[key][k]

    def __getitem__(self, key):
        sym, par = key
        c, k = self._sol.circuit, _param_column(self._col, par)
        r = _resolve_sym(c, sym)
        nt = len(self._sol.t)
        if r[0] == "v":
            return np.zeros(nt) if r[1] == 0 else self._row(r, k)
        if r[0] == "dv":
            a, b = (np.zeros(nt) if n == 0 else self._row(("v", n), k) for n in r[1:])
            return a - b
        row = self._row(r, k)
        if np.any(np.isnan(row)) and self._sol.rc == 0:
            raise KeyError("branch current of '%s' was eliminated: observe it when building the circuit" % sym)
        return row

    def __call__(self, t, idxs=None, par=None):
        names = idxs if isinstance(idxs, (list, tuple)) else [idxs]
        out = self._sol._sample([self[n, par] for n in names], t)
        return out if isinstance(idxs, (list, tuple)) else out[0]


class TranSensSolution(Solution):
    """A transient Solution of one sample plus the derivatives of its observables with respect to the requested parameters along the
    waveform (direct method on the GPU, ch_tran_sens): `sol.sens["node_out", ("m1", "w")]` over `sol.t`, `sol.sens(t, idxs=…, par=…)` in
    between.  The derivative is that of the discrete solution on the step sequence the run took.  With `measures=`
    it also carries `measure_sens[name, par]`, the exact derivatives of the measures with respect to the same parameters."""
    measure_sens = None

    def __init__(self, circuit, t, cols, x_final, rc, stats, params, sens_params, sens_rows):
        super().__init__(circuit, t, cols, x_final, rc, stats, params)
        self.sens = _SensRows(self, sens_params, sens_rows)

    def _sens_rows(self):
        return tuple(self.sens.params), self.sens._rows


def dc_solution(ckt, x_row, rc, stats, params=None):
    """The one-point Solution of a DC operating point: node voltages and branch currents picked out of an MNA state row."""
    cols = {o: np.array([x_row[(o[1] - 1) if o[0] == "v" else ckt.mna_index("i", ckt.dev_names[o[1]])]]) for o in ckt.obs}
    return Solution(ckt, np.array([0.0]), cols, x_row, rc, stats, params)


class ACSolution:
    """Linearisation around the DC operating point, sampled on demand (ACSol, src/ac.jl:10-13)."""

    def __init__(self, circuit, eng, opts):
        self.circuit, self._eng, self._opts = circuit, eng, opts
        self.stats = None

    def freqresp(self, sym, omegas, sample=0):
        """Complex response of `sym` to the circuit's AC sources at angular frequencies `omegas` (rad/s)."""
        w = np.asarray(omegas, dtype=np.float64)
        rc, x, st = self._eng.ac(w / (2.0 * math.pi), self._opts)
        self.stats = st
        if rc != 0:
            raise _failure("AC analysis", rc, self._eng)
        return _pick(self.circuit, _resolve_sym(self.circuit, sym), sym, x[sample], True)

    def bode(self, sym, omegas, sample=0):
        h = self.freqresp(sym, omegas, sample)
        return np.abs(h), np.degrees(np.unwrap(np.angle(h))), np.asarray(omegas)


class ACMeasured:
    """One sample of `ac_measure`: `measures[name]`, `measure_status[name]` (acmeasure.STATUS) and, with `params`,
    `measure_sens[name, par]` — the exact derivatives of the discrete measures; `rc` is the sample's operating-point status and
    `params` its sweep point."""

    def __init__(self, circuit, names, val, status, sens, par_names, rc, stats, point_params=None):
        self.circuit, self.rc, self.retcode, self.stats, self.params = circuit, int(rc), RETCODES.get(int(rc), str(rc)), stats, point_params
        self.measures = {n: float(val[k]) for k, n in enumerate(names)}
        self.measure_status = {n: int(status[k]) for k, n in enumerate(names)}
        self.measure_sens = MeasureSens(names, _param_columns(par_names), sens) if par_names else None


class _RowSens:
    """`LoopGainSolution.sens`: `sens["r2"]`, `sens[("m1", "w")]` is dT/d(parameter) [n_freq], complex; `sens.array` the raw
    [n_freq][n_par] values in the order of the requested parameters."""

    def __init__(self, cols, array):
        self._cols, self.array = cols, np.asarray(array)

    def __getitem__(self, par):
        return self.array[:, _param_column(self._cols, par)]


class LoopGainSolution:
    """One sample of `loop_gain`: `freqs` (Hz), the loop gain `T` [n_freq] (complex) at the probe and, with `params`, `sens[par]` =
    dT/d(parameter) [n_freq]; with `measures`, `measures[name]`, `measure_status[name]` (acmeasure.STATUS) and `measure_sens[name, par]`
    — the exact derivatives of the discrete measures; `rc` is the sample's operating-point status and `params` its sweep point."""

    def __init__(self, circuit, probe, freqs, T, dT, par_names, names, val, status, sens, rc, stats, point_params=None):
        self.circuit, self.probe, self.rc, self.retcode, self.stats, self.params = circuit, probe, int(rc), RETCODES.get(int(rc), str(rc)), stats, point_params
        self.freqs, self.T = np.asarray(freqs, dtype=np.float64), T
        cols = _param_columns(par_names)
        self.sens = _RowSens(cols, dT) if par_names else None
        self.measures = {n: float(val[k]) for k, n in enumerate(names)}
        self.measure_status = {n: int(status[k]) for k, n in enumerate(names)}
        self.measure_sens = MeasureSens(names, cols, sens) if par_names and names else None


class _MatSens:
    """`NetParamsSolution.sens_S` (and `_Y`, `_Z`): `sens_S["r2"]`, `sens_S[("m1", "w")]` is dS/d(parameter) [n_freq][P][P], complex;
    `.array` the raw [n_freq][n_par][P][P] values in the order of the requested parameters."""

    def __init__(self, cols, array):
        self._cols, self.array = cols, np.asarray(array)

    def __getitem__(self, par):
        return self.array[:, _param_column(self._cols, par)]


class NetParamsSolution:
    """One sample of `net_params`: `freqs` (Hz), `ports` (names, port 1 first), `z0` (one reference impedance per port) and the
    matrices `S`, `Y`, `Z` [n_freq][P][P] (complex): entry [j][k] is the response at port j + 1 to port k + 1, also `s(2, 1)`,
    `y(1, 1)`, `z(1, 2)` with 1-based port numbers ([n_freq]).  With `params`, `sens_S[par]`, `sens_Y[par]`, `sens_Z[par]`
    [n_freq][P][P]; with `measures`, `measures[name]`, `measure_status[name]` (acmeasure.STATUS) and `measure_sens[name, par]` — the
    exact derivatives of the discrete measures; `rc` is the sample's operating-point status and `params` its sweep point.  Z (and
    sens_Z) is NaN at a frequency where Y is singular, as it is for a series-only network."""

    def __init__(self, circuit, ports, z0, freqs, X, dX, par_names, names, val, status, sens, rc, stats, point_params=None):
        self.circuit, self.rc, self.retcode, self.stats, self.params = circuit, int(rc), RETCODES.get(int(rc), str(rc)), stats, point_params
        self.ports, self.z0, self.freqs = tuple(ports), np.asarray(z0, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
        self.S, self.Y, self.Z = X.get("S"), X.get("Y"), X.get("Z")
        cols = _param_columns(par_names)
        self.sens_S, self.sens_Y, self.sens_Z = ((_MatSens(cols, dX[k]) if k in dX else None) for k in "SYZ") if par_names and dX else (None, None, None)
        self.measures = {n: float(val[k]) for k, n in enumerate(names)}
        self.measure_status = {n: int(status[k]) for k, n in enumerate(names)}
        self.measure_sens = MeasureSens(names, cols, sens) if par_names and names else None

    def _entry(self, M, j, k):
        P = len(self.ports)
        if not (1 <= j <= P and 1 <= k <= P):
            raise CedarError("port numbers run from 1 to %d" % P)
        return M[:, j - 1, k - 1]

    def s(self, j, k):
        return self._entry(self.S, j, k)

    def y(self, j, k):
        return self._entry(self.Y, j, k)

    def z(self, j, k):
        return self._entry(self.Z, j, k)

    def write_touchstone(self, path, fmt="RI"):
        """S as Touchstone text (`.sNp`, version 1): the option line `# Hz S RI R z0`, then per frequency the entries as real /
        imaginary pairs — row-wise (S11 S12 ... ; at most four pairs on a line), but for two ports in the order S11 S21 S12 S22 the
        format prescribes.  One reference impedance serves the file, so unequal `z0` are refused."""
        if str(fmt).upper() != "RI":
            raise CedarError("write_touchstone: only the RI format is written")
        if np.any(self.z0 != self.z0[0]):
            raise CedarError("write_touchstone: a Touchstone file has one reference impedance; the ports' z0 differ")
        P = len(self.ports)
        with open(path, "w") as out:
            out.write("! %d-port S-parameters, ports: %s\n" % (P, " ".join(self.ports)))
            out.write("# Hz S RI R %s\n" % repr(float(self.z0[0])))
            for f, M in zip(self.freqs, self.S):
                M = M.T if P == 2 else M
                rows = [["%s %s" % (repr(float(v.real)), repr(float(v.imag))) for v in r] for r in M]
                if P <= 2:
                    out.write("%s %s\n" % (repr(float(f)), " ".join(p for r in rows for p in r)))
                    continue
                for j, r in enumerate(rows):
                    for q in range(0, P, 4):
                        out.write("%s%s\n" % (repr(float(f)) + " " if j == 0 and q == 0 else "  ", " ".join(r[q:q + 4])))


def _noise_measure(sol, ctx, measures, omegas, output, sens_of=None, params=()):
    """`Measured` of frequency-domain measures over the PSD rows of a noise solution (ch_freq_measure_rows): one row per distinct
    output among the signals (`onoise` is `output`); sens_of(sym) gives dS/dp[n_freq][n_par] of an output, or None."""
    from .acmeasure import resolve_fmeasures   # (acmeasure imports this module)
    w = np.ascontiguousarray(omegas, dtype=np.float64).reshape(-1)
    outs = []

    def row_of(sym, name):
        sym = output if sym is None else sym
        if sym is None:
            raise CedarError("measure '%s': onoise needs `output=`, the symbol the noise is referred to" % name)
        if isinstance(sym, (tuple, list)):
            raise CedarError("measure '%s': noise output must be a node voltage or a branch current" % name)
        key = str(sym).lower()
        if key not in outs:
            outs.append(key)
        return outs.index(key), -1, 1.0

    res = resolve_fmeasures(measures, row_of)
    values = np.array([sol.psd(o, w) for o in outs], dtype=np.complex128)[:, :, None]
    sens = None
    if sens_of is not None and params:
        sens = np.array([np.transpose(sens_of(o, w)) for o in outs], dtype=np.complex128)[:, :, :, None]   # [n_out][n_par][n_freq][1]
    val, status, ds = ctx.freq_measure_rows(w / (2.0 * math.pi), values, res.specs, len(res.names), sens)
    val, ds = res.apply(val, ds)
    return Measured({n: float(val[k, 0]) for k, n in enumerate(res.names)}, {n: int(status[k, 0]) for k, n in enumerate(res.names)},
                    MeasureSens(res.names, _param_columns(params), ds[:, :, 0]) if ds is not None else None)


def _name_model_card(e, circuit):
    """A refusal of the MOSFET noise names a model card by its index — the engine knows no names; the text "model card <index>"
    is written by b4n_table (csrc/ch_noise_params.hpp), which says so at the string: add the card's name."""
    m = re.search(r"model card (\d+)", str(e))
    if m and int(m.group(1)) < len(circuit.model_names):
        return CedarError("%s (model '%s')" % (e, circuit.model_names[int(m.group(1))]))
    return e


class NoiseRun:
    """What the samples of a swept noise analysis share: one batched ch_noise / ch_noise_ex per (output, frequency list,
    contributions or not), run when the first sample asks and kept until another is asked for."""

    def __init__(self, eng, opts, device_noise):
        self.eng, self.opts, self.device_noise = eng, opts, bool(device_noise)
        self._key, self._res = None, None

    def solve(self, kind, index, freqs_hz, contributions):
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64)
        key = (kind, index, f.tobytes(), bool(contributions))
        if key != self._key:
            if self.device_noise or contributions:
                self._res = self.eng.noise_ex(kind, index, f, self.opts, mos_noise=self.device_noise, contributions=contributions)
            else:
                rc, out, st = self.eng.noise(kind, index, f, self.opts)
                self._res = (rc, out, None, st)
            self._key = key
        return self._res


class NoiseSolution:
    """Output-noise analysis around the DC operating point (NoiseSol, src/ac.jl:15-20).  One point of a swept analysis is sample
    `sample` of the batch behind `run`; a single circuit has no run and calls the engine itself."""

    def __init__(self, circuit, eng, opts, device_noise=False, run=None, sample=0, params=None):
        self.circuit, self._eng, self._opts, self.device_noise = circuit, eng, opts, bool(device_noise)
        self._run, self._sample, self.params = run, int(sample), params
        self.stats = None

    def _output(self, sym):
        r = _resolve_sym(self.circuit, sym)
        if r[0] == "dv":
            raise CedarError("noise output must be a node voltage or a branch current")
        return (0 if r[0] == "v" else 1), r[1]

    def _failure(self, rc):
        return _name_model_card(_failure("noise analysis", rc, self._eng), self.circuit)

    def _solve(self, kind, index, freqs_hz, contributions):
        """(psd[S][n_freq], contrib[S][n_freq][n_src] or None) of the engine call behind this solution."""
        if self._run is not None:
            rc, out, contrib, st = self._run.solve(kind, index, freqs_hz, contributions)
        elif self.device_noise or contributions:
            rc, out, contrib, st = self._eng.noise_ex(kind, index, freqs_hz, self._opts, mos_noise=self.device_noise, contributions=contributions)
        else:
            (rc, out, st), contrib = self._eng.noise(kind, index, freqs_hz, self._opts), None
        self.stats = st
        if rc != 0:
            raise self._failure(rc)
        return out, contrib

    def psd(self, sym, omegas, sample=None):
        """Power spectral density of `sym` (V²/Hz or A²/Hz) at angular frequencies `omegas` — PSD(noise, sym, ωs).  With
        device_noise the BSIM4 MOSFETs' channel thermal and flicker noise is part of it."""
        kind, index = self._output(sym)
        w = np.asarray(omegas, dtype=np.float64)
        out, _ = self._solve(kind, index, w / (2.0 * math.pi), False)
        return out[self._sample if sample is None else sample]

    def contributions(self, sym, omegas, sample=None):
        """Every noise source's share of `psd(sym, omegas)` (ngspice: the per-device lines of .noise):
        {(device name, source): psd array}, source = "thermal" for a resistor, "id" (channel thermal noise) and "1overf" (flicker
        noise) for a MOSFET, "noise<k>" for the k-th source of a compiled module.  The shares sum to the PSD."""
        kind, index = self._output(sym)
        sample = self._sample if sample is None else sample
        w = np.asarray(omegas, dtype=np.float64)
        _, contrib = self._solve(kind, index, w / (2.0 * math.pi), True)
        src = self._eng.noise_sources(kind, index, sample)
        out, seen = {}, {}
        for k, d in enumerate(src["dev"]):
            j = seen[d] = seen.get(d, -1) + 1
            dk = self.circuit.dev_kind[d]
            if dk == DEV_MOS and not self.device_noise:
                continue
            if dk not in (DEV_R, DEV_MOS) and src["pwr"][k] == 0.0:
                continue   # an unused entry of a compiled module
            label = "thermal" if dk == DEV_R else (("id", "1overf")[j] if dk == DEV_MOS else "noise%d" % j)
            out[(self.circuit.dev_names[d], label)] = contrib[sample, :, k].copy()
        return out

    def measure(self, measures, omegas, output=None):
        """Frequency-domain measurements (acmeasure.py: `finteg`, `ffind_at`, `fwhen`, ..., `parse_ac_measure`) of this solution's PSD
        rows at angular frequencies `omegas`, on the GPU (ch_freq_measure_rows): a `Measured` of {name: value}, {name: status}.  A
        signal names the output its PSD is referred to; `onoise` of a card is `output`."""
        return _noise_measure(self, self._eng.ctx, measures, omegas, output)

    def summary(self, sym, omegas, sample=None):
        """Noise per device, largest first: [(device name, value)], value = the device's sources integrated over the band of
        `omegas` (trapezoid rule over frequency in Hz: V² or A²), or its spot noise (V²/Hz) when `omegas` is one frequency."""
        w = np.atleast_1d(np.asarray(omegas, dtype=np.float64))
        per = {}
        for (name, _), y in self.contributions(sym, w, sample).items():
            f = w / (2.0 * math.pi)
            v = float(y[0]) if len(w) == 1 else float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(f)))
            per[name] = per.get(name, 0.0) + v
        return sorted(per.items(), key=lambda kv: -kv[1])


class SensSolution:
    """DC operating point of one sample and its derivatives with respect to the requested parameters (direct method on the GPU,
    ch_dc_sens): `s["node_out", "r1"]`, `s["v1.i", ("m1", "w")]`; `s.op` is the operating-point Solution, `s.sens` the raw
    [n_par][n_mna] array in the order of `s.params`."""

    def __init__(self, circuit, params, sens, op, rc):
        self.circuit, self.params, self.sens, self.op = circuit, list(params), np.asarray(sens), op
        self.rc, self.retcode = rc, RETCODES.get(rc, str(rc))
        self._col = _param_columns(self.params)

    def __getitem__(self, key):
        sym, par = key
        row = self.sens[_param_column(self._col, par)]
        return float(_pick(self.circuit, _resolve_sym(self.circuit, sym), sym, row, self.rc == 0))


def mag_phase_sens(h, dh):
    """d|H|/dp and d(arg H)/dp (radians) from a complex response `h` and its derivative `dh` = dH/dp:
    (Re(conj(h) dh) / |h|, Im(dh / h))."""
    h, dh = np.asarray(h, complex), np.asarray(dh, complex)
    return np.real(np.conj(h) * dh) / np.abs(h), np.imag(dh / h)


class ACSensRun:
    """One engine circuit (one sample per sweep point) behind the ACSensSolutions of its samples: a ch_ac_sens call per distinct
    frequency list, shared by all of them, and one unchecked DC solve for their `.op`, made when first asked for."""

    def __init__(self, eng, dc_kw, slot_ids, rel_step, abs_step):
        self.eng, self.dc_kw, self.slot_ids, self.rel_step, self.abs_step = eng, dict(dc_kw), list(slot_ids), rel_step, abs_step
        self._key, self._res, self._op, self.stats = None, None, None, None

    def at(self, omegas):
        """(x_ac, dc_sens, sens, status) of all samples at `omegas`."""
        w = np.ascontiguousarray(omegas, dtype=np.float64).reshape(-1)
        if self._key is None or self._key != w.tobytes():
            rc, x, dsens, sens, status, st = self.eng.ac_sens(self.slot_ids, w / (2.0 * math.pi), dc_opts(**self.dc_kw), rel_step=self.rel_step,
                                                              abs_step=self.abs_step)
            self.stats = st
            if _nothing_to_hand_out(rc, status):
                raise _failure("AC sensitivity analysis", rc, self.eng)
            self._key, self._res = w.tobytes(), (x, dsens, sens, status)
        return self._res

    def dc_sens(self):
        """(dc_sens, status) of all samples: of the last frequency list asked for — they do not depend on it — or of a solve at 0 Hz."""
        _, dsens, _, status = self._res if self._res is not None else self.at([0.0])
        return dsens, status

    def op(self):
        if self._op is None:
            rc, x, status, st = self.eng.dc(dc_opts(**self.dc_kw), check=False)
            self._op = (x, status, st)
        return self._op


class ACSensSolution:
    """Small-signal response of one sample and its derivatives with respect to the requested parameters (direct method on the GPU,
    ch_ac_sens), sampled on demand like ACSolution: `.freqresp(sym, ωs)` is H, `.sens(sym, par, ωs)` the complex dH/dp
    (`mag_phase_sens(H, dH)` turns the pair into d|H|/dp and dφ/dp); `.op` is the operating-point Solution and `.dc_sens` the
    SensSolution of the same parameters."""

    def __init__(self, circuit, run, params, sample=0, point_params=None):
        self.circuit, self._run, self.params, self._s, self._pp = circuit, run, list(params), sample, point_params
        self._col = _param_columns(self.params)

    @property
    def stats(self):
        return self._run.stats

    def _picked(self, sym, x):
        return _pick(self.circuit, _resolve_sym(self.circuit, sym), sym, x, True)

    def freqresp(self, sym, omegas):
        return self._picked(sym, self._run.at(omegas)[0][self._s])

    def sens(self, sym, par, omegas):
        k = _param_column(self._col, par)
        return self._picked(sym, self._run.at(omegas)[2][self._s][:, k, :])

    @property
    def op(self):
        x, status, st = self._run.op()
        return dc_solution(self.circuit, x[self._s], int(status[self._s]), st, self._pp)

    @property
    def dc_sens(self):
        dsens, status = self._run.dc_sens()
        return SensSolution(self.circuit, self.params, dsens[self._s], self.op, int(status[self._s]))


class NoiseSensRun:
    """One engine circuit (one sample per sweep point) behind the NoiseSensSolutions of its samples: a ch_noise_sens call per distinct
    (output, frequency list), shared by all of them, and one unchecked DC solve for their `.op`, made when first asked for."""

    def __init__(self, circuit, eng, dc_kw, slot_ids, rel_step, abs_step, device_noise):
        self.circuit, self.eng, self.dc_kw, self.slot_ids = circuit, eng, dict(dc_kw), list(slot_ids)
        self.rel_step, self.abs_step, self.device_noise = rel_step, abs_step, bool(device_noise)
        self._key, self._res, self._op, self.stats = None, None, None, None

    def at(self, kind, index, omegas):
        """(psd, dpsd, dc_sens, status) of all samples for the output (kind, index) at `omegas`."""
        w = np.ascontiguousarray(omegas, dtype=np.float64).reshape(-1)
        key = (kind, index, w.tobytes())
        if key != self._key:
            rc, psd, dpsd, dsens, status, st = self.eng.noise_sens(kind, index, self.slot_ids, w / (2.0 * math.pi), dc_opts(**self.dc_kw),
                                                                   mos_noise=self.device_noise, rel_step=self.rel_step, abs_step=self.abs_step)
            self.stats = st
            if _nothing_to_hand_out(rc, status):
                raise _name_model_card(_failure("noise sensitivity analysis", rc, self.eng), self.circuit)
            self._key, self._res = key, (psd, dpsd, dsens, status)
        return self._res

    def dc_sens(self):
        """(dc_sens, status) of all samples: of the last call — they depend on neither output nor frequencies — or of one on ground at 0 Hz."""
        _, _, dsens, status = self._res if self._res is not None else self.at(0, 0, [0.0])
        return dsens, status

    def op(self):
        if self._op is None:
            rc, x, status, st = self.eng.dc(dc_opts(**self.dc_kw), check=False)
            self._op = (x, status, st)
        return self._op


class NoiseSensSolution:
    """Output-noise PSD of one sample and its derivatives with respect to the requested parameters (direct method on the adjoint
    system on the GPU, ch_noise_sens), sampled on demand like NoiseSolution: `.psd(sym, ωs)` is S, `.sens(sym, par, ωs)` dS/dp,
    `.log_sens` (p/S)·dS/dp; `.integrated` / `.integrated_sens` apply the trapezoid rule over Hz of `NoiseSolution.summary` to S and
    to dS/dp; `.op` is the operating-point Solution and `.dc_sens` the SensSolution of the same parameters."""

    def __init__(self, circuit, run, params, sample=0, point_params=None):
        self.circuit, self._run, self.params, self._s, self._pp = circuit, run, list(params), sample, point_params
        self.device_noise = run.device_noise
        self._col = _param_columns(self.params)

    @property
    def stats(self):
        return self._run.stats

    def _at(self, sym, omegas):
        r = _resolve_sym(self.circuit, sym)
        if r[0] == "dv":
            raise CedarError("noise output must be a node voltage or a branch current")
        return self._run.at(0 if r[0] == "v" else 1, r[1], omegas)

    def psd(self, sym, omegas):
        return self._at(sym, omegas)[0][self._s]

    def sens(self, sym, par, omegas):
        """dS/dp of the PSD of `sym` at angular frequencies `omegas`."""
        return self._at(sym, omegas)[1][self._s][:, _param_column(self._col, par)]

    def _value(self, par):
        """The parameter's value at this sample's point: the field of the sample's circuit that the slot addresses."""
        c = self.circuit
        kind, a, b = c.slots[self._run.slot_ids[_param_column(self._col, par)]]
        return float({SLOT_DEV_PAR: lambda: c.dev_par[a][b], SLOT_DEV_MULT: lambda: c.dev_mult[a], SLOT_MODEL_PAR: lambda: c.models[a][b],
                      SLOT_SRC_DC: lambda: c.sources[a][0], SLOT_SRC_PAR: lambda: c.sources[a][1].par[b], SLOT_TEMP: lambda: c.temp,
                      SLOT_GMIN: lambda: c.gmin, SLOT_VA_PAR: lambda: c.va_par[a]}[kind]())

    def log_sens(self, sym, par, omegas):
        """(p/S)·dS/dp: the relative change of the PSD per relative change of the parameter."""
        return self._value(par) * self.sens(sym, par, omegas) / self.psd(sym, omegas)

    @staticmethod
    def _band(y, omegas):
        f = np.atleast_1d(np.asarray(omegas, dtype=np.float64)) / (2.0 * math.pi)
        return float(y[0]) if len(f) == 1 else float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(f)))

    def measure(self, measures, omegas, output=None):
        """As `NoiseSolution.measure`, with the measures' exact derivatives with respect to this solution's parameters
        (`.sens[name, par]`) out of the dS/dp rows."""
        return _noise_measure(self, self._run.eng.ctx, measures, omegas, output, lambda sym, w: self._at(sym, w)[1][self._s], self.params)

    def integrated(self, sym, omegas):
        """The PSD over the band of `omegas` (trapezoid rule over frequency in Hz: V² or A²); its spot value for one frequency."""
        return self._band(self.psd(sym, np.atleast_1d(omegas)), omegas)

    def integrated_sens(self, sym, par, omegas):
        """d(integrated)/dp: the same rule applied to dS/dp."""
        return self._band(self.sens(sym, par, np.atleast_1d(omegas)), omegas)

    @property
    def op(self):
        x, status, st = self._run.op()
        return dc_solution(self.circuit, x[self._s], int(status[self._s]), st, self._pp)

    @property
    def dc_sens(self):
        dsens, status = self._run.dc_sens()
        return SensSolution(self.circuit, self.params, dsens[self._s], self.op, int(status[self._s]))
