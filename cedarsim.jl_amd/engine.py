"""ctypes binding of libcedarhip.so — the C-ABI of include/cedarhip.h.

The library is built in-tree (cedarsim.jl_amd/lib/libcedarhip.so) by `__graft_entry__.build()` or
`make -C cedarsim.jl_amd/csrc`.  There is no CPU fallback: if the library is missing, or no HIP
device is present, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

from . import bsim4_params as _B4
from .acmeasure import ChFMeasureSpec
from .measure import ChMeasureSpec
from .circuit import (ChDcOpts, ChDesc, ChInfo, ChSensOpts, ChStats, ChTranOpts, CedarError, RETCODES, dc_opts, sens_opts, tran_opts)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", os.environ.get("CEDARHIP_LIB", "libcedarhip.so"))  # CEDARHIP_LIB: diagnostic builds
_pf64 = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_vp, _str, _int, _i32, _i64, _f64 = C.c_void_p, C.c_char_p, C.c_int, C.c_int32, C.c_int64, C.c_double
_dco, _sts, _sno = C.POINTER(ChDcOpts), C.POINTER(ChStats), C.POINTER(ChSensOpts)
_msp = C.POINTER(ChMeasureSpec)
_fmsp = C.POINTER(ChFMeasureSpec)


class ChNoiseOpts(C.Structure):
    """ch_noise_opts of include/cedarhip.h."""
    _fields_ = [("mos_noise", C.c_int32)]


# CH_B4N_* of include/cedarhip.h: the BSIM4 noise parameters in the order of a ch_set_mos_noise row
MOS_NOISE_PARAMS = tuple(_B4.NOISE)
# the operand row of a MOSFET's noise records (ch_noise_sources, mos_operands): enum B4NOp of csrc/ch_b4_noise.hpp
# (tests/test_host_b4_noise.py holds this tuple, B4.NOISE and the two C enums to each other)
MOS_NOISE_OPERANDS = ("ids", "ueff", "vgsteff", "abulk", "vdseff", "vds", "rds", "esat", "litl", "leff", "weffnf", "coxe", "cdep0", "cit", "vtm", "qinv")

# Every function include/cedarhip.h declares: name -> (restype, argtypes).  The one place the C ABI is written down on this side.
_PROTOTYPES = {
    "ch_dc_opts_default": (None, [_dco]),
    "ch_tran_opts_default": (None, [C.POINTER(ChTranOpts)]),
    "ch_create": (_vp, [_int, _str, C.c_size_t]),
    "ch_destroy": (None, [_vp]),
    "ch_last_error": (_str, [_vp]),
    "ch_circuit_build": (_vp, [_vp, C.POINTER(ChDesc)]),
    "ch_circuit_free": (None, [_vp]),
    "ch_circuit_info": (_int, [_vp, C.POINTER(ChInfo)]),
    "ch_circuit_maps": (_int, [_vp, _pi32, _pi32, _pi32]),
    "ch_set_samples": (_int, [_vp, _i32]),
    "ch_set_params": (_int, [_vp, _i32, _i32, _i32, _pi32, _pf64]),
    "ch_dc": (_int, [_vp, _dco, _pf64, _pi32, _sts]),
    "ch_tran": (_int, [_vp, _f64, _f64, C.POINTER(ChTranOpts), C.POINTER(_vp)]),
    "ch_result_n_times": (_i64, [_vp]),
    "ch_result_times": (_pf64, [_vp]),
    "ch_result_dense_points": (_pi32, [_vp]),
    "ch_result_device_values": (_int, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "ch_result_values": (_pf64, [_vp]),
    "ch_result_final_state": (_pf64, [_vp]),
    "ch_result_stats": (_int, [_vp, _sts]),
    "ch_result_status": (_int, [_vp]),
    "ch_result_free": (None, [_vp]),
    "ch_eval": (_int, [_vp, _i32, _pf64, _f64, _f64, _i32, _pf64, _pf64, _pf64]),
    "ch_ac": (_int, [_vp, _dco, _i32, _pf64, _pf64, _sts]),
    "ch_noise": (_int, [_vp, _dco, _i32, _i32, _i32, _pf64, _pf64, _sts]),
    "ch_sens_opts_default": (None, [_sno]),
    "ch_dc_sens": (_int, [_vp, _dco, _i32, _pi32, _sno, _pf64, _pf64, _pi32, _sts]),
    "ch_ac_sens": (_int, [_vp, _dco, _i32, _pi32, _sno, _i32, _pf64, _pf64, _pf64, _pf64, _pi32, _sts]),
    "ch_mos_eval": (_int, [_vp, _i32, _pf64, _pf64]),
    "ch_mos_eval_quad": (_int, [_vp, _i32, _pf64, _pf64]),
    "ch_bsim4_npar": (_i32, []),
    "ch_bsim4_param_name": (_str, [_i32]),
    "ch_bsim4_param_ignored": (_i32, [_str]),
    "ch_version": (_str, []),
    "ch_bench_triad": (_int, [_vp, _i64, _i32, _pf64]),
    "ch_bench_fp64": (_int, [_vp, _i32, _pf64]),
    "ch_va_n_modules": (_i32, []),
    "ch_va_find": (_i32, [_str]),
    "ch_va_module_name": (_str, [_i32]),
    "ch_va_module_info": (_i32, [_i32, _pi32, _pi32, _pi32]),
    "ch_va_node_name": (_str, [_i32, _i32]),
    "ch_va_param_name": (_str, [_i32, _i32]),
    "ch_va_eval": (_int, [_vp, _i32, _pf64, _pf64, _f64, _f64, _pf64]),
    "ch_va_n_opvars": (_i32, [_i32]),
    "ch_va_opvar_name": (_str, [_i32, _i32]),
    "ch_va_opvars": (_int, [_vp, _i32, _pf64, _pf64, _f64, _f64, _pf64]),
    "ch_debug_poison_lds": (_int, [_vp]),
    "ch_debug_math": (_int, [_vp, _i32, _i32, _pf64, _pf64]),
    "ch_tran_sens": (_int, [_vp, _f64, _f64, C.POINTER(ChTranOpts), _i32, _pi32, _sno, C.POINTER(_vp)]),
    "ch_result_n_par": (_i32, [_vp]),
    "ch_result_sens": (_pf64, [_vp]),
    "ch_set_mos_noise": (_int, [_vp, _i32, _pf64]),
    "ch_noise_sens": (_int, [_vp, _dco, C.POINTER(ChNoiseOpts), _i32, _pi32, _sno, _i32, _i32, _i32, _pf64, _pf64, _pf64, _pf64, _pi32, _sts]),
    "ch_noise_ex": (_int, [_vp, _dco, C.POINTER(ChNoiseOpts), _i32, _i32, _i32, _pf64, _pf64, _pf64, _sts]),
    "ch_noise_sources": (_int, [_vp, _i32, _i32, _i32, _pi32, _pi32, _pi32, _pi32, _pf64, _pf64, _pf64]),
    "ch_measure_rows": (_int, [_vp, _i64, _pf64, _pi32, _i32, _i32, _pf64, _i32, _pf64, _i32, _msp, _pf64, _pf64, _pi32]),
    "ch_result_measure": (_int, [_vp, _i32, _msp, _pf64, _pf64, _pi32]),
    "ch_freq_measure_rows": (_int, [_vp, _i32, _pf64, _i32, _i32, _pf64, _i32, _pf64, _i32, _fmsp, _pf64, _pf64, _pi32]),
    "ch_ac_measure": (_int, [_vp, _dco, _i32, _pi32, _sno, _i32, _pf64, _i32, _fmsp, _pf64, _pf64, _pi32, _pi32, _sts]),
    "ch_loop_gain": (_int, [_vp, _dco, _i32, _i32, _pi32, _sno, _i32, _pf64, _pf64, _pf64, _i32, _fmsp, _pf64, _pf64, _pi32, _pi32, _sts]),
    "ch_net_params": (_int, [_vp, _dco, _i32, _pi32, _pf64, _i32, _pi32, _sno, _i32, _pf64, _pf64, _pf64, _pf64, _pf64, _pf64, _pf64, _i32, _fmsp, _pf64, _pf64, _pi32, _pi32,
                             _sts]),
}
EXPORTS = list(_PROTOTYPES)

_lib = None


def load_library():
    """Load libcedarhip.so and declare every prototype.  Raises if the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libcedarhip.so is not built (%s missing): run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C cedarsim.jl_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(_pf64)


def _v8(v_nodes):
    """Node voltages of one Verilog-A instance, zero-padded to the 8 terminals the wide stamp has."""
    v = np.zeros(8)
    v[:len(v_nodes)] = v_nodes
    return v


class Context:
    """One per GPU (one process per GPU)."""

    def __init__(self, device_id=0):
        self.L = load_library()
        buf = C.create_string_buffer(512)
        self.h = self.L.ch_create(device_id, buf, 512)
        if not self.h:
            raise RuntimeError("ch_create failed: %s" % buf.value.decode())
        self.device_id = device_id

    def last_error(self):
        return self.L.ch_last_error(self.h).decode()

    def _call(self, name, *args):
        """`name(ctx, *args)` of the library; a non-zero return raises with the context's error text."""
        if getattr(self.L, name)(self.h, *args) != 0:
            raise RuntimeError("%s failed: %s" % (name, self.last_error()))

    def fp64_tflops(self, iters=3):
        """Measured vector fp64 FMA peak of this GPU in TFLOP/s (measurement utility)."""
        out = C.c_double(0.0)
        self._call("ch_bench_fp64", int(iters), C.byref(out))
        return out.value

    def va_eval(self, module_id, par_and_given, v_nodes, temperature_k=300.15, gmin=1e-12):
        """One compiled Verilog-A module on the GPU: the 144-double wide stamp [I(8)|Q(8)|G(8x8)|C(8x8)]."""
        p = np.ascontiguousarray(par_and_given, dtype=np.float64)
        out = np.zeros(144)
        self._call("ch_va_eval", int(module_id), _p(p), _p(_v8(v_nodes)), float(temperature_k), float(gmin), _p(out))
        return out

    def va_opvars(self, module_id, par_and_given, v_nodes, temperature_k=300.15, gmin=1e-12):
        """{name: value} of the (* desc *) observables of a compiled module at the given node voltages (on the GPU)."""
        n = self.L.ch_va_n_opvars(int(module_id))
        p = np.ascontiguousarray(par_and_given, dtype=np.float64)
        out = np.zeros(max(1, n))
        self._call("ch_va_opvars", int(module_id), _p(p), _p(_v8(v_nodes)), float(temperature_k), float(gmin), _p(out))
        return {self.L.ch_va_opvar_name(int(module_id), k).decode(): float(out[k]) for k in range(n)}

    def debug_math(self, which, x):
        """Test hook: the device's own exp (which=0), ln (1) and the BSIM4 code's ln (2) over a vector (ch_debug_math)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        self._call("ch_debug_math", int(which), len(x), _p(x), _p(y))
        return y

    def poison_lds(self):
        """Test hook: leave every CU's LDS full of garbage (ch_debug_poison_lds)."""
        self._call("ch_debug_poison_lds")

    def triad_gbps(self, n_doubles=1 << 27, iters=5):
        """Measured STREAM-triad bandwidth of this GPU in GB/s (measurement utility)."""
        out = C.c_double(0.0)
        self._call("ch_bench_triad", int(n_doubles), int(iters), C.byref(out))
        return out.value

    def measure_rows(self, t, values, specs, n_meas, dense_points=None, sens=None):
        """ch_measure_rows: measures of any rows.  values[n_rows][n_times][S], sens[n_rows][n_par][n_times][S] or None, specs a ctypes
        array of ch_measure_spec (measure.resolve_measures): (value[n_meas][S], status[n_meas][S], sens[n_meas][n_par][S] or None)."""
        t = np.ascontiguousarray(t, dtype=np.float64)
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 3 or v.shape[1] != len(t):
            raise CedarError("measure_rows: values must be [n_rows][n_times][n_samples]")
        n_rows, _, S = v.shape
        dp = None if dense_points is None else np.ascontiguousarray(dense_points, dtype=np.int32)
        sn = None if sens is None else np.ascontiguousarray(sens, dtype=np.float64)
        n_par = 0 if sn is None else sn.shape[1]
        if sn is not None and sn.shape != (n_rows, n_par, len(t), S):
            raise CedarError("measure_rows: sens must be [n_rows][n_par][n_times][n_samples]")
        val, status = np.full((n_meas, S), np.nan), np.zeros((n_meas, S), np.int32)
        out_s = np.full((n_meas, n_par, S), np.nan) if sn is not None else None
        rc = self.L.ch_measure_rows(self.h, len(t), _p(t), dp.ctypes.data_as(_pi32) if dp is not None else None, n_rows, S, _p(v), n_par,
                                    _p(sn) if sn is not None else None, n_meas, specs, _p(val), _p(out_s) if out_s is not None else None,
                                    status.ctypes.data_as(_pi32))
        if rc != 0:
            raise CedarError("ch_measure_rows failed (%s): %s" % (RETCODES.get(rc, rc), self.last_error()))
        return val, status, out_s

    def freq_measure_rows(self, freqs_hz, values, specs, n_meas, sens=None):
        """ch_freq_measure_rows: frequency-domain measures of any rows.  values[n_rows][n_freq][S] complex (a PSD row: real),
        sens[n_rows][n_par][n_freq][S] or None, specs a ctypes array of ch_fmeasure_spec (acmeasure.resolve_fmeasures):
        (value[n_meas][S], status[n_meas][S], sens[n_meas][n_par][S] or None)."""
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64).reshape(-1)
        v = np.asarray(values, dtype=np.complex128)
        if v.ndim != 3 or v.shape[1] != len(f):
            raise CedarError("freq_measure_rows: values must be [n_rows][n_freq][n_samples]")
        n_rows, _, S = v.shape
        v = np.ascontiguousarray(v).view(np.float64)
        sn = None if sens is None else np.asarray(sens, dtype=np.complex128)
        n_par = 0 if sn is None else sn.shape[1]
        if sn is not None and sn.shape != (n_rows, n_par, len(f), S):
            raise CedarError("freq_measure_rows: sens must be [n_rows][n_par][n_freq][n_samples]")
        if sn is not None:
            sn = np.ascontiguousarray(sn).view(np.float64)
        val, status = np.full((n_meas, S), np.nan), np.zeros((n_meas, S), np.int32)
        out_s = np.full((n_meas, n_par, S), np.nan) if sn is not None else None
        rc = self.L.ch_freq_measure_rows(self.h, len(f), _p(f), n_rows, S, _p(v), n_par, _p(sn) if sn is not None else None, n_meas, specs, _p(val),
                                         _p(out_s) if out_s is not None else None, status.ctypes.data_as(_pi32))
        if rc != 0:
            raise CedarError("ch_freq_measure_rows failed (%s): %s" % (RETCODES.get(rc, rc), self.last_error()))
        return val, status, out_s

    def close(self):
        if getattr(self, "h", None):
            self.L.ch_destroy(self.h)
            self.h = None


_default_ctx = {}


def default_context(device_id=None):
    if device_id is None:
        device_id = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("CEDARHIP_USE_LOCAL_RANK", "1") == "1" else 0
    if device_id not in _default_ctx:
        _default_ctx[device_id] = Context(device_id)
    return _default_ctx[device_id]


class DeviceRows:
    """Result rows of the last transient still in HBM, [n_obs][n_times][n_samples] fp64, exposed through `__cuda_array_interface__`
    (zero-copy: `torch.as_tensor(rows, device="cuda")`).  Owned by the engine circuit: valid until its next call; `owner` keeps it alive."""

    def __init__(self, ptr, shape, owner):
        self.ptr, self.shape, self.owner = int(ptr), tuple(int(x) for x in shape), owner
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": "<f8", "data": (self.ptr, False), "version": 2, "strides": None}


class EngineCircuit:
    """A circuit resident on the GPU: structure analysed once, parameters per sample."""

    def __init__(self, circuit, ctx=None, small_signal=False):
        """small_signal=True keeps the sources' AC magnitudes (needed by .ac(); .noise() works either way)."""
        self.ctx = ctx or default_context()
        self.L = self.ctx.L
        self.circuit = circuit
        self._desc = circuit.to_desc(small_signal=small_signal)
        for nm, (mod, _) in getattr(circuit, "va_instances", {}).items():
            mid = circuit.dev_ipar[circuit.dev_names.index(nm)][0]
            got = self.L.ch_va_module_name(mid)
            if got is None or got.decode() != mod.name:
                raise CedarError("the Verilog-A model library (lib/va_modules.json) and libcedarhip.so are out of step: rebuild both")
        self.h = self.L.ch_circuit_build(self.ctx.h, C.byref(self._desc))
        if not self.h:
            raise CedarError("ch_circuit_build failed: %s" % self.ctx.last_error())
        self.n_mna = circuit.n_mna
        self.n_samples = 1
        # the library writes [n_samples][n_mna] doubles into buffers this class allocates: the two sides must agree on n_mna
        lib_n_mna = self.info()["n_mna"]
        if lib_n_mna != self.n_mna:
            self.L.ch_circuit_free(self.h)
            self.h = None
            raise CedarError("host mirror and engine disagree on the MNA size (%d vs %d)" % (self.n_mna, lib_n_mna))

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.L.ch_circuit_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def info(self):
        i = ChInfo()
        self.L.ch_circuit_info(self.h, C.byref(i))
        return i.asdict()

    def maps(self):
        nn, nb = self.circuit.n_nodes, len(self.circuit.branch_devices)
        nu = np.zeros(nn + 1, np.int32)
        nk = np.zeros(nn + 1, np.int32)
        bu = np.zeros(max(1, nb), np.int32)
        self.L.ch_circuit_maps(self.h, nu.ctypes.data_as(_pi32), nk.ctypes.data_as(_pi32), bu.ctypes.data_as(_pi32))
        return nu, nk, bu[:nb]

    def _check(self, rc, what):
        if rc != 0:
            raise CedarError("%s failed (%s): %s" % (what, RETCODES.get(rc, rc), self.ctx.last_error()))

    def set_samples(self, n):
        self._check(self.L.ch_set_samples(self.h, int(n)), "ch_set_samples")
        self.n_samples = int(n)

    def set_params(self, slot_ids, values, lo=0, hi=None):
        """values[slot][sample] for samples lo..hi."""
        hi = self.n_samples if hi is None else hi
        ids = np.ascontiguousarray(slot_ids, dtype=np.int32)
        vals = np.ascontiguousarray(values, dtype=np.float64).reshape(len(ids), hi - lo)
        self._check(self.L.ch_set_params(self.h, lo, hi, len(ids), ids.ctypes.data_as(_pi32), _p(vals)), "ch_set_params")

    def dc(self, opts=None, check=False):
        opts = opts or dc_opts()
        x = np.zeros((self.n_samples, self.n_mna))
        status = np.zeros(self.n_samples, np.int32)
        st = ChStats()
        rc = self.L.ch_dc(self.h, C.byref(opts), _p(x), status.ctypes.data_as(_pi32), C.byref(st))
        if check:
            self._check(rc, "ch_dc")
        return rc, x, status, st.asdict()

    def tran(self, t0, t1, opts=None, measures=None):
        """measures: (n_meas, ctypes array of ch_measure_spec) or None.  With measures the stats carry "measures" = (value[n_meas][S],
        status[n_meas][S], None), taken by ch_result_measure before the handle is freed (in HBM where the rows are still there)."""
        opts = opts or tran_opts()
        r = C.c_void_p()
        rc = self.L.ch_tran(self.h, float(t0), float(t1), C.byref(opts), C.byref(r))
        if not r:
            raise CedarError("ch_tran failed: %s" % self.ctx.last_error())
        try:
            res = self._result(r)
            if measures is not None:
                res[3]["measures"] = self._measure(r, measures, 0, len(res[0]))
            return (rc,) + res
        finally:
            self.L.ch_result_free(r)

    def _measure(self, r, measures, n_par, nt):
        """ch_result_measure on a result handle: (value, status, sens or None); all NaN / "not found" for a result without rows."""
        n_meas, specs = measures
        S = self.n_samples
        val, status = np.full((n_meas, S), np.nan), np.ones((n_meas, S), np.int32)
        sens = np.full((n_meas, n_par, S), np.nan) if n_par else None
        if n_meas and nt and len(self.circuit.obs):
            rc = self.L.ch_result_measure(r, n_meas, specs, _p(val), _p(sens) if sens is not None else None, status.ctypes.data_as(_pi32))
            self._check(rc, "ch_result_measure")
        return val, status, sens

    def _result(self, r):
        """(t, values[n_obs][n_times][S], final state, stats) of a transient result handle."""
        nt = self.L.ch_result_n_times(r)
        nobs = len(self.circuit.obs)
        S = self.n_samples
        t = np.ctypeslib.as_array(self.L.ch_result_times(r), (nt,)).copy() if nt else np.zeros(0)
        v = np.ctypeslib.as_array(self.L.ch_result_values(r), (nobs, nt, S)).copy() if nt and nobs else np.zeros((nobs, nt, S))
        fs = self.L.ch_result_final_state(r)
        xf = np.ctypeslib.as_array(fs, (S, self.n_mna)).copy() if fs and nt else np.zeros((S, self.n_mna))
        st = ChStats()
        self.L.ch_result_stats(r, C.byref(st))
        sd = st.asdict()
        dp = self.L.ch_result_dense_points(r)
        # per saved row: how many newest rows the step's dense-output polynomial runs through (0: none; api.Solution.__call__)
        sd["dense_points"] = np.ctypeslib.as_array(dp, (nt,)).copy() if (dp and nt) else None
        # the same rows still in HBM (ch_result_device_values): a view for torch.as_tensor(..., device="cuda"), valid until the next call on this circuit
        dptr, dn = C.c_void_p(), C.c_int64(0)
        ok = self.L.ch_result_device_values(r, C.byref(dptr), C.byref(dn)) == 0 and dptr.value and dn.value == nobs * nt * S
        sd["device_rows"] = DeviceRows(dptr.value, (nobs, nt, S), self) if ok else None
        return t, v, xf, sd

    def tran_sens(self, t0, t1, slot_ids, opts=None, rel_step=None, abs_step=None, measures=None):
        """Transient on the host stepper and the derivatives of every observable with respect to the declared slots `slot_ids` along
        it (direct method, ch_tran_sens): what `tran` returns, then sens[n_obs][n_par][n_times][S].  measures as for `tran`; the
        stats' "measures" then end with the measures' own derivatives [n_meas][n_par][S]."""
        opts = opts or tran_opts()
        ids = np.ascontiguousarray(slot_ids, dtype=np.int32).reshape(-1)
        so = sens_opts(rel_step=rel_step, abs_step=abs_step, n_par=len(ids))
        r = C.c_void_p()
        rc = self.L.ch_tran_sens(self.h, float(t0), float(t1), C.byref(opts), len(ids), ids.ctypes.data_as(_pi32), C.byref(so), C.byref(r))
        if not r:
            raise CedarError("ch_tran_sens failed: %s" % self.ctx.last_error())
        try:
            t, v, xf, sd = self._result(r)
            nobs, nt, npar = len(self.circuit.obs), len(t), self.L.ch_result_n_par(r)
            ps = self.L.ch_result_sens(r)
            have = bool(ps) and npar == len(ids) and nt > 0 and nobs > 0
            sens = np.ctypeslib.as_array(ps, (nobs, npar, nt, self.n_samples)).copy() if have else np.full((nobs, len(ids), nt, self.n_samples), np.nan)
            if measures is not None:
                sd["measures"] = self._measure(r, measures, len(ids) if have else 0, nt)
            return rc, t, v, xf, sd, sens
        finally:
            self.L.ch_result_free(r)

    def ac(self, freqs_hz, opts=None):
        """Small-signal sweep: complex MNA phasors [S][n_freq][n_mna] for unit excitation of the sources' `ac`."""
        opts = opts or dc_opts()
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64)
        out = np.zeros((self.n_samples, len(f), self.n_mna, 2))
        st = ChStats()
        rc = self.L.ch_ac(self.h, C.byref(opts), len(f), _p(f), _p(out), C.byref(st))
        return rc, out[..., 0] + 1j * out[..., 1], st.asdict()

    def noise(self, out_kind, out_index, freqs_hz, opts=None):
        """Output-noise PSD [S][n_freq] at a node (out_kind 0, node id) or branch current (1, device index)."""
        opts = opts or dc_opts()
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64)
        out = np.zeros((self.n_samples, len(f)))
        st = ChStats()
        rc = self.L.ch_noise(self.h, C.byref(opts), int(out_kind), int(out_index), len(f), _p(f), _p(out), C.byref(st))
        return rc, out, st.asdict()

    def _send_mos_noise(self):
        """The noise parameters Circuit.add_model kept beside each card go down once, before the first ch_noise_ex."""
        if getattr(self, "_mos_noise_sent", False):
            return
        for mi, rec in enumerate(getattr(self.circuit, "model_noise", [])):
            row = np.array([rec.get(k, np.nan) for k in MOS_NOISE_PARAMS], dtype=np.float64)
            self._check(self.L.ch_set_mos_noise(self.h, mi, _p(row)), "ch_set_mos_noise")
        self._mos_noise_sent = True

    def noise_sources_count(self, out_kind, out_index):
        """Columns of the source table of the output's block (ch_noise_sources with every array NULL)."""
        n = C.c_int32(0)
        self._check(self.L.ch_noise_sources(self.h, int(out_kind), int(out_index), 0, C.byref(n), None, None, None, None, None, None), "ch_noise_sources")
        return n.value

    def noise_ex(self, out_kind, out_index, freqs_hz, opts=None, mos_noise=True, contributions=False):
        """ch_noise_ex: (rc, psd[S][n_freq], contrib[S][n_freq][n_src] or None, stats).  mos_noise: the BSIM4 MOSFETs' channel thermal
        and flicker noise join the resistors' and the compiled modules'; contributions: every source's share of the PSD."""
        opts = opts or dc_opts()
        self._send_mos_noise()
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64)
        out = np.zeros((self.n_samples, len(f)))
        contrib = np.zeros((self.n_samples, len(f), self.noise_sources_count(out_kind, out_index))) if contributions else None
        no = ChNoiseOpts(1 if mos_noise else 0)
        st = ChStats()
        rc = self.L.ch_noise_ex(self.h, C.byref(opts), C.byref(no), int(out_kind), int(out_index), len(f), _p(f), _p(out),
                                _p(contrib) if contrib is not None and contrib.size else None, C.byref(st))
        return rc, out, contrib, st.asdict()

    def noise_sources(self, out_kind, out_index, sample=0):
        """The source table the last noise_ex built for this output, sample `sample`: dict of arrays dev, a, b (MNA indices, -1: ground
        or a node held by sources), pwr, ex, and operands[n_src][16] (MOS_NOISE_OPERANDS; zeros for other devices)."""
        n = self.noise_sources_count(out_kind, out_index)
        dev, a, b = (np.zeros(max(1, n), np.int32) for _ in range(3))
        pwr, ex, ops = np.zeros(max(1, n)), np.zeros(max(1, n)), np.zeros((max(1, n), len(MOS_NOISE_OPERANDS)))
        nn = C.c_int32(0)
        if n:
            self._check(self.L.ch_noise_sources(self.h, int(out_kind), int(out_index), int(sample), C.byref(nn), dev.ctypes.data_as(_pi32), a.ctypes.data_as(_pi32),
                                                b.ctypes.data_as(_pi32), _p(pwr), _p(ex), _p(ops)), "ch_noise_sources")
        return {"dev": dev[:n], "a": a[:n], "b": b[:n], "pwr": pwr[:n], "ex": ex[:n], "operands": ops[:n]}

    def dc_sens(self, slot_ids, opts=None, rel_step=None, abs_step=None):
        """DC operating point and its derivatives with respect to the declared slots `slot_ids` (direct method, ch_dc_sens):
        (rc, x[S][n_mna], sens[S][n_par][n_mna], status[S], stats).  rel_step / abs_step: see include/cedarhip.h ch_sens_opts."""
        opts = opts or dc_opts()
        ids = np.ascontiguousarray(slot_ids, dtype=np.int32).reshape(-1)
        so = sens_opts(rel_step=rel_step, abs_step=abs_step, n_par=len(ids))
        x = np.zeros((self.n_samples, self.n_mna))
        sens = np.full((self.n_samples, len(ids), self.n_mna), np.nan)
        status = np.zeros(self.n_samples, np.int32)
        st = ChStats()
        rc = self.L.ch_dc_sens(self.h, C.byref(opts), len(ids), ids.ctypes.data_as(_pi32), C.byref(so), _p(x), _p(sens),
                               status.ctypes.data_as(_pi32), C.byref(st))
        return rc, x, sens, status, st.asdict()

    def ac_sens(self, slot_ids, freqs_hz, opts=None, rel_step=None, abs_step=None):
        """Small-signal sweep and its derivatives with respect to the declared slots `slot_ids` (direct method, ch_ac_sens):
        (rc, x_ac[S][n_freq][n_mna], dc_sens[S][n_par][n_mna], sens[S][n_freq][n_par][n_mna], status[S], stats); x_ac and sens complex.
        Needs an engine circuit built with small_signal=True."""
        opts = opts or dc_opts()
        ids = np.ascontiguousarray(slot_ids, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64).reshape(-1)
        so = sens_opts(rel_step=rel_step, abs_step=abs_step, n_par=len(ids))
        S = self.n_samples
        x = np.full((S, len(f), self.n_mna, 2), np.nan)
        dsens = np.full((S, len(ids), self.n_mna), np.nan)
        sens = np.full((S, len(f), len(ids), self.n_mna, 2), np.nan)
        status = np.zeros(S, np.int32)
        st = ChStats()
        rc = self.L.ch_ac_sens(self.h, C.byref(opts), len(ids), ids.ctypes.data_as(_pi32), C.byref(so), len(f), _p(f), _p(x), _p(dsens), _p(sens),
                               status.ctypes.data_as(_pi32), C.byref(st))
        return rc, x[..., 0] + 1j * x[..., 1], dsens, sens[..., 0] + 1j * sens[..., 1], status, st.asdict()

    def ac_measure(self, slot_ids, freqs_hz, specs, n_meas, opts=None, rel_step=None, abs_step=None):
        """The AC analysis measured in HBM (ch_ac_measure): the launches of ch_ac (no slots) or ch_ac_sens, then the measures of `specs`
        (a ctypes array of ch_fmeasure_spec over MNA rows) where the result lies: (rc, value[n_meas][S], status[n_meas][S],
        sens[n_meas][n_par][S] or None, sample_status[S], stats).  Needs an engine circuit built with small_signal=True."""
        opts = opts or dc_opts()
        ids = np.ascontiguousarray(slot_ids, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64).reshape(-1)
        so = sens_opts(rel_step=rel_step, abs_step=abs_step, n_par=max(1, len(ids)))
        S = self.n_samples
        val, status = np.full((n_meas, S), np.nan), np.zeros((n_meas, S), np.int32)
        sens = np.full((n_meas, len(ids), S), np.nan) if len(ids) else None
        sample_status = np.zeros(S, np.int32)
        st = ChStats()
        rc = self.L.ch_ac_measure(self.h, C.byref(opts), len(ids), ids.ctypes.data_as(_pi32) if len(ids) else None, C.byref(so), len(f), _p(f), n_meas, specs,
                                  _p(val), _p(sens) if sens is not None else None, status.ctypes.data_as(_pi32), sample_status.ctypes.data_as(_pi32), C.byref(st))
        return rc, val, status, sens, sample_status, st.asdict()

    def loop_gain(self, probe_dev, freqs_hz, slot_ids=(), specs=None, n_meas=0, opts=None, rel_step=None, abs_step=None):
        """Loop gain of the closed loop at the voltage-source probe `probe_dev` (device index), its derivatives with respect to the
        declared slots `slot_ids` and the measures of `specs` (a ctypes array of ch_fmeasure_spec over one row, 0 = T) where the rows
        lie (ch_loop_gain): (rc, T[S][n_freq], dT[S][n_freq][n_par] or None, value[n_meas][S], status[n_meas][S], sens[n_meas][n_par][S]
        or None, sample_status[S], stats); T and dT complex.  Needs an engine circuit whose description carries |ac| = 1 on the probe's
        source and 0 on every other one."""
        opts = opts or dc_opts()
        ids = np.ascontiguousarray(slot_ids, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64).reshape(-1)
        so = sens_opts(rel_step=rel_step, abs_step=abs_step, n_par=max(1, len(ids)))
        S = self.n_samples
        T = np.full((S, len(f), 2), np.nan)
        dT = np.full((S, len(f), len(ids), 2), np.nan) if len(ids) else None
        val, status = np.full((n_meas, S), np.nan), np.zeros((n_meas, S), np.int32)
        sens = np.full((n_meas, len(ids), S), np.nan) if len(ids) and n_meas else None
        sample_status = np.zeros(S, np.int32)
        st = ChStats()
        rc = self.L.ch_loop_gain(self.h, C.byref(opts), int(probe_dev), len(ids), ids.ctypes.data_as(_pi32) if len(ids) else None, C.byref(so), len(f), _p(f),
                                 _p(T), _p(dT) if dT is not None else None, n_meas, specs if n_meas else None,
                                 _p(val) if n_meas else None, _p(sens) if sens is not None else None, status.ctypes.data_as(_pi32) if n_meas else None,
                                 sample_status.ctypes.data_as(_pi32), C.byref(st))
        return rc, T[..., 0] + 1j * T[..., 1], dT[..., 0] + 1j * dT[..., 1] if dT is not None else None, val, status, sens, sample_status, st.asdict()

    def net_params(self, port_devs, z0, freqs_hz, slot_ids=(), specs=None, n_meas=0, opts=None, rel_step=None, abs_step=None, kinds="SYZ"):
        """S, Y and Z parameters seen from the voltage-source ports `port_devs` (device indices, port 1 first) with the reference
        impedances `z0` (one per port), their derivatives with respect to the declared slots `slot_ids` and the measures of `specs` (a
        ctypes array of ch_fmeasure_spec over the rows kind * P^2 + j * P + k, kind 0 = S, 1 = Y, 2 = Z) where the rows lie
        (ch_net_params): (rc, {kind: X[S][n_freq][P][P]}, {kind: dX[S][n_freq][n_par][P][P]} or None, value[n_meas][S],
        status[n_meas][S], sens[n_meas][n_par][S] or None, sample_status[S], stats); X and dX complex, only the `kinds` asked for.
        Needs an engine circuit whose description carries |ac| = 1 on every port's source and 0 on every other one."""
        opts = opts or dc_opts()
        ports = np.ascontiguousarray(port_devs, dtype=np.int32).reshape(-1)
        z = np.ascontiguousarray(z0, dtype=np.float64).reshape(-1)
        ids = np.ascontiguousarray(slot_ids, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64).reshape(-1)
        so = sens_opts(rel_step=rel_step, abs_step=abs_step, n_par=max(1, len(ids)))
        S, P = self.n_samples, len(ports)
        val_of = {k: np.full((S, len(f), P, P, 2), np.nan) for k in "SYZ" if k in kinds}
        der_of = {k: np.full((S, len(f), len(ids), P, P, 2), np.nan) for k in val_of} if len(ids) else None
        val, status = np.full((n_meas, S), np.nan), np.zeros((n_meas, S), np.int32)
        sens = np.full((n_meas, len(ids), S), np.nan) if len(ids) and n_meas else None
        sample_status = np.zeros(S, np.int32)
        st = ChStats()
        rc = self.L.ch_net_params(self.h, C.byref(opts), P, ports.ctypes.data_as(_pi32), _p(z), len(ids), ids.ctypes.data_as(_pi32) if len(ids) else None, C.byref(so), len(f), _p(f),
                                  *[_p(val_of[k]) if k in val_of else None for k in "SYZ"], *[_p(der_of[k]) if der_of and k in der_of else None for k in "SYZ"],
                                  n_meas, specs if n_meas else None, _p(val) if n_meas else None, _p(sens) if sens is not None else None,
                                  status.ctypes.data_as(_pi32) if n_meas else None, sample_status.ctypes.data_as(_pi32), C.byref(st))
        cplx = lambda d: {k: v[..., 0] + 1j * v[..., 1] for k, v in d.items()} if d is not None else None   # noqa: E731
        return rc, cplx(val_of), cplx(der_of), val, status, sens, sample_status, st.asdict()

    def noise_sens(self, out_kind, out_index, slot_ids, freqs_hz, opts=None, mos_noise=False, rel_step=None, abs_step=None):
        """Output-noise PSD and its derivatives with respect to the declared slots `slot_ids` (direct method on the adjoint system,
        ch_noise_sens): (rc, psd[S][n_freq], dpsd[S][n_freq][n_par], dc_sens[S][n_par][n_mna], status[S], stats).  mos_noise: as in noise_ex."""
        opts = opts or dc_opts()
        if mos_noise:
            self._send_mos_noise()
        ids = np.ascontiguousarray(slot_ids, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(freqs_hz, dtype=np.float64).reshape(-1)
        so = sens_opts(rel_step=rel_step, abs_step=abs_step, n_par=len(ids))
        S = self.n_samples
        psd = np.full((S, len(f)), np.nan)
        dpsd = np.full((S, len(f), len(ids)), np.nan)
        dsens = np.full((S, len(ids), self.n_mna), np.nan)
        status = np.zeros(S, np.int32)
        no = ChNoiseOpts(1 if mos_noise else 0)
        st = ChStats()
        rc = self.L.ch_noise_sens(self.h, C.byref(opts), C.byref(no), len(ids), ids.ctypes.data_as(_pi32), C.byref(so), int(out_kind), int(out_index), len(f), _p(f),
                                  _p(psd), _p(dpsd), _p(dsens), status.ctypes.data_as(_pi32), C.byref(st))
        return rc, psd, dpsd, dsens, status, st.asdict()

    def eval(self, x_mna, t=0.0, alpha0=0.0, mode=1, sample=0):
        x = np.ascontiguousarray(x_mna, dtype=np.float64)
        n = self.n_mna
        F, Q, J = np.zeros(n), np.zeros(n), np.zeros((n, n))
        self._check(self.L.ch_eval(self.h, sample, _p(x), t, alpha0, mode, _p(F), _p(Q), _p(J)), "ch_eval")
        return F, Q, J

    def mos_eval(self, v, sample=0, quad=False):
        v = np.ascontiguousarray(v, dtype=np.float64)
        nm = self.info()["n_mos"]
        out = np.zeros((nm, 40))
        fn = self.L.ch_mos_eval_quad if quad else self.L.ch_mos_eval
        self._check(fn(self.h, sample, _p(v), _p(out)), "ch_mos_eval")
        return out
