"""What a circuit keeps from call to call around the device stepper's launch — the first DC pass' start vector on the device with
the generator states behind it, the launch's constants, the kernel's attributes — never shows in a result: every output of a call
on a circuit that has been used before is bit for bit that of the same call on a fresh EngineCircuit.  Circuits: dff_array(3) (the
last wave pair has a helper wave), dff_array(4) (a full workgroup) and one DFF with three samples (S > 1: three generators, the
donor pass of the first restart).  Between the calls change: nothing (three transients), the seed, x0 given and not, a parameter,
the time span, the output grid, the DC options so that restarts run, the row limit so that the launch resumes; and ch_dc alone
behind a transient.  The reference of every (circuit, call) is computed once on its own fresh circuit and shared."""
import os

import numpy as np
import pytest

from cedarsim_jl_amd import bsim4_params as B4
from cedarsim_jl_amd import dc_opts, tran_opts
from cedarsim_jl_amd.workloads import DFF_TSPAN, dff_array

pytestmark = pytest.mark.gpu

NAMES = ("dff3", "dff4", "dff1x3")
SPAN = (0.0, 2.0e-7)          # the clock's first edges: every phase of the stepper runs, a transient takes a few milliseconds
SPAN2 = (0.0, 1.3e-7)
GRID_A = np.linspace(0.0, 2.0e-7, 41)
GRID_B = np.linspace(0.0, 2.0e-7, 17)
_refs = {}


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


def circuit(name):
    return dff_array({"dff3": 3, "dff4": 4, "dff1x3": 1}[name], observe="q")


def vth0(c, scale):
    """(slot, value) of the n-channel card's vth0 times `scale`"""
    return c.slot("nfet_06v0", "vth0"), c.models[c.model_names.index("nfet_06v0")][B4.PARAM_INDEX["vth0"]] * scale


def engine(E, name, scale=1.0):
    """a fresh circuit; dff1x3: three samples of vth0; `scale` moves vth0 of every sample (what set_params does between calls)"""
    c = circuit(name)
    slot, v = vth0(c, scale)
    e = E(c)
    S = 3 if name == "dff1x3" else 1
    e.set_samples(S)
    e.set_params([slot], [[v * (1.0 + 0.01 * s) for s in range(S)]])
    return e


def rescale(e, scale):
    slot, v = vth0(e.circuit, scale)
    e.set_params([slot], [[v * (1.0 + 0.01 * s) for s in range(e.n_samples)]])


def tran(e, span=SPAN, saveat=None, maxrows=None, **dc):
    dc.setdefault("abstol", 1e-14)
    if maxrows is not None:
        os.environ["CEDARHIP_PERSIST_MAXROWS"] = str(maxrows)
    try:
        rc, t, v, xf, st = e.tran(span[0], span[1], tran_opts(abstol=1e-4, reltol=1e-4, saveat=saveat, stepper="device", dc=dc_opts(**dc)))
    finally:
        if maxrows is not None:
            del os.environ["CEDARHIP_PERSIST_MAXROWS"]
    assert rc == 0, (rc, e.ctx.last_error())
    assert st["stepper"] == 2
    meta = [st[k] for k in ("stepper_mode", "naccept", "nreject", "nnonliniter", "nrestarts", "n_step_attempts", "n_kernel_launches")]
    return {"t": np.asarray(t, np.float64), "v": np.asarray(v, np.float64), "xf": np.asarray(xf, np.float64), "meta": np.array(meta, np.int64)}


def dc(e, **kw):
    rc, x, status, st = e.dc(dc_opts(**kw))
    meta = [rc, st["nrestarts"], st["nnonliniter"], st["n_block_iters"]]
    return {"x": np.asarray(x, np.float64), "status": np.asarray(status, np.int64), "meta": np.array(meta, np.int64)}


def ref(E, name, key, call, scale=1.0):
    """`call` on a fresh circuit, once per (circuit, key)"""
    k = (name, key)
    if k not in _refs:
        _refs[k] = call(engine(E, name, scale))
    return _refs[k]


def bits_equal(got, want, what):
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if a.dtype == np.float64:
            n = int(np.count_nonzero(a.view(np.uint64) != b.view(np.uint64)))   # NaN of an eliminated branch compares by its bits too
        else:
            n = int(np.count_nonzero(a != b))
        print("%s: %s %r, %d of %d differ" % (what, k, a.shape, n, a.size))
        assert n == 0, (what, k, n, got["meta"].tolist(), want["meta"].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_second_and_third_transient_on_one_circuit(E, name):
    want = ref(E, name, "base", tran)
    e = engine(E, name)
    for i in range(3):
        bits_equal(tran(e), want, "%s call %d" % (name, i + 1))
    assert len(want["t"]) > 20 and want["meta"][1] == len(want["t"]) - 1


@pytest.mark.parametrize("name", NAMES)
def test_seed_changed_between_calls(E, name):
    e = engine(E, name)
    bits_equal(tran(e), ref(E, name, "base", tran), name + " seed 10")
    bits_equal(tran(e, seed=11), ref(E, name, "seed11", lambda f: tran(f, seed=11)), name + " seed 11")
    bits_equal(tran(e), ref(E, name, "base", tran), name + " seed 10 again")


@pytest.mark.parametrize("name", NAMES)
def test_x0_given_then_not_given(E, name):
    e = engine(E, name)
    x0 = np.full((e.n_samples, e.n_mna), 0.25) + 0.001 * np.arange(e.n_mna)[None, :]
    bits_equal(tran(e), ref(E, name, "base", tran), name + " no x0")
    bits_equal(tran(e, x0=x0), ref(E, name, "x0", lambda f: tran(f, x0=x0)), name + " x0")
    bits_equal(tran(e), ref(E, name, "base", tran), name + " no x0 again")


@pytest.mark.parametrize("name", NAMES)
def test_set_params_between_calls(E, name):
    e = engine(E, name)
    bits_equal(tran(e), ref(E, name, "base", tran), name + " base")
    rescale(e, 1.03)
    bits_equal(tran(e), ref(E, name, "vth0*1.03", tran, scale=1.03), name + " vth0 * 1.03")
    rescale(e, 1.0)
    bits_equal(tran(e), ref(E, name, "base", tran), name + " base again")


@pytest.mark.parametrize("name", NAMES)
def test_another_tspan_and_another_saveat_between_calls(E, name):
    e = engine(E, name)
    bits_equal(tran(e), ref(E, name, "base", tran), name + " base")
    bits_equal(tran(e, span=SPAN2), ref(E, name, "span2", lambda f: tran(f, span=SPAN2)), name + " shorter span")
    bits_equal(tran(e, saveat=GRID_A), ref(E, name, "gridA", lambda f: tran(f, saveat=GRID_A)), name + " grid of 41")
    bits_equal(tran(e, saveat=GRID_B), ref(E, name, "gridB", lambda f: tran(f, saveat=GRID_B)), name + " grid of 17")
    bits_equal(tran(e), ref(E, name, "base", tran), name + " base again")


@pytest.mark.parametrize("name", NAMES)
def test_restarts_draw_what_they_drew(E, name):
    """maxiters = 5 does not reach the operating point of a DFF from 1e-7*randn: the restart (donor pass for S > 1) and the gmin
    stepping run; statuses, the restart count and the state they leave are those of a fresh circuit, also from the cached start."""
    few = dict(abstol=1e-14, maxiters=5, n_restarts=2)
    want = ref(E, name, "dc few", lambda f: dc(f, **few))
    assert want["meta"][1] >= 1      # restarts ran
    e = engine(E, name)
    bits_equal(dc(e, **few), want, name + " first call")
    bits_equal(dc(e, **few), want, name + " second call (cached start)")
    bits_equal(tran(e), ref(E, name, "base", tran), name + " transient behind it")
    bits_equal(dc(e, **few), want, name + " third call")
    more = dict(abstol=1e-14, maxiters=5, n_restarts=4, seed=11)
    bits_equal(dc(e, **more), ref(E, name, "dc more", lambda f: dc(f, **more)), name + " four restarts, seed 11")


@pytest.mark.parametrize("name", NAMES)
def test_resumed_launches(E, name):
    want = ref(E, name, "rows100", lambda f: tran(f, span=DFF_TSPAN, maxrows=100))
    assert want["meta"][6] > 3       # the launch was resumed
    e = engine(E, name)
    bits_equal(tran(e), ref(E, name, "base", tran), name + " base")
    bits_equal(tran(e, span=DFF_TSPAN, maxrows=100), want, name + " 100 rows per launch")
    bits_equal(tran(e, span=DFF_TSPAN, maxrows=100), want, name + " 100 rows per launch again")
    bits_equal(tran(e), ref(E, name, "base", tran), name + " base again")


@pytest.mark.parametrize("name", NAMES)
def test_dc_alone_after_a_transient(E, name):
    want = ref(E, name, "dc", lambda f: dc(f, abstol=1e-14))
    assert want["meta"][0] == 0
    e = engine(E, name)
    tran(e)
    bits_equal(dc(e, abstol=1e-14), want, name + " dc behind a transient")
    bits_equal(dc(e, abstol=1e-14, seed=11), ref(E, name, "dc seed11", lambda f: dc(f, abstol=1e-14, seed=11)), name + " dc, seed 11")
