"""What the BSIM4 device code computes over the card space of tests/bsim4_cards.py equals what tests/golden/make_b4_bits.py recorded
in tests/golden/b4_bits.npz at commit be60700, the parent of the change that gave the dual numbers of ch_bsim4.hpp a compile-time
set of present partials and took the reciprocals of card values out of the Newton loop of the device stepper:
leaving out the terms that are zero by construction may change the sign of an exact zero in a stamp entry and nothing else, and no
step of the device stepper.  Shapes: tests/b4_bits_cases.py."""
import numpy as np
import pytest

import b4_bits_cases as B
import bsim4_cards as BC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def golden():
    with np.load(B.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def differing(a, b):
    """positions whose 64-bit patterns differ"""
    return np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)


_TEMPS = {}
for _n, _t in B.STAMP_CASES:
    _TEMPS.setdefault(_n, []).append(_t)


@pytest.mark.parametrize("name", BC.NAMES)
def test_stamps(E, golden, name):
    got = B.run_stamps(E, name, _TEMPS[name])
    assert sorted(got) == sorted(k for k in golden if k.startswith("stamps/%s/" % name))
    bad = []
    for key, a in sorted(got.items()):
        w = golden[key]
        assert a.shape == w.shape == (len(B.VBANK), 40)
        d = differing(a, w)
        zeros = d & (a == 0.0) & (w == 0.0)               # +0 against -0
        print("%s: %d of %d entries differ in their bits, %d of them as +0 against -0" % (key, int(d.sum()), a.size, int(zeros.sum())))
        if not np.array_equal(np.isnan(a), np.isnan(w)):
            bad.append((key, "NaN positions", np.argwhere(np.isnan(a) != np.isnan(w))[:4].tolist()))
        ne = ~((a == w) | (np.isnan(a) & np.isnan(w)))
        if ne.any():
            r, s = np.argwhere(ne)[0]
            bad.append((key, "%d entries are other numbers" % int(ne.sum()), "instance %d slot %s: %.17g recorded %.17g" % (r, BC.SLOT_NAMES[s], a[r, s], w[r, s])))
        if (d & ~zeros & ~ne).any():                      # differing bits of equal numbers that are not zeros: NaN payloads
            bad.append((key, "NaN bits", int((d & ~zeros & ~ne).sum())))
    assert not bad, bad


def _same_run(got, golden, prefix):
    want = {k: golden["%s/%s" % (prefix, k)] for k in got}
    print("%s: meta (stepper, mode, accepted, rejected, iterations) got %r recorded %r" % (prefix, got["meta"].tolist(), want["meta"].tolist()))
    assert got["meta"].tolist() == want["meta"].tolist()
    assert np.array_equal(got["xf_kept"], want["xf_kept"])
    for k in ("t", "v", "xf"):
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        n = int(differing(got[k], want[k]).sum())
        print("%s: %s %r, %d of %d values differ in their bits" % (prefix, k, got[k].shape, n, got[k].size))
        assert n == 0, (k, n)


def test_recorded_chain_list_holds_the_circuit_variants():
    assert set(BC.CIRCUIT_NAMES) <= set(B.recorded_chain_names())


@pytest.mark.parametrize("nopair", [False, True], ids=["pair", "nopair"])
@pytest.mark.parametrize("name", B.recorded_chain_names())
def test_device_stepper(E, golden, monkeypatch, name, nopair):
    if nopair:
        monkeypatch.setenv("CEDARHIP_PERSIST_NOPAIR", "1")
    else:
        monkeypatch.delenv("CEDARHIP_PERSIST_NOPAIR", raising=False)
    rc, got = B.run_chain(E, name)
    assert rc == 0, rc
    assert np.array_equal(got["t"], BC.CHAIN_SAVEAT)
    assert got["meta"][0] == 2 and got["meta"][1] == 1          # the device-resident stepper, lock-step
    _same_run(got, golden, "chain/%s/%s" % (name, "nopair" if nopair else "pair"))


def test_own_steps(E, golden):
    got = B.run_own(E)
    assert got["meta"][0] == 2 and got["meta"][1] == 2          # the device-resident stepper, CH_MODE_OWN_STEPS
    _same_run(got, golden, "own")
