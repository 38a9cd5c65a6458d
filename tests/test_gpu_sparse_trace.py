"""The sparse path (path 2) against tests/golden/sparse_path_trace.json, recorded on an MI355X from the commit before its host side
was reorganised (tests/golden/make_sparse_path_trace.py).  The kernels are the same, the stream sees the same launches in the same
order and every sum on this path has a fixed order, so every quantity is compared for EQUALITY: return codes, per-sample status,
`info()`, every integer statistic (launch counts included) and every bit of the DC solutions and saved rows."""
import json
import os

import pytest

import sparse_path_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    return EngineCircuit


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_path_trace.json")) as f:
        return json.load(f)["cases"]


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(sc.CASES)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_sparse_path_reproduces_the_recorded_parent_bit_for_bit(E, recorded, name):
    got, want = sc.run_case(E, name), recorded[name]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["info"]["path"] == 2                      # the case really runs on the sparse path
        assert sorted(g) == sorted(w)
        for key in sorted(w):
            if key in ("x", "t", "v"):
                assert len(g[key]) == len(w[key]), (name, g["kind"], key)
                diff = [i for i, (a, b) in enumerate(zip(g[key], w[key])) if a != b]
                assert not diff, (name, g["kind"], key, len(diff), diff[:5], [(g[key][i], w[key][i]) for i in diff[:3]])
            else:
                assert g[key] == w[key], (name, g["kind"], key, g[key], w[key])
