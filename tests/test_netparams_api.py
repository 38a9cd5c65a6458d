"""The Python surface of net_params that needs no GPU: the reserved row symbols of its measures and the Touchstone writer."""
import numpy as np
import pytest

from cedarsim_jl_amd import NetParamsSolution, bandwidth, db, phase
from cedarsim_jl_amd.acmeasure import net_rows, resolve_fmeasures
from cedarsim_jl_amd.batch import net_params_request
from cedarsim_jl_amd.circuit import CedarError


def test_row_symbols():
    for P in (1, 2, 3, 8):
        row_of = net_rows(P)
        for kind, letter in enumerate("syz"):       # rows: kind * P^2 + j * P + k, kind 0 = S, 1 = Y, 2 = Z
            for j in range(1, P + 1):
                for k in range(1, P + 1):
                    want = kind * P * P + (j - 1) * P + (k - 1)
                    assert row_of("%s%d%d" % (letter, j, k), "m") == (want, -1, 1.0)
                    assert row_of("%s%d%d" % (letter.upper(), j, k), "m") == (want, -1, 1.0)
    row_of = net_rows(2)
    assert row_of("s21", "m")[0] == 1 * 2 + 0 and row_of("y11", "m")[0] == 4 and row_of("z12", "m")[0] == 8 + 1
    for sym in ("s01", "s10", "s31", "s13", "y33"):
        with pytest.raises(CedarError, match="outside 1 .. 2"):
            row_of(sym, "m")
    for sym in ("t", "T", "s2", "s211", "x21", "vout", ("a", "b"), None):
        with pytest.raises(CedarError, match="s21"):
            row_of(sym, "m")


def test_rows_are_accepted_where_a_measure_takes_a_row():
    res = resolve_fmeasures([bandwidth("bw", "s21", ref_at=1e3), bandwidth("bw2", db("S21"), ref_at=1e3), bandwidth("py", phase("y11"), ref_at=1e3)], net_rows(2))
    assert res.names == ["bw", "bw2", "py"]
    assert res.specs[0].s1.row_a == 2 and res.specs[0].s1.row_b == -1 and res.specs[1].s1.row_a == 2 and res.specs[2].s1.row_a == 4
    with pytest.raises(CedarError, match="bw"):
        resolve_fmeasures([bandwidth("bw", "s31", ref_at=1e3)], net_rows(2))


def test_request_resolves_ports_and_reference_impedances():
    given = dict(abstol=1e-10, maxiters=200, n_restarts=10, seed=10, rel_step=None, abs_step=None)
    r = net_params_request(("VP1", "vp2"), [1e3, 1e6], 50.0, ("r1",), (), given)
    assert r.kind == "net_params" and r.probe == ("vp1", "vp2") and r.z0 == (50.0, 50.0) and r.freqs_hz == (1e3, 1e6)
    assert net_params_request("vp1", [1.0], 75, (), (), given).probe == ("vp1",)
    assert net_params_request(("a", "b"), [1.0], (50.0, 75.0), (), (), given).z0 == (50.0, 75.0)
    with pytest.raises(CedarError, match="3 reference impedances for 2 ports"):
        net_params_request(("a", "b"), [1.0], (50.0, 75.0, 1.0), (), (), given)


def solution(P, z0, rng):
    f = np.array([1e6, 2.5e8, 1e9])
    S = rng.normal(size=(3, P, P)) + 1j * rng.normal(size=(3, P, P))
    return NetParamsSolution(None, ["vp%d" % j for j in range(1, P + 1)], z0, f, {"S": S, "Y": 2.0 * S, "Z": 3.0 * S}, None, (), [], [], [], None, 0, {})


def read_touchstone(path, P):
    z0, rows = None, []
    for line in open(path).read().splitlines():
        line = line.split("!")[0].strip()
        if not line:
            continue
        if line.startswith("#"):
            t = line[1:].split()
            assert [x.upper() for x in t[:4]] == ["HZ", "S", "RI", "R"]
            z0 = float(t[4])
            continue
        rows += [float(x) for x in line.split()]
    per = 1 + 2 * P * P
    data = np.array(rows).reshape(-1, per)
    M = (data[:, 1::2] + 1j * data[:, 2::2]).reshape(-1, P, P)
    return z0, data[:, 0], np.transpose(M, (0, 2, 1)) if P == 2 else M   # two ports: S11 S21 S12 S22


@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_write_touchstone_round_trip(tmp_path, P):
    sol = solution(P, [50.0] * P, np.random.default_rng(P))
    path = str(tmp_path / ("net.s%dp" % P))
    sol.write_touchstone(path)
    z0, f, S = read_touchstone(path, P)
    assert z0 == 50.0 and np.array_equal(f, sol.freqs) and np.array_equal(S, sol.S)   # repr round-trips a double exactly
    assert "# Hz S RI R 50.0" in open(path).read()
    if P > 2:
        assert max(len(ln.split()) for ln in open(path).read().splitlines() if not ln.startswith(("!", "#"))) <= 9   # at most four pairs on a line
    assert np.array_equal(sol.s(1, 1), sol.S[:, 0, 0]) and np.array_equal(sol.y(P, 1), sol.Y[:, P - 1, 0]) and np.array_equal(sol.z(1, P), sol.Z[:, 0, P - 1])
    with pytest.raises(CedarError, match="1 to %d" % P):
        sol.s(0, 1)
    with pytest.raises(CedarError, match="1 to %d" % P):
        sol.z(1, P + 1)


def test_write_touchstone_refusals(tmp_path):
    sol = solution(2, [50.0, 75.0], np.random.default_rng(0))
    with pytest.raises(CedarError, match="z0 differ"):
        sol.write_touchstone(str(tmp_path / "a.s2p"))
    with pytest.raises(CedarError, match="RI"):
        solution(2, [50.0, 50.0], np.random.default_rng(0)).write_touchstone(str(tmp_path / "a.s2p"), fmt="MA")
