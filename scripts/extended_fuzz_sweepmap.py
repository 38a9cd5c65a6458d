"""CPU fuzz of the sweep-map learner (cedarsim.jl_amd/sweepmap.py, reached through CircuitSweep._batch): the random builders of
tests/sweepmap_cases.py, whose resistor / capacitor values are random expressions of the sweep variables (identity, proportional,
affine, product, sum, reciprocal, square, conditional, clipped), under product and tandem sweeps; the table the map assembles must
equal one build per point.  No GPU.
usage: python scripts/extended_fuzz_sweepmap.py [first_seed] [n_seeds]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cedarsim_jl_amd import CircuitSweep  # noqa: E402
from sweepmap_cases import random_case, table_mismatch  # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
n_seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
fails, hows = [], {}
for seed in range(first, first + n_seeds):
    build, sweep = random_case(seed)
    try:
        cs = CircuitSweep(build, sweep)
        base, ids, vals = cs._batch(0, len(cs.points))
        how = cs.setup["how"].split(" (")[0]
        hows[how] = hows.get(how, 0) + 1
        bad = table_mismatch(build, cs.points, base, vals)
        if bad is not None:
            fails.append((seed,) + bad + (cs.setup["how"],))
    except Exception as ex:  # noqa: BLE001
        fails.append((seed, "raised", type(ex).__name__, str(ex)[:200]))
for f in fails[:30]:
    print("FAIL", f)
print("%d seeds, %d failures, how: %s" % (n_seeds, len(fails), hows))
sys.exit(1 if fails else 0)
