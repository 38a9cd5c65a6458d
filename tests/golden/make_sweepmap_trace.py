"""Writes tests/golden/sweepmap_trace.json: what `CircuitSweep._batch` does for seeds 0..299 of tests/sweepmap_cases.random_case —
which way it went (`how` up to " ("), how many circuits it built, the slots it found and a digest of the value table (sha256 of
the float64 C-order bytes, 16 hex digits).  Recorded from the commit BEFORE the learner moved to sweepmap.py, so that the test
compares the moved code with its parent and not with itself; run it again only when the algorithm is changed on purpose."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from cedarsim_jl_amd import CircuitSweep  # noqa: E402
from sweepmap_cases import random_case  # noqa: E402

N_SEEDS = 300


def trace(seed):
    build, sweep = random_case(seed)
    cs = CircuitSweep(build, sweep)
    base, _, vals = cs._batch(0, len(cs.points))
    digest = hashlib.sha256(np.ascontiguousarray(vals, np.float64).tobytes()).hexdigest()[:16]
    return {"how": cs.setup["how"].split(" (")[0], "circuit_builds": cs.setup["circuit_builds"],
            "slots": [[int(x) for x in s] for s in base.slots], "vals_sha256_16": digest}


if __name__ == "__main__":
    with open(os.path.join(HERE, "sweepmap_trace.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(trace(s)) for s in range(N_SEEDS)) + "\n]\n")
