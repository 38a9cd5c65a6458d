"""Records tests/golden/lockstep_bits.npz: the device stepper's complete outputs for the shapes of tests/lockstep_bits_cases.py, as
computed by the library that is built in the tree.  Run on the GPU at the commit whose results are to be pinned:

    python tests/golden/make_lockstep_bits.py [output.npz]

Every case is run twice in this process and the two results must be bit-for-bit equal before anything is written; record in two
separate processes as well and compare the two files (`cmp`) before committing one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root

from lockstep_bits_cases import CASES, run_case  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lockstep_bits.npz")
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    rec = {}
    for name in CASES:
        a, b = run_case(EngineCircuit, name), run_case(EngineCircuit, name)
        for k in a:
            if a[k].tobytes() != b[k].tobytes() or a[k].shape != b[k].shape:
                sys.exit("%s/%s differs between two runs: nothing written" % (name, k))
            rec["%s/%s" % (name, k)] = a[k]
        print("%s: meta (stepper, mode, accepted, rejected, iterations) %r, t %r, v %r, xf %r" % (
            name, a["meta"].tolist(), a["t"].shape, a["v"].shape, a["xf"].shape))
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
