"""Records tests/golden/pad_edges_bits.npz: the device stepper's outputs for the cases of tests/pad_edges_cases.py, as computed by
the library that is built in the tree (or the one CEDARHIP_LIB names).  Run on the GPU at the commit whose results are to be pinned:

    python tests/golden/make_pad_edges_bits.py [output.npz]

Every case is run twice in this process; a case whose two results are not bit-for-bit equal is reported and left out.  Record in two
separate processes as well and compare the two files (`cmp`) before committing one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root

from pad_edges_cases import CASES, run_case  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pad_edges_bits.npz")
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    rec, dropped = {}, []
    for name in CASES:
        a, b = run_case(EngineCircuit, name), run_case(EngineCircuit, name)
        bad = [k for k in a if a[k].tobytes() != b[k].tobytes() or a[k].shape != b[k].shape]
        if bad:
            dropped.append(name)
            print("%s: %s differ between two runs: case left out" % (name, ", ".join(bad)))
            continue
        for k in a:
            rec["%s/%s" % (name, k)] = a[k]
        print("%s: meta %r, %s" % (name, a["meta"].tolist(), ", ".join("%s %r" % (k, a[k].shape) for k in a if k != "meta")))
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes), %d cases, left out: %s" % (out, os.path.getsize(out), len(CASES) - len(dropped), dropped or "none"))


if __name__ == "__main__":
    main()
