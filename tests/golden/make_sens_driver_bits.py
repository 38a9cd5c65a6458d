"""Records one golden file of tests/sens_driver_bits_cases.py (GOLDEN_FILES: sens_driver_bits.npz, loopgain_bits.npz): the outputs of
the sensitivity drivers for the cases that file holds, as computed by the library that is built in the tree (or the one CEDARHIP_LIB
names).  Run on the GPU at the commit whose results are to be pinned:

    python tests/golden/make_sens_driver_bits.py [--file loopgain_bits.npz] [output.npz]

--file names the subset (default sens_driver_bits.npz); the output defaults to that file beside this script.
Every case is run twice in this process; a case whose two results are not bit-for-bit equal is reported and left out, and the
exit status is then 1.  Record in two separate processes as well and compare the two files (`cmp`) before committing one."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root

from sens_driver_bits_cases import CASES, GOLDEN_FILES, golden_file, run_case  # noqa: E402


def main():
    args = sys.argv[1:]
    which = "sens_driver_bits.npz"
    if args[:1] == ["--file"]:
        if len(args) < 2 or args[1] not in GOLDEN_FILES:
            sys.exit("usage: make_sens_driver_bits.py [--file {%s}] [output.npz]" % ",".join(GOLDEN_FILES))
        which, args = args[1], args[2:]
    names = [n for n in CASES if golden_file(n) == which]
    out = args[0] if args else os.path.join(HERE, which)
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    rec, dropped = {}, []
    for name in names:
        t0 = time.time()
        a, b = run_case(EngineCircuit, name), run_case(EngineCircuit, name)
        bad = [k for k in a if k not in b or a[k].tobytes() != b[k].tobytes() or a[k].shape != b[k].shape]
        if bad:
            dropped.append(name)
            print("%s: %s differ between two runs: case left out" % (name, ", ".join(bad)))
            continue
        for k in a:
            rec["%s/%s" % (name, k)] = a[k]
        print("%s: %.1f s for two runs, meta %r, %s" % (name, time.time() - t0, a["meta"].tolist(),
                                                         ", ".join("%s %r" % (k, a[k].shape) for k in a if k not in ("meta", "stats_names"))), flush=True)
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes), %d cases, left out: %s" % (out, os.path.getsize(out), len(names) - len(dropped), dropped or "none"))
    return 1 if dropped else 0


if __name__ == "__main__":
    sys.exit(main())
