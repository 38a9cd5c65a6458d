"""Records tests/golden/api_layer_bits.npz (CPU: the user-facing analyses against the stand-in engine) or tests/golden/api_gpu_bits.npz
(GPU: the same analyses end to end) for the cases of tests/api_bits_cases.py, as computed by the tree it is run in.  Run at the commit
whose results are to be pinned:

    python tests/golden/make_api_bits.py cpu [output.npz]
    python tests/golden/make_api_bits.py gpu [output.npz]        (on the GPU)

Every case is run twice in this process; a case whose two results are not bit-for-bit equal is reported and left out.  Record in two
separate processes as well and compare the two files (`cmp`) before committing one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root

from api_bits_cases import CPU_CASES, GPU_CASES, record  # noqa: E402


def main():
    which = sys.argv[1]
    cases, default = {"cpu": (CPU_CASES, "api_layer_bits.npz"), "gpu": (GPU_CASES, "api_gpu_bits.npz")}[which]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, default)
    rec, dropped = record(cases)
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes), %d cases, left out: %s" % (out, os.path.getsize(out), len(cases) - len(dropped), dropped or "none"))


if __name__ == "__main__":
    main()
