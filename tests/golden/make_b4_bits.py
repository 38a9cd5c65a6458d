"""Records tests/golden/b4_bits.npz: the BSIM4 stamps over the card space and the device stepper's complete outputs for the shapes
of tests/b4_bits_cases.py, as computed by the library that is built in the tree.  Run on the GPU at the commit whose results are
to be pinned:

    python tests/golden/make_b4_bits.py [output.npz]

Every case is run twice in this process and the two results must be bit-for-bit equal before anything is written; record in two
separate processes as well and compare the two files (`cmp`) before committing one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # repository root

import bsim4_cards as BC  # noqa: E402
import b4_bits_cases as B  # noqa: E402


def same(a, b, what):
    for k in a:
        if a[k].tobytes() != b[k].tobytes() or a[k].shape != b[k].shape:
            sys.exit("%s/%s differs between two runs: nothing written" % (what, k))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else B.GOLDEN
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    rec = {}
    temps = {}
    for name, temp in B.STAMP_CASES:
        temps.setdefault(name, []).append(temp)
    for name, tt in temps.items():
        a, b = B.run_stamps(EngineCircuit, name, tt), B.run_stamps(EngineCircuit, name, tt)
        same(a, b, "stamps " + name)
        rec.update(a)
        print("stamps %-9s %s: %d NaN entries" % (name, sorted(a), sum(int(np.isnan(x).sum()) for x in a.values())))
    for name in B.CHAIN_CANDIDATES:
        both = {}
        for label, nopair in (("pair", False), ("nopair", True)):
            if nopair:
                os.environ["CEDARHIP_PERSIST_NOPAIR"] = "1"
            try:
                (rc1, a), (rc2, b) = B.run_chain(EngineCircuit, name), B.run_chain(EngineCircuit, name)
            finally:
                os.environ.pop("CEDARHIP_PERSIST_NOPAIR", None)
            if rc1 != rc2:
                sys.exit("chain %s %s: return codes %d and %d" % (name, label, rc1, rc2))
            if rc1 != 0:
                if name in BC.CIRCUIT_NAMES:
                    sys.exit("chain %s %s returned %d" % (name, label, rc1))
                print("chain %-5s %-6s returned %d: not recorded" % (name, label, rc1))
                both = None
                break
            same(a, b, "chain %s %s" % (name, label))
            both[label] = a
            print("chain %-5s %-6s meta (stepper, mode, accepted, rejected, iterations) %r" % (name, label, a["meta"].tolist()))
        if both:
            for label, a in both.items():
                for k in a:
                    rec["chain/%s/%s/%s" % (name, label, k)] = a[k]
    a, b = B.run_own(EngineCircuit), B.run_own(EngineCircuit)
    same(a, b, "own")
    for k in a:
        rec["own/%s" % k] = a[k]
    print("own: meta %r, t %r, v %r, xf %r" % (a["meta"].tolist(), a["t"].shape, a["v"].shape, a["xf"].shape))
    np.savez_compressed(out, **rec)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
