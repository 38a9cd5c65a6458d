"""Writes tests/golden/sparse_path_trace.json (or the file named on the command line): what the sparse path computes on the GPU for
the cases of tests/sparse_path_cases.py — per case and run the return code, the per-sample status, `info()`, every integer field of
the stats and the DC solution / the saved rows as `float.hex` strings.

Recorded on an MI355X from the commit BEFORE the host side of the sparse path was reorganised (one plan table, named passes, the
Newton policy in ch_sparse_newton.hpp), so that tests/test_gpu_sparse_trace.py compares the reorganised host code with its parent
and not with itself.  Recorded twice there; the two recordings were identical in every quantity, so the test asks for equality.
Run it again only when the sparse path is changed on purpose."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import sparse_path_cases as sc  # noqa: E402

if __name__ == "__main__":
    from cedarsim_jl_amd.engine import EngineCircuit, load_library
    load_library()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sparse_path_trace.json")
    cases = {}
    for name in sc.CASES:
        t0 = time.time()
        cases[name] = sc.run_case(EngineCircuit, name)
        print("%-24s %.2f s  %s" % (name, time.time() - t0, "; ".join(
            "%s rc %d path %d iters %d launches %d" % (r["kind"], r["rc"], r["info"]["path"], r["stats"]["nnonliniter"], r["stats"]["n_kernel_launches"])
            for r in cases[name])), flush=True)
    with open(out, "w") as f:
        f.write('{"cases": {\n' + ",\n".join("%s: [\n%s\n]" % (json.dumps(k), ",\n".join(json.dumps(r) for r in v)) for k, v in cases.items()) + "\n}}\n")
