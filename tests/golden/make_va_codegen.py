"""Writes tests/golden/va_codegen_*.hpp: the header `va.codegen.generate_header` emits (empty source tag) for the project's own
library (cedarsim.jl_amd/va/library/cedar_basic.va) and for the two torture modules of tests/test_va_compiler.py.  Recorded from
the commit BEFORE the generator was split into passes, so that the test compares the regrouped generator with its parent and not
with itself; run it again only when the generated text is changed on purpose."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from cedarsim_jl_amd.va.codegen import generate_header  # noqa: E402
from test_va_compiler import codegen_golden_modules  # noqa: E402

if __name__ == "__main__":
    for name, mods in codegen_golden_modules().items():
        with open(os.path.join(HERE, "va_codegen_%s.hpp" % name), "w") as f:
            f.write(generate_header(mods))
