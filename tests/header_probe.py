"""What include/ketogpu.h says to a C compiler: one gcc program per call that prints the values of C expressions
(sizeof(...), offsetof(...), constants).  The layout tests compare them with keto_amd._lib's ctypes structs."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def probe(exprs):
    """The integer values of the C expressions `exprs` (non-negative, at most 64 bits), in their order."""
    exprs = list(exprs)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ketogpu.h"\n'
                    "int main(void) {\n  unsigned long long v[] = {\n"
                    + "".join(f"    (unsigned long long)({e}),\n" for e in exprs)
                    + '  };\n  for (size_t i = 0; i < sizeof v / sizeof *v; i++) printf("%llu\\n", v[i]);\n  return 0;\n}\n')
        subprocess.run(["gcc", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert len(got) == len(exprs)
    return got
