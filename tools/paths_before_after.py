"""Posterior paths: the existing kernels before and after -> profiles/paths_before_after.txt.

The feature adds kernels and entries of its own and changes no existing one; this record holds what was measured to show it:
``bench.py`` and ``bench.py --small-calls`` on the parent commit and on this tree, alternating in ONE visit.  The runs and the file
layout are those of tools/mes_before_after.py (see its docstring); this tool assembles the record from them.

    python tools/paths_before_after.py DIR
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mes_before_after  # noqa: E402

OUT = os.path.join(mes_before_after.ROOT, "profiles", "paths_before_after.txt")

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/paths_before_after.py DIR   (tools/mes_before_after.py says what DIR holds)")
    sys.exit(mes_before_after.main(sys.argv[1], what="posterior paths", dest=OUT))
