"""Max-value entropy search: the existing kernels before and after -> profiles/mes_before_after.txt.

The feature adds instances and kernels of its own and leaves the EI / LCB / MPI kernels the code they were; this record holds what
was measured to show it: ``bench.py`` (the headline fit+predict step) and ``bench.py --small-calls`` (the one-location calls whose
finishing kernel has MES instances beside it) on the parent commit and on this tree, alternating in ONE visit.

The tool does not run the benchmarks: two checkouts are needed for that.  From each checkout's root, on the GPU box, alternating
parent and tree, i = 1, 2, ...:
    python bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline > DIR/bench_<side>_<i>.json
    python bench.py --small-calls --no-cpu-baseline                 > DIR/small_<side>_<i>.txt        (<side>: parent | tree)
then  python tools/mes_before_after.py DIR  assembles the record from those files; nothing in it is typed by hand.
"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "mes_before_after.txt")
SIDES = ("parent", "tree")


def main(src, what="max-value entropy search", dest=None):
    out = ["existing kernels before / after %s: the parent commit and this tree in ONE visit, alternating" % what, "",
           "bench.py --gpus 1 --steps 20 --warmup 3 (N = 16384, D = 8, M = 10000; ms per fit+predict step)"]
    for side in SIDES:
        v = []
        for f in sorted(glob.glob(os.path.join(src, "bench_%s_*.json" % side))):
            line = [x for x in open(f).read().splitlines() if x.startswith("{")][-1]
            v.append(json.loads(line)["ms_per_step"])
        out.append("  %-6s  %s   mean %.3f" % (side, "  ".join("%.3f" % x for x in v), sum(v) / len(v)))
    out += ["", "bench.py --small-calls --no-cpu-baseline (RBF, D = 8; ms per call: GPU predict, GPU acq_grad with EI; one pair per run)"]
    rows = {}
    for side in SIDES:
        for f in sorted(glob.glob(os.path.join(src, "small_%s_*.txt" % side))):
            for line in open(f):
                p = line.split("|")
                if len(p) >= 3 and p[0].split() and p[0].split()[0].isdigit():
                    N, M = p[0].split()
                    a, b = p[1].split()
                    rows.setdefault((int(N), int(M)), {}).setdefault(side, []).append((float(a), float(b)))
    out.append("%6s %5s | %-31s | %-31s" % ("N", "M", "parent: predict acq_grad ...", "tree: predict acq_grad ..."))
    for k in sorted(rows):
        cell = lambda s: "  ".join("%.3f %.3f" % x for x in rows[k].get(s, []))     # noqa: E731
        out.append("%6d %5d | %-31s | %-31s" % (k[0], k[1], cell("parent"), cell("tree")))
    open(dest or OUT, "w").write("\n".join(out) + "\n")
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/mes_before_after.py DIR   (see the docstring for what DIR holds)")
    sys.exit(main(sys.argv[1]))
