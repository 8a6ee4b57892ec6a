"""Mean function: the errors the GPU tests measure against the long-double truth, kept as a record -> profiles/mean_errors.txt.

Runs tests/test_gpu_mean_function.py (pytest -s: the module prints every figure before it asserts it) -- or reads the saved
output of such a run -- and keeps, from its TRUTH lines (tests/test_gpu_ensemble_sizes.py's format: what, scale, the device's error,
the float64 oracle's error against the same truth, their ratio, the bound max(64 x oracle, floor) and the floor): the count, how
many device errors lie above the floor, the worst multiple of the oracle's error among those, the ten largest, and per group of
quantities (fit, tables, rows, scores) the largest error over its bound.  GOWER and MODEL lines are kept as they are.

Run on the GPU box:  python tools/mean_errors.py            (runs the module)
                     python tools/mean_errors.py run.log    (reads a saved `pytest -s` output of the module)
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "mean_errors.txt")
TRUTH = re.compile(r"^\.*TRUTH (.+?)\s+scale (\S+)\s+device (\S+)\s+oracle (\S+)\s+ratio\s+(\S+)\s+bound (\S+)\s+floor (\S+)")
GROUPS = (("fit and gradients", re.compile(r"^\w: ")), ("tables", re.compile(r"^\w table \d+ (mean|var|dmdx|dvdx)")),
          ("rows", re.compile(r"^\w rows \d+ (mean|var|dmdx|dvdx)")), ("scores", re.compile(r"(EI|LCB|MPI|fmin)")),
          ("model", re.compile(r"^model")))


def main():
    if len(sys.argv) > 1:
        text, status = open(sys.argv[1]).read(), 0
    else:
        run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_mean_function.py"), "-m", "gpu", "-q", "-s",
                              "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        text, status = run.stdout, run.returncode
    rows, other = [], []
    for line in text.splitlines():
        m = TRUTH.match(line)
        if m:
            rows.append((m.group(1).strip(),) + tuple(float(m.group(i)) for i in (2, 3, 4, 6, 7)))
        elif re.match(r"^\.*(GOWER|MODEL|BO) ", line):
            other.append("    " + line.lstrip("."))
    above = sorted(((dev / max(orc, 1e-300), what, scale, dev, orc) for what, scale, dev, orc, bound, floor in rows if dev > floor),
                   reverse=True)
    keep = ["mean function: figures printed by tests/test_gpu_mean_function.py against the long-double truth of tests/_mean_truth.py",
            "(bound of every line: max(64 x the float64 oracle's own error, 1e-13 max(1, Npad / 384) x scale))", "",
            "%d quantities, %d with a device error above the floor; worst multiple of the oracle's error among those: %.2f (MULT = 64)"
            % (len(rows), len(above), above[0][0] if above else 0.0), "", "the ten largest multiples above the floor:"]
    keep += ["    %8.2f  %s  (scale %.3e, device %.3e, oracle %.3e)" % r for r in above[:10]]
    keep += ["", "largest error over its bound, per group:"]
    for name, pat in GROUPS:
        sel = [(dev / bound, what) for what, scale, dev, orc, bound, floor in rows if pat.search(what)]
        if sel:
            worst = max(sel)
            keep.append("    %-18s %4d quantities, worst %.3f of the bound  (%s)" % (name, len(sel), worst[0], worst[1]))
    keep += ["", "other lines:"] + other + ["", text.strip().splitlines()[-1] if text.strip() else ""]
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    return status


if __name__ == "__main__":
    sys.exit(main())
