"""Writes profiles/sparse_acq_errors.txt: runs tests/test_gpu_sparse_acq.py on the MI355X (pytest -s: the suite prints every
figure before it asserts it) and derives what the suite's three tolerances are set from --
  check 1, rows posterior against the long-double truth: per quantity the device's error, the float64 oracle's and their ratio;
           MULT is the smallest power of two that leaves a factor 4 over the worst ratio among the quantities whose device
           error lies above the floor of the rule (1e-13 x scale);
  check 2, rows against table (lines ROWS-TABLE, and MODEL for the model level) and check 3, the rule's arithmetic (lines RULE):
           the largest difference relative to the largest entry; the tolerance is the worst x 4 rounded up to a power of ten.
Exits with pytest's status.
usage: sparse_acq_errors.py [out.txt]        (default: profiles/sparse_acq_errors.txt)"""
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-13
TRUTH = re.compile(r"^\.*(.+?)\s+scale (\S+)\s+device (\S+)\s+oracle (\S+)\s+ratio\s+(\S+)\s+bound (\S+)")
REL = re.compile(r"^\.*(ROWS-TABLE|RULE|MODEL) (.+?)\s+scale (\S+)\s+rel (\S+)\s+tol (\S+)")


def power_of_ten_above(x):
    return 10.0 ** math.ceil(math.log10(x)) if x > 0 else 0.0


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_acq_errors.txt")
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_sparse_acq.py"), "-m", "gpu", "-q", "-s",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    truth, rel, seen = [], {"ROWS-TABLE": [], "RULE": [], "MODEL": []}, set()
    for line in run.stdout.splitlines():
        m = TRUTH.match(line)
        if m and m.group(1).strip() not in seen:
            seen.add(m.group(1).strip())
            truth.append((m.group(1).strip(), float(m.group(2)), float(m.group(3)), float(m.group(4))))
        m = REL.match(line)
        if m:
            rel[m.group(1)].append((float(m.group(4)), m.group(2).strip(), float(m.group(3))))
    above = [(dev / max(orc, 1e-300), what) for what, scale, dev, orc in truth if dev > FLOOR * scale]
    worst = max(above) if above else (0.0, "none")
    under = max([(dev / max(orc, 1e-300), what) for what, scale, dev, orc in truth if dev <= FLOOR * scale] or [(0.0, "none")])
    mult = 1.0
    while mult < 4 * worst[0]:
        mult *= 2
    text = ["Acquisitions over the sparse GP (gp_sparse_predict_rows, gp_sparse_acq_rows, gp_sparse_acq) on an MI355X: "
            "tools/sparse_acq_errors.py.",
            "pytest: " + (run.stdout.strip().splitlines() or ["no output"])[-1], "",
            "1. Rows posterior (csrc/sparse_rows.hip) against the long-double truth, 1 / 4 / 5 / 8 locations, with and without noise.",
            "   Bound of the rule: max(MULT x the float64 oracle's error, 1e-13 x scale); a ratio counts for MULT where the device's error",
            "   is above that floor.  Below it the floor is the bound and the oracle's own error is often a lucky 1e-17: the largest",
            "   ratio there is %.2f (%s)." % under,
            "   %d quantities, %d above the floor; worst ratio above the floor %.2f (%s); x 4 = %.2f -> MULT = %g."
            % (len(truth), len(above), worst[0], worst[1], 4 * worst[0], mult), ""]
    names = {"ROWS-TABLE": "2. Rows against table (gp_sparse_predict_rows / gp_sparse_acq_rows against gp_sparse_predict / gp_sparse_acq)",
             "RULE": "3. The rule's arithmetic (gp_sparse_acq against acquisitions._Rule and the oracle's penaliser in float64 NumPy / SciPy)",
             "MODEL": "7. The model level (GPModel twins with device_acquisitions on and off; held to the tolerance of 2.)"}
    for key in ("ROWS-TABLE", "RULE", "MODEL"):
        rows = rel[key]
        w = max(rows) if rows else (0.0, "none", 0.0)
        text += ["%s: %d comparisons, difference relative to the largest entry." % (names[key], len(rows)),
                 "   worst %.3e (%s, scale %.3e); x 4 = %.3e%s." % (w[0], w[1], w[2], 4 * w[0], "" if key == "MODEL" else
                                                                         " -> tolerance %.0e" % power_of_ten_above(4 * w[0])),
                 "   the five largest:"]
        text += ["     %.3e  %s  (scale %.3e)" % t for t in sorted(rows, reverse=True)[:5]] + [""]
    text.append("Check 1, every quantity above the floor and the worst of each run below it:")
    per_run = {}
    for what, scale, dev, orc in truth:
        hi = dev > FLOOR * scale
        line = "%-46s scale %.3e  device %.3e  oracle %.3e  ratio %8.2f  %s" % (what, scale, dev, orc, dev / max(orc, 1e-300),
                                                                               "ABOVE the floor" if hi else "under the floor")
        if hi:
            text.append(line)
        else:
            run_id = what.split(":")[0]
            if run_id not in per_run or dev / scale > per_run[run_id][0]:
                per_run[run_id] = (dev / scale, line)
    text += [v[1] for v in per_run.values()]
    with open(out_path, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text[:30]))
    if run.returncode:
        print(run.stdout[-4000:])
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
