"""Writes profiles/ens_errors.txt: runs tests/test_gpu_ensemble.py on the MI355X (pytest -s: the suite prints every figure
before it asserts it) and derives what the suite's tolerances are set from --
  checks 1 and 2, ensemble posteriors, fmin and integrated acquisitions against the oracle (lines TRUTH): per quantity the
           device's error, the float64 oracle's own scatter (direct-distance against Gram-trick oracle) and their ratio; MULT is the
           smallest power of two that leaves a factor 4 over the worst ratio among the quantities whose device error lies above
           the floor of the rule (1e-13 x scale);
  the rule's arithmetic (lines RULE), check 3, rows against table (lines ROWS-TABLE), and the model level (lines MODEL): the
           largest difference relative to the largest entry; the tolerance is the worst x 4 rounded up to a power of ten.
Exits with pytest's status.
usage: ens_errors.py [out.txt]        (default: profiles/ens_errors.txt)"""
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-13
TRUTH = re.compile(r"^\.*TRUTH (.+?)\s+scale (\S+)\s+device (\S+)\s+oracle (\S+)\s+ratio\s+(\S+)\s+bound (\S+)")
REL = re.compile(r"^\.*(ROWS-TABLE|RULE|MODEL) (.+?)\s+scale (\S+)\s+rel (\S+)\s+tol (\S+)")


def power_of_ten_above(x):
    return 10.0 ** math.ceil(math.log10(x)) if x > 0 else 0.0


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ens_errors.txt")
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_ensemble.py"), "-m", "gpu", "-q", "-s",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    truth, rel = [], {"ROWS-TABLE": [], "RULE": [], "MODEL": []}
    for line in run.stdout.splitlines():
        m = TRUTH.match(line)
        if m:
            truth.append((m.group(1).strip(), float(m.group(2)), float(m.group(3)), float(m.group(4))))
        m = REL.match(line)
        if m:
            rel[m.group(1)].append((float(m.group(4)), m.group(2).strip(), float(m.group(3))))
    above = sorted(((dev / max(orc, 1e-300), what, scale, dev, orc) for what, scale, dev, orc in truth if dev > FLOOR * scale), reverse=True)
    under = sorted(((dev / scale, what, scale, dev, orc) for what, scale, dev, orc in truth if dev <= FLOOR * scale), reverse=True)
    worst = above[0][0] if above else 0.0
    mult = 1.0
    while mult < 4 * worst:
        mult *= 2
    text = ["Ensemble entry points (gp_ens_fit, gp_ens_predict_rows, gp_ens_acq_rows, gp_ens_acq) on an MI355X: tools/ens_errors.py.",
            "pytest: " + (run.stdout.strip().splitlines() or ["no output"])[-1], "",
            "1./2. Members' posteriors, fmin and the integrated acquisitions against the oracle; 1 / 3 / 4 / 5 / 8 rows, with and without noise.",
            "   Bound of the rule: max(MULT x the float64 oracle's scatter, 1e-13 x scale); a ratio counts for MULT where the device's",
            "   error is above that floor.  %d quantities, %d above the floor; worst ratio above the floor %.2f; x 4 = %.2f -> MULT = %g."
            % (len(truth), len(above), worst, 4 * worst, mult),
            "   the five largest ratios above the floor:"]
    text += ["     %8.2f  %s  (scale %.3e, device %.3e, oracle %.3e)" % r for r in above[:5]]
    text += ["   the five largest errors under the floor, relative to the scale:"]
    text += ["     %.3e  %s  (scale %.3e, device %.3e, oracle %.3e)" % r for r in under[:5]]
    text.append("")
    names = {"RULE": "The rule's arithmetic (gp_ens_acq_rows against acquisitions._Rule over the device's own gp_ens_predict_rows, NumPy)",
             "ROWS-TABLE": "3. Rows against table (gp_ens_acq_rows against gp_ens_acq)",
             "MODEL": "6. The model level (GPModel_MCMC lists against OracleGP at 1e-6; the *_MCMC classes' device route against the "
                      "reference formulas at the two tolerances above)"}
    for key in ("RULE", "ROWS-TABLE", "MODEL"):
        rows = sorted(rel[key], reverse=True)
        w = rows[0] if rows else (0.0, "none", 0.0)
        text += ["%s: %d comparisons, difference relative to the largest entry." % (names[key], len(rows)),
                 "   worst %.3e (%s, scale %.3e); x 4 = %.3e%s." % (w[0], w[1], w[2], 4 * w[0], "" if key == "MODEL" else
                                                                   " -> tolerance %.0e" % power_of_ten_above(4 * w[0])),
                 "   the five largest:"]
        text += ["     %.3e  %s  (scale %.3e)" % r for r in rows[:5]]
        text.append("")
    with open(out_path, "w") as f:
        f.write("\n".join(text))
    print("\n".join(text))
    sys.stdout.write("\n".join(run.stdout.splitlines()[-25:]) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
