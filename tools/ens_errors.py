"""Writes profiles/ens_errors.txt: runs tests/test_gpu_ensemble.py and tests/test_gpu_ensemble_sizes.py on the MI355X (pytest -s:
the suites print every figure before they assert it) and derives what the suites' tolerances are set from --
  checks 1 and 2, ensemble posteriors, fmin and integrated acquisitions against the oracle (lines TRUTH): per quantity the
           device's error, the float64 oracle's own scatter (direct-distance against Gram-trick oracle) and their ratio; MULT is the
           smallest power of two that leaves a factor 4 over the worst ratio among the quantities whose device error lies above
           the floor of the rule (1e-13 x scale);
  the rule's arithmetic (lines RULE), check 3, rows against table (lines ROWS-TABLE), and the model level (lines MODEL): the
           largest difference relative to the largest entry; the tolerance is the worst x 4 rounded up to a power of ten;
  the second module (the sizes the code branches on, against the long-double truth of tests/_ens_truth.py): the same figures in a
           section of its own, where the "oracle" of a TRUTH line is the float64 oracle's error against the truth and the floor
           is the one the line carries (1e-13 max(1, Npad / 384) x scale); posteriors and fmin apart from the integrated
           acquisitions, which carry a multiple of their own; RULE and ROWS-TABLE against the first module's tolerances; and the
           module's wall time (line SIZES).
Exits with the first non-zero pytest status.
usage: ens_errors.py [out.txt]        (default: profiles/ens_errors.txt)"""
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-13
TRUTH = re.compile(r"^\.*TRUTH (.+?)\s+scale (\S+)\s+device (\S+)\s+oracle (\S+)\s+ratio\s+(\S+)\s+bound (\S+)(?:\s+floor (\S+))?")
REL = re.compile(r"^\.*(ROWS-TABLE|RULE|MODEL) (.+?)\s+scale (\S+)\s+rel (\S+)\s+tol (\S+)")
ACQ = re.compile(r" (EI|LCB|MPI)\b")      # a TRUTH line of an integrated acquisition (the others: posteriors and fmin)
WALL = re.compile(r"^\.*SIZES wall time.*?: (\S+) s")


def power_of_ten_above(x):
    return 10.0 ** math.ceil(math.log10(x)) if x > 0 else 0.0


def run_module(name):
    """(pytest's status, its output, TRUTH rows (what, scale, device, oracle, floor), RULE / ROWS-TABLE / MODEL rows)."""
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", name), "-m", "gpu", "-q", "-s",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    truth, rel = [], {"ROWS-TABLE": [], "RULE": [], "MODEL": []}
    for line in run.stdout.splitlines():
        m = TRUTH.match(line)
        if m:
            scale = float(m.group(2))
            truth.append((m.group(1).strip(), scale, float(m.group(3)), float(m.group(4)), float(m.group(7)) if m.group(7) else FLOOR * scale))
        m = REL.match(line)
        if m:
            rel[m.group(1)].append((float(m.group(4)), m.group(2).strip(), float(m.group(3))))
    return run.returncode, run.stdout, truth, rel


def truth_section(truth, head):
    above = sorted(((dev / max(orc, 1e-300), what, scale, dev, orc) for what, scale, dev, orc, floor in truth if dev > floor), reverse=True)
    under = sorted(((dev / scale, what, scale, dev, orc) for what, scale, dev, orc, floor in truth if dev <= floor), reverse=True)
    worst = above[0][0] if above else 0.0
    mult = 1.0
    while mult < 4 * worst:
        mult *= 2
    text = head + ["   error is above that floor.  %d quantities, %d above the floor; worst ratio above the floor %.2f; x 4 = %.2f -> MULT = %g."
                   % (len(truth), len(above), worst, 4 * worst, mult),
                   "   the five largest ratios above the floor:"]
    text += ["     %8.2f  %s  (scale %.3e, device %.3e, oracle %.3e)" % r for r in above[:5]]
    text += ["   the five largest errors under the floor, relative to the scale:"]
    text += ["     %.3e  %s  (scale %.3e, device %.3e, oracle %.3e)" % r for r in under[:5]]
    text.append("")
    return text


def rel_sections(rel, names, keys, held=None):
    """``held``: the tolerance these comparisons are held to (the first module's); without it the tolerance is derived here."""
    text = []
    for key in keys:
        rows = sorted(rel[key], reverse=True)
        w = rows[0] if rows else (0.0, "none", 0.0)
        tol = "" if key == "MODEL" else " -> tolerance %.0e" % power_of_ten_above(4 * w[0]) if held is None else \
            "; held to the tolerance above, %.0e: %.1f x the worst" % (held, held / max(w[0], 1e-300))
        text += ["%s: %d comparisons, difference relative to the largest entry." % (names[key], len(rows)),
                 "   worst %.3e (%s, scale %.3e); x 4 = %.3e%s." % (w[0], w[1], w[2], 4 * w[0], tol),
                 "   the five largest:"]
        text += ["     %.3e  %s  (scale %.3e)" % r for r in rows[:5]]
        text.append("")
    return text


def last_line(out):
    return (out.strip().splitlines() or ["no output"])[-1]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ens_errors.txt")
    rc1, out1, truth, rel = run_module("test_gpu_ensemble.py")
    text = ["Ensemble entry points (gp_ens_fit, gp_ens_predict_rows, gp_ens_acq_rows, gp_ens_acq) on an MI355X: tools/ens_errors.py.",
            "pytest: " + last_line(out1), ""]
    text += truth_section(truth, [
        "1./2. Members' posteriors, fmin and the integrated acquisitions against the oracle; 1 / 3 / 4 / 5 / 8 rows, with and without noise.",
        "   Bound of the rule: max(MULT x the float64 oracle's scatter, 1e-13 x scale); a ratio counts for MULT where the device's"])
    names = {"RULE": "The rule's arithmetic (gp_ens_acq_rows against acquisitions._Rule over the device's own gp_ens_predict_rows, NumPy)",
             "ROWS-TABLE": "3. Rows against table (gp_ens_acq_rows against gp_ens_acq)",
             "MODEL": "6. The model level (GPModel_MCMC lists against OracleGP at 1e-6; the *_MCMC classes' device route against the "
                      "reference formulas at the two tolerances above)"}
    text += rel_sections(rel, names, ("RULE", "ROWS-TABLE", "MODEL"))

    rc2, out2, truth, rel = run_module("test_gpu_ensemble_sizes.py")
    wall = [m.group(1) for m in map(WALL.match, out2.splitlines()) if m]
    text += ["The sizes the code branches on (tests/test_gpu_ensemble_sizes.py: 7, 8, 9 and 16 tiles, S = 64, D = 64, tables of 512 / 513 /",
             "1100 rows, members on the jitter ladder) against the long-double truth of tests/_ens_truth.py.",
             "pytest: " + last_line(out2) + ("; the module's wall time, host-side truth included: %s s" % wall[-1] if wall else ""), ""]
    acq = [t for t in truth if ACQ.search(t[0])]
    post = [t for t in truth if not ACQ.search(t[0])]
    text += truth_section(post, [
        "Members' posteriors and fmin against the truth; 1 / 4 / 5 / 8 rows, with and without noise.",
        "   Bound: max(MULT x e64, 1e-13 max(1, Npad / 384) x scale), e64 (the column \"oracle\") the float64 direct-distance oracle's",
        "   own error against the truth for that quantity; the module keeps MULT = 64 from above.  A ratio counts where the device's"])
    text += truth_section(acq, [
        "The integrated acquisitions, rows (value, gradient) and table, against the truth: the same bound with a multiple of their own.",
        "   The large ratios are tail values (the scale column): every location of the call lies far above fmin, u = (fmin - m - jitter) / s",
        "   near -8, where EI = s (u Phi + phi) cancels to phi / u^2 and a posterior error dm shows as Phi(u) dm / EI ~ |u| dm / s, about 50 dm,",
        "   of the value.  The floor of the rule does not pass through that factor: a mean that is off by 4e-14 of its scale -- ten times",
        "   under the mean's own floor -- is 2e-12 of such an EI, above the EI's floor, and is then measured against what the float64",
        "   oracle happens to lose at that one location (tests/test_gpu_ensemble_sizes.py, docstring).  A ratio counts where the device's"])
    names = {"RULE": "The rule's arithmetic at these sizes (as above; and at S = 64 over all 64 posteriors)",
             "ROWS-TABLE": "Rows against table at 9 and 16 tiles, and a table against itself reversed (512 / 513 / 1100 rows)"}
    text += rel_sections(rel, names, ("RULE", "ROWS-TABLE"), held=1e-12)
    with open(out_path, "w") as f:
        f.write("\n".join(text))
    print("\n".join(text))
    sys.stdout.write("\n".join(out1.splitlines()[-25:] + out2.splitlines()[-25:]) + "\n")
    return rc1 or rc2


if __name__ == "__main__":
    sys.exit(main())
