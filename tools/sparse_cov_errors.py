"""Writes profiles/sparse_cov_errors.txt: runs tests/test_gpu_sparse_cov.py on the MI355X (pytest -s: the suite prints every
figure before it asserts it) and derives what the suite's MULT is set from -- per quantity (mean, full covariance with and without
noise, its diagonal against the unclipped variance, between-points covariance) the device's error against the long-double truth,
the float64 oracle's and their ratio; MULT is the smallest power of two that leaves a factor 4 over the worst ratio among the
quantities whose device error lies above the floor of the rule (1e-13 x scale).  The factor's and the draws' figures (lines
"samples", "singular case", "model", "entropy search") are copied as the suite printed them.  Exits with pytest's status.
usage: sparse_cov_errors.py [out.txt]        (default: profiles/sparse_cov_errors.txt)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-13
VARIANCE, EPS = 1.3, 2.220446049250313e-16      # the prior variance of the suite's runs (tests/_sparse_ref.py), the ulp of 1
TRUTH = re.compile(r"^\.*(.+?)\s+scale (\S+)\s+device (\S+)\s+oracle (\S+)\s+ratio\s+(\S+)\s+bound (\S+)")
FACTOR = re.compile(r"^\.*(.+?: samples noise=\d)\s+jitter (\S+)\s+\|C C\^T - cov - jit I\| / max\|cov\| (\S+)")
OTHER = re.compile(r"^\.*((?:.+?: samples noise=1\s+(?:factor|four draws)|singular case|model:|entropy search|between-points after).*)$")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_cov_errors.txt")
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_sparse_cov.py"), "-m", "gpu", "-q", "-s",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    truth, seen, factor, draws, other = [], set(), [], [], []
    for line in run.stdout.splitlines():
        m = TRUTH.match(line)
        if m and m.group(1).strip() not in seen:
            seen.add(m.group(1).strip())
            truth.append((m.group(1).strip(), float(m.group(2)), float(m.group(3)), float(m.group(4))))
            continue
        m = FACTOR.match(line)
        if m:
            factor.append((float(m.group(3)), m.group(1).strip(), float(m.group(2))))
            continue
        m = OTHER.match(line)
        if m:
            (draws if "samples noise=1" in m.group(1) else other).append(m.group(1).strip())
    above = [(dev / max(orc, 1e-300), what, scale, dev, orc) for what, scale, dev, orc in truth if dev > FLOOR * scale]
    worst = max(above) if above else (0.0, "none", 1.0, 0.0, 0.0)
    under = max([(dev / max(orc, 1e-300), what) for what, scale, dev, orc in truth if dev <= FLOOR * scale] or [(0.0, "none")])
    mult = 1.0
    while mult < 4 * worst[0]:
        mult *= 2
    text = ["The joint posterior of the sparse GP (gp_sparse_predict_full_cov, gp_sparse_posterior_samples, gp_sparse_cov_between) on an "
            "MI355X: tools/sparse_cov_errors.py.",
            "pytest: " + (run.stdout.strip().splitlines() or ["no output"])[-1], "",
            "1. Mean, full covariance (130 / 128 / 5 / 1 rows, with and without noise), its diagonal against the unclipped variance and the",
            "   between-points covariance (R = 1 / 50 / 130, M1 = 1 / 5 / 8 / 9 / 130) against the long-double truth.",
            "   Bound of the rule: max(MULT x the float64 oracle's error, 1e-13 x scale); a ratio counts for MULT where the device's error",
            "   is above that floor.  Below it the floor is the bound and the oracle's own error is often a lucky 1e-17: the largest",
            "   ratio there is %.2f (%s)." % under,
            "   %d quantities, %d above the floor; worst ratio above the floor %.2f (%s); x 4 = %.2f -> MULT = %g."
            % (len(truth), len(above), worst[0], worst[1], 4 * worst[0], mult),
            "   %s   scale %.3e  device %.3e  oracle %.3e  ratio %.2f" % (worst[1], worst[2], worst[3], worst[4], worst[0])]
    if mult > 8:
        text += ["   MULT is above the sparse suite's 8.  The floor of the rule is taken from the largest entry of the RESULT; every entry of",
                 "   these matrices is the difference of terms of the order of the prior variance %.1f, whose ulp is %.1e." % (VARIANCE, VARIANCE * EPS)]
        if worst[3] < VARIANCE * EPS:
            text += ["   The worst case is a block whose largest entry is %.1e: its floor lies at %.1e, far below one rounding of the terms"
                     % (worst[2], FLOOR * worst[2]),
                     "   subtracted.  The device's error there is %.2f ulp of those terms and the oracle's %.2f: both are the luck of one"
                     % (worst[3] / (VARIANCE * EPS), worst[4] / (VARIANCE * EPS)),
                     "   rounding, and their quotient says nothing about the summation.  The largest error of the suite in those units is",
                     "   %.0f ulp (%s), where the float64 oracle is off by %.0f ulp: the error of woodbury_inv at cond(Kmm) 8.9e4."
                     % max((dev / (VARIANCE * EPS), what, orc / (VARIANCE * EPS)) for what, scale, dev, orc in truth)]
        else:
            text += ["   The worst case's device error is %.2f ulp of those terms, the oracle's %.2f."
                     % (worst[3] / (VARIANCE * EPS), worst[4] / (VARIANCE * EPS))]
    text += ["",
             "2. The factor of gp_sparse_posterior_samples, max|C C^T - cov - jit I| / max|cov| (bound 1e-12; jitter 0 asserted on every run):",
             "   %d factorisations, worst %.3e (%s); jitters seen: %s." % ((len(factor),) + (max(factor)[:2] if factor else (0.0, "none")) +
                                                                         (sorted(set(j for _, _, j in factor)),)),
             "   against numpy's Cholesky of the float64 oracle's covariance, noise in (bound 1e-6 of the largest entry): worst %s."
             % max([float(d.split()[-1]) for d in draws] or [0.0]), ""]
    text += ["3. As the suite printed them:"] + ["   " + o for o in other] + [""]
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
    print("\n".join(text[:40]))
    if run.returncode:
        print(run.stdout[-4000:])
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
