"""Writes profiles/sparse_gp_errors.txt: runs tests/test_gpu_sparse_gp.py on the MI355X (pytest -s: the suite prints every figure
before it asserts it) and tabulates, per case and quantity, the device's error and the float64 oracle's error against the
long-double truth, their ratio, and whether the device's error lies above the floor of the tolerance rule -- what the suite's
multiple is set from.  Exits with pytest's status.
usage: sparse_errors.py [out.txt]        (default: profiles/sparse_gp_errors.txt)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-13
LINE = re.compile(r"^\.*(.+?)\s+scale (\S+)\s+device (\S+)\s+oracle (\S+)\s+ratio\s+(\S+)\s+bound (\S+)")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_gp_errors.txt")
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_sparse_gp.py"), "-m", "gpu", "-q", "-s",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    rows, seen = [], set()
    for line in run.stdout.splitlines():
        m = LINE.match(line)
        if m and m.group(1).strip() not in seen:
            seen.add(m.group(1).strip())
            rows.append((m.group(1).strip(), float(m.group(2)), float(m.group(3)), float(m.group(4))))
    above = [(dev / max(orc, 1e-300), what) for what, scale, dev, orc in rows if dev > FLOOR * scale]
    worst = max(above) if above else (0.0, "none")
    under = max((dev / max(orc, 1e-300), what) for what, scale, dev, orc in rows if dev <= FLOOR * scale) if rows else (0.0, "none")
    mult = 1.0
    while mult < 4 * worst[0]:
        mult *= 2
    text = ["Sparse GP (gp_sparse_fit_grad, gp_sparse_posterior, gp_sparse_predict, gp_sparse_fmin) on an MI355X: tools/sparse_errors.py.",
            "Per case and quantity: the largest entry of the long-double truth (scale), the device's largest error against it, the float64",
            "oracle's (tests/_sparse_ref.py, LAPACK) on the same inputs, and their ratio.  The bound of the tolerance rule is",
            "max(MULT x oracle error, 1e-13 x scale); a ratio counts for MULT where the device's error is above that floor.  Below it the",
            "floor is the bound and the oracle's own error is often a lucky 1e-17: the largest ratio there is %.2f (%s)." % under,
            "%d quantities, %d above the floor; worst ratio above the floor %.2f (%s); x 4 = %.2f -> MULT = %g."
            % (len(rows), len(above), worst[0], worst[1], 4 * worst[0], mult),
            "pytest: " + (run.stdout.strip().splitlines() or ["no output"])[-1], ""]
    for what, scale, dev, orc in rows:
        text.append("%-46s scale %.3e  device %.3e  oracle %.3e  ratio %8.2f  %s"
                    % (what, scale, dev, orc, dev / max(orc, 1e-300), "ABOVE the floor" if dev > FLOOR * scale else "under the floor"))
    with open(out_path, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text[:7]))
    if run.returncode:
        print(run.stdout[-4000:])
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
