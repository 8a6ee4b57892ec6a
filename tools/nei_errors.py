"""Noisy expected improvement: the errors the GPU tests measure, kept as a record -> profiles/nei_errors.txt.

Runs tests/test_gpu_nei.py and keeps what its comparisons print before they assert: per case of tests/_nei_truth.py the error of
the fantasies and of their minima over the relative tolerance at the model's noise, the worst error of the table's and of the rows
entry's values over their first-order allowances, rows against table over the twin's relative tolerance, the gradient's error
beside the error of the same algorithm in plain float64 (and their ratio), S = 1 against gp_acq on the fantasy, and the end-to-end
suggestion beside EI's.

Run on the GPU box:  python tools/nei_errors.py            (or, from a saved `pytest -s` output of that file:
                      python tools/nei_errors.py OUTPUT.txt)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "nei_errors.txt")


def main():
    if len(sys.argv) > 1:
        run = subprocess.CompletedProcess([], 0, stdout=open(sys.argv[1]).read())
    else:
        run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_nei.py"), "-m", "gpu", "-q", "-rP",
                              "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["noisy expected improvement: figures printed by tests/test_gpu_nei.py (errors over the allowance named; 1 = at it)", ""]
    for line in run.stdout.splitlines():
        line = line.lstrip(".")      # (under -s a line follows the progress dots of the tests before it)
        if line.startswith("nei "):
            keep.append(line[4:])
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    if run.returncode:
        print(run.stdout[-6000:])
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
