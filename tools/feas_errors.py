"""Black-box constraints: the errors the GPU tests measure, kept as a record -> profiles/feas_errors.txt.

Runs tests/test_gpu_feas.py and keeps what its comparisons print before they assert: per case of tests/_feas_truth.py and per
placement of z the largest error of ``gp_feas_rows`` over the derived rounding bound (fold arithmetic) and over the propagated
posterior tolerance (against the oracle), the tables against the rows, the flagged scores and ``gp_acq_rows_feas``.

Run on the GPU box:  python tools/feas_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "feas_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_feas.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["probability of feasibility: figures printed by tests/test_gpu_feas.py (largest error over the bound or tolerance named; "
            "1 = at it)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("FEAS "):
            keep.append(line[5:])
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
