"""Expected hypervolume improvement: the errors the GPU tests measure, kept as a record -> profiles/ehvi_errors.txt.

Runs tests/test_gpu_ehvi.py and keeps what its comparisons print before they assert: per case of tests/_ehvi_truth.py and per
placement of the location the largest error of ``gp_ehvi_rows`` over the derived rounding bound (fold arithmetic) and over the
propagated posterior tolerance (against the oracle), the table against the rows, the decompositions from one cell to the caps,
the fallback route, and the loop's device acquisition against its host rule.

Run on the GPU box:  python tools/ehvi_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "ehvi_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_ehvi.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["expected hypervolume improvement: figures printed by tests/test_gpu_ehvi.py (largest error over the bound or tolerance "
            "named; 1 = at it)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("EHVI ") or line.startswith("MOBO"):
            keep.append(line[5:] if line.startswith("EHVI ") else line)
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
