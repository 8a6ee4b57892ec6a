"""Cost-aware EI / MPI: the errors the GPU tests measure, kept as a record -> profiles/cost_errors.txt.

Runs tests/test_gpu_cost.py and keeps what its comparisons print before they assert: per case of tests/_cost_truth.py the largest
error of ``gp_cost_rows`` over its derived bound (log cost and gradient), and per scoring entry the largest error of the flagged
scores over theirs (value, then gradient).

Run on the GPU box:  python tools/cost_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "cost_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_cost.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["cost surface and flagged scores: figures printed by tests/test_gpu_cost.py (largest error over the derived bound; 1 = at "
            "the bound)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("_") and " test_" in line:
            keep.append(line.strip("_ "))
        elif "error / bound" in line:
            keep.append("    " + line)
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
