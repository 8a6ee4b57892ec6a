"""Posterior paths: the errors the GPU tests measure, kept as a record -> profiles/paths_errors.txt.

Runs tests/test_gpu_paths.py and keeps what its comparisons print before they assert: per case of tests/_paths_truth.py the largest
error of ``gp_paths_table`` and of ``gp_paths_rows`` (values and gradients, calls of 1 and of 8 rows) over their allowance -- the
derived bound of the prior term plus the posterior-mean tolerance of the update term --, the zero-draw paths against the handle's
own ``gp_predict`` / ``gp_predict_grad``, and the interpolation identity at the training inputs.

Run on the GPU box:  python tools/paths_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "paths_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_paths.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["posterior paths: figures printed by tests/test_gpu_paths.py (largest error over the allowance named; 1 = at it)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("paths "):
            keep.append(line[6:])
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    if run.returncode:
        print(run.stdout[-6000:])
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
