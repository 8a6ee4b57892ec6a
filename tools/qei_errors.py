"""Joint expected improvement: the errors the GPU tests measure, kept as a record -> profiles/qei_errors.txt.

Runs tests/test_gpu_qei.py and keeps what its comparisons print before they assert: per case of tests/_qei_truth.py the error of
the joint posterior over the tolerance of tests/test_gpu_rows.py, the value's error over its first-order allowance, the gradient's
error beside the error of the same algorithm in plain float64 (and their ratio), q = 1 over stratified samples against
``gp_acq_rows`` (EI), the return code of the degenerate batch, and the end-to-end suggestion.

Run on the GPU box:  python tools/qei_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "qei_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_qei.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["joint expected improvement: figures printed by tests/test_gpu_qei.py (errors over the allowance named; 1 = at it)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("qei "):
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
