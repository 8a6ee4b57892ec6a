"""Knowledge gradient: the errors the GPU tests measure, kept as a record -> profiles/kg_errors.txt.

Runs tests/test_gpu_kg.py and tests/test_gpu_kg_domains.py and keeps what their comparisons print before they assert: per case
of tests/_kg_truth.py the error of the discretisation points' means over the tolerance of tests/test_gpu_rows.py, the worst error of the table's and of the rows entry's
values over their first-order allowances, rows against table, the gradient's error beside the error of the same algorithm in plain
float64 (and their ratio), A = 1 against the two-line closed form, the end-to-end suggestion; and off the unit cube (cases b and f of
tests/_kg_domain.py) whether power-of-two scales kept every bit, and per result the device's error on the shifted arrays over the
existing tolerance plus 2 Delta.

Run on the GPU box:  python tools/kg_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "kg_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_kg.py"),
                          os.path.join("tests", "test_gpu_kg_domains.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["knowledge gradient: figures printed by tests/test_gpu_kg.py and tests/test_gpu_kg_domains.py (errors over the allowance "
            "named; 1 = at it)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("kg "):
            keep.append(line[3:])
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    if run.returncode:
        print(run.stdout[-6000:])
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
