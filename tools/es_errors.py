"""Entropy search: the errors the GPU tests measure, kept as a record -> profiles/es_errors.txt.

Runs tests/test_gpu_entropy_search.py and keeps what its comparisons print before they assert: the EP kernel against the
reference's recorded joint_min outputs (per fixture case: status counts, sweep counts, relative error of logP and of every
derivative), the representers' posterior against the oracle, table scores against the long-double statement, the fused rows
route against the table route, the class's device route against its host twin.

Run on the GPU box:  python tools/es_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "es_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_entropy_search.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["entropy search: figures printed by tests/test_gpu_entropy_search.py (relative to the largest reference magnitude unless "
            "said otherwise)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("_") and " test_" in line:
            keep.append(line.strip("_ "))
        elif line and not line.startswith(("=", "-", ".", "_")) and "Captured" not in line:
            keep.append("    " + line)
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
