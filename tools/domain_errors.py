"""Inputs off the unit cube: what the GPU tests measure, kept as a record -> profiles/domain_errors.txt.

Runs tests/test_gpu_domains.py and keeps what its comparisons print before they assert: per family and exponent set how many
results the power-of-two scaling moved (none may), and per result of the shifted problem Delta (what rounding x / l once moves the
long-double truth by), the entry's existing tolerance, the device's error and its ratio to the allowance existing + 2 Delta
(1 = at the allowance); for the residue-path case the launches of the residue GEMM.  The case table of tests/_domain_cases.py goes
in front.

Run on the GPU box:  python tools/domain_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "domain_errors.txt")


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import _domain_cases as DC
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_domains.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["inputs off the unit cube: figures printed by tests/test_gpu_domains.py", "",
            "the case table (tests/_domain_cases.py)", ""] + DC.table() + [""]
    for line in run.stdout.splitlines():
        if line.startswith("_") and " test_" in line:
            keep.append(line.strip("_ "))
        elif "results moved" in line or "error / (existing" in line or ", offsets [" in line or "residue GEMM launches" in line:
            keep.append("    " + line)
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep[-40:]))
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
