"""Max-value entropy search: the errors the GPU tests measure, kept as a record -> profiles/mes_errors.txt.

Runs tests/test_gpu_mes.py and keeps what its comparisons print before they assert: per case of tests/_mes_truth.py and per
placement of g the largest error of ``gp_acq`` / ``gp_acq_grad`` with ``GP_ACQ_MES`` over the derived rounding bound (rule
arithmetic) and over the propagated posterior tolerance (against the oracle); the fused rows passes against the table; the
penalised and per-cost scores against their documented maps of the base scores; ``gp_mes_logsurv`` over its bound; the sampler's
brackets against the truth's quantiles; the classes against the host rule over the oracle.

Run on the GPU box:  python tools/mes_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "mes_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_mes.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["max-value entropy search: figures printed by tests/test_gpu_mes.py (largest error over the bound or tolerance named; "
            "1 = at it)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("MES "):
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
