"""GP classification (Laplace): the errors the GPU tests measure, kept as a record -> profiles/laplace_errors.txt.

Runs tests/test_gpu_laplace.py and keeps what its comparisons print before they assert: per case of tests/_laplace_truth.py the
errors of log Z, log|B|, alpha and f, the Newton steps and the range of W; the gradient's worst entry; the latent posterior through
gp_predict, gp_predict_grad and gp_predict_rows and the class probability over their tolerances; the binary constraint's fold over
its bound; the codes of the refused entries.

Run on the GPU box:  python tools/laplace_errors.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "laplace_errors.txt")


def main():
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_laplace.py"), "-m", "gpu", "-q", "-rP",
                          "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    keep = ["GP classification, Laplace probit fit: figures printed by tests/test_gpu_laplace.py against the long-double truth "
            "(tests/_laplace_truth.py)", ""]
    for line in run.stdout.splitlines():
        if line.startswith("LAPLACE "):
            keep.append(line[8:])
    keep.append("")
    keep.append(run.stdout.strip().splitlines()[-1])
    open(OUT, "w").write("\n".join(keep) + "\n")
    print("\n".join(keep))
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
