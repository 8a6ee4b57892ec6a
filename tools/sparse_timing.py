"""The sparse GP's first timing record (a baseline for later work: nothing here was measured before, and no target is set).
At N = 16384, D = 8, RBF, P = 1: gp_sparse_fit_grad and gp_sparse_predict (10^4 candidates) for Mz in {10, 128, 512, 1024},
median of 20 calls after 3 warm-ups, with the phases of the last call; gp_fit_grad at the same N on the same build (what a user
pays today); the float64 oracle's VarDTC (tests/_sparse_ref.py) on the host's threads; and the new gradient kernel's covariance
evaluations per second beside gradx_tile_kernel's at a square size with the same pair count (N = 4096 against 16384 x 1024).
usage: sparse_timing.py [out.txt]        (default: profiles/sparse_gp_timing.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path += [ROOT, os.path.join(ROOT, "tests")]
from gaussian_process_optimization_amd import _lib   # noqa: E402

N, D, M = 16384, 8, 10000
MZS = (10, 128, 512, 1024)
VAR, NOISE = 1.3, 2e-2
LS = np.linspace(0.15, 0.35, D) * np.sqrt(D / 3.0)


def median_ms(call, reps=20, warm=3):
    for _ in range(warm):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def phases(h):
    return "  ".join("%s %.3f" % (p["name"], p["ms"]) for p in h.phases())


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_gp_timing.txt")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    Xs = rng.uniform(0, 1, (M, D))
    lines = ["Sparse GP (variational DTC) on one MI355X: the FIRST timing record, a baseline for later work (no target was set).",
             "N = %d, D = %d, RBF ARD, P = 1, %d candidates; wall-clock medians of 20 calls after 3 warm-ups, ms; phases: device time "
             "of the last call (HIP events)." % (N, D, M), ""]
    h = _lib.Handle(0)
    h.set_data(X, Y)
    h.set_params(_lib.GP_KERNEL_RBF, True, VAR, LS, NOISE)
    nm_ms = None
    for mz in MZS:
        Z = X[rng.permutation(N)[:mz]].copy()
        Z[mz // 2:] += 0.03 * rng.standard_normal((mz - mz // 2, D))
        h.sparse_set_inducing(Z)
        fg = median_ms(lambda: h.sparse_fit_grad(D))
        ph_fit = phases(h)
        if mz == 1024:
            nm_ms = [p["ms"] for p in h.phases() if p["name"] == "sparse_grad_nm"][0]
        pr = median_ms(lambda: h.sparse_predict(Xs, include_noise=True))
        prg = median_ms(lambda: h.sparse_predict(Xs, include_noise=True, grad=True))
        lines += ["Mz = %4d   gp_sparse_fit_grad %9.3f   gp_sparse_predict %9.3f   with gradients %9.3f" % (mz, fg, pr, prg),
                  "            phases: " + ph_fit]
        print(lines[-2], flush=True)
    exact = median_ms(lambda: h.fit_grad(D), reps=5, warm=1)
    lines += ["", "gp_fit_grad (the exact model) at N = %d on the same build: %.3f   (median of 5 after 1 warm-up)" % (N, exact)]
    print(lines[-1], flush=True)
    h.close()
    # the gradient kernel beside its square sibling at the same pair count
    n2 = 4096
    h2 = _lib.Handle(0)
    h2.set_data(X[:n2], Y[:n2])
    h2.set_params(_lib.GP_KERNEL_RBF, True, VAR, LS, NOISE)
    for _ in range(3):
        h2.fit_grad_x(D)
    gx_ms = [p["ms"] for p in h2.phases() if p["name"] == "lml_grad_x"]
    h2.close()
    if nm_ms and gx_ms:
        lines += ["", "covariance evaluations per second (D = 8: one pass each):",
                  "  sparse_grad_tile_kernel + sums, N x Mz = %d x 1024 (%.1f M pairs): %.3f ms -> %.2f G pairs/s"
                  % (N, N * 1024 / 1e6, nm_ms, N * 1024 / nm_ms / 1e6),
                  "  gradx_tile_kernel + sum,         N x N  = %d x %d (%.1f M pairs): %.3f ms -> %.2f G pairs/s"
                  % (n2, n2, n2 * n2 / 1e6, gx_ms[0], n2 * n2 / gx_ms[0] / 1e6)]
    # the float64 oracle on the host
    import _sparse_ref as R
    from oracle import cpu_ref as O
    keep = O.limit_blas_threads()   # (held: the limit lasts as long as the object)
    lines += ["", "float64 oracle (tests/_sparse_ref.py: LAPACK substitutions, NumPy products, direct-difference distances rounded to "
              "float64) on %d host threads, one call each, seconds:" % O.usable_cpus()]
    for mz in MZS:
        Z = X[rng.permutation(N)[:mz]].copy()
        t0 = time.perf_counter()
        R.inference("rbf", X, Z, Y, VAR, LS, True, NOISE, R.F64)
        lines.append("  Mz = %4d   inference with gradients %.2f" % (mz, time.perf_counter() - t0))
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
