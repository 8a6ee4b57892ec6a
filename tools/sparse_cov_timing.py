"""Writes profiles/sparse_cov_timing.txt: what the sparse model's joint posterior costs at the handle level.  A record, not a pass
mark.  Protocol of profiles/sparse_acq_timing.txt: N = 16384, D = 8, RBF ARD, P = 1, wall-clock medians.
  * Mz in {128, 2048}, R = 50 resident points: the one-location gp_sparse_cov_between call beside the one-location
    gp_sparse_predict_rows value call at the same Mz (both one launch and a drain; 200 calls after 20), the 8-location call, and the
    1000-row block call (20 after 3); the first call after a fit, which builds G (5 fits).
  * gp_sparse_predict_full_cov and gp_sparse_posterior_samples (S = 10) at M = 1024 (5 after 1).
usage: sparse_cov_timing.py [out.txt]        (default: profiles/sparse_cov_timing.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path += [ROOT]
from gaussian_process_optimization_amd import _lib   # noqa: E402

N, D, R = 16384, 8, 50
MZS = (128, 2048)
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


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_cov_timing.txt")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    pts, loc = rng.uniform(0, 1, (R, D)), rng.uniform(0, 1, (1024, D))
    lines = ["The joint posterior of the sparse GP on one MI355X, handle level: tools/sparse_cov_timing.py.  A record, no pass mark.",
             "N = %d, D = %d, RBF ARD, P = 1, R = %d resident points; wall-clock medians, ms." % (N, D, R), ""]
    for mz in MZS:
        h = _lib.Handle(0)
        h.set_data(X, Y)
        h.set_params(_lib.GP_KERNEL_RBF, True, VAR, LS, NOISE)
        h.sparse_set_inducing(X[rng.permutation(N)[:mz]])
        h.sparse_fit()
        h.sparse_cov_set_points(pts)
        x1, x8, x1000 = (np.ascontiguousarray(loc[:k]) for k in (1, 8, 1000))
        one = median_ms(lambda: h.sparse_cov_between(x1), reps=200, warm=20)
        rows = median_ms(lambda: h.sparse_predict_rows(x1, include_noise=False), reps=200, warm=20)
        eight = median_ms(lambda: h.sparse_cov_between(x8), reps=200, warm=20)
        block = median_ms(lambda: h.sparse_cov_between(x1000))
        first = []
        for _ in range(5):      # the first call after a fit builds G
            h.sparse_fit()
            t0 = time.perf_counter()
            h.sparse_cov_between(x1)
            first.append(1e3 * (time.perf_counter() - t0))
        full = median_ms(lambda: h.sparse_predict_full_cov(loc, include_noise=False), reps=5, warm=1)
        Zn = rng.standard_normal((10, 1024))
        samp = median_ms(lambda: h.sparse_posterior_samples(loc, Zn, include_noise=True), reps=5, warm=1)
        h.close()
        npad = (mz + 127) // 128 * 128
        gbytes = 8.0 * R * npad
        lines += ["Mz = %4d   G is %d x %d: %.3f MB" % (mz, R, npad, gbytes / 1e6),
                  "            gp_sparse_cov_between, 1 location              %10.4f" % one,
                  "            gp_sparse_predict_rows value call, 1 location  %10.4f   (cov_between / rows: %.2f)" % (rows, one / rows),
                  "            gp_sparse_cov_between, 8 locations             %10.4f" % eight,
                  "            gp_sparse_cov_between, 1000 locations          %10.4f   (%.2f us per location)" % (block, 1e3 * block / 1000),
                  "            gp_sparse_cov_between, first call after a fit  %10.4f   (builds G)" % float(np.median(first)),
                  "            gp_sparse_predict_full_cov, M = 1024           %10.4f" % full,
                  "            gp_sparse_posterior_samples, M = 1024, S = 10  %10.4f" % samp, ""]
        if one > 2 * rows:
            lines += ["            The one-location call costs more than twice the rows call.  Both are one launch and a drain.  The rows call",
                      "            spreads Mz / 8 workgroups over the matrix; this one has R / 8 = %d workgroups, and each generates k(x, Z) for" % ((R + 7) // 8),
                      "            the whole of Z before its first product.  By the kernel's structure the time is in that serial head and not in",
                      "            the %.3f MB of G; the two parts were not timed apart." % (gbytes / 1e6), ""]
        print("\n".join(lines[-10:]), flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
