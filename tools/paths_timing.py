"""Posterior paths: what the entries cost -> profiles/paths_timing.txt.

Wall time in ms after warm-up, median and quartiles; N = 16384, D = 8, Matern-5/2, fixed hyper-parameters:
  set       gp_paths_set for S = 16 paths of F = 1024 features (upload of the draws, Phi(X) W, the two substitutions for V)
  table     gp_paths_table over M = 10^4 and M = 2048 resident candidates (the copy of the [S, M] result included)
  samples   gp_posterior_samples -- what ``posterior_samples_f`` runs: the M x M posterior covariance built and factored -- for the
            same S = 16 draws at M = 2048, beside the table above
  argbest   gp_paths_argbest at M = 10^4
  rows      gp_paths_rows with gradient for 1 and 8 locations, beside the existing one-location gradient call gp_acq_rows (EI, the
            inverse factor built: option rows_build = 1) for 1 and 8 locations on the SAME handle
Every figure is measured by this tool on the machine it runs on; nothing is estimated.

Run on the GPU box:  python tools/paths_timing.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402
from gaussian_process_optimization_amd import posterior_paths as PP  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "paths_timing.txt")
N, D, S, F = 16384, 8, 16, 1024


def spread(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(t, [25, 50, 75])
    return "%.3f [%.3f, %.3f]" % (q[1], q[0], q[2])


def main():
    rng = np.random.default_rng(7)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    h = _lib.Handle(0)
    h.set_data(X, (Y - Y.mean()) / Y.std())
    h.set_params(_lib.GP_KERNEL_MATERN52, 0, 1.0, np.array([0.9]), 1e-2)
    h.fit()
    h.set_option("rows_build", 1)
    draws = PP.draw(_lib.GP_KERNEL_MATERN52, N, D, S, F, seed=1)
    lines = ["posterior paths: wall time in ms, median [quartiles]; N = %d, D = %d, Matern-5/2, S = %d, F = %d" % (N, D, S, F), ""]
    lines.append("set      gp_paths_set                                   %s" % spread(lambda: h.paths_set(*draws), 10, 2))
    for M in (10000, 2048):
        Xs = rng.uniform(0, 1, (M, D))
        h.set_candidates(Xs)
        lines.append("table    gp_paths_table, M = %-5d                        %s" % (M, spread(h.paths_table, 20)))
        if M == 10000:
            lines.append("argbest  gp_paths_argbest, M = %-5d                      %s" % (M, spread(h.paths_argbest, 20)))
        else:
            Z = rng.standard_normal((S, M))
            lines.append("samples  gp_posterior_samples, M = %-5d (S = %d draws)   %s"
                         % (M, S, spread(lambda: h.posterior_samples(Z, include_noise=False), 5, 1)))
            h.paths_set(*draws)      # the state every other timing starts from
    fmin = h.fmin()
    for M in (1, 8):
        x = rng.uniform(0, 1, (M, D))
        path = np.arange(M) % S
        lines.append("rows     gp_paths_rows with gradient, %d location(s)       %s" % (M, spread(lambda: h.paths_rows(x, path, grad=True), 300, 10)))
        lines.append("rows     gp_paths_rows value only, %d location(s)          %s" % (M, spread(lambda: h.paths_rows(x, path), 300, 10)))
        lines.append("rows     gp_acq_rows (EI) with gradient, %d location(s)    %s"
                     % (M, spread(lambda: h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True), 300, 10)))
    lines.append("")
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
