"""Expected hypervolume improvement: what the fold costs, beside the probability of feasibility -> profiles/ehvi_timing.txt.

Per size N (512, 4000 and the bench size 16384; D = 8, Matern-5/2, fixed hyper-parameters; K = 2 and 3 objective models of N
points each), median and quartiles after warm-up, at fronts of 10 and of 100 points drawn on a plane (K = 2: 11 and 101 cells;
K = 3: what the slabs of that draw make, about 50 and 1300 to 1550):
  table     gp_ehvi_table over M = 10^4 resident candidates, beside gp_feas_table with K - 1 constraints on the same handles: the
            same K - 1 candidate solves over the other handles' tables (the scored handle's own posterior is cached on either
            side after the first call), so the difference is the fold -- one workgroup per row against one thread per row
  one row   gp_ehvi_rows with a gradient, beside gp_acq_rows_feas with K - 1 constraints: the same K fused passes and one drain,
            so again the difference is the fold
No speed is promised; the figures are the record.

Run on the GPU box:  python tools/ehvi_timing.py [N ...]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402
from gaussian_process_optimization_amd import multi_objective as MO  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ehvi_timing.txt")
D, M = 8, 10000
EI = _lib.GP_ACQ_EI


def spread(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(t, [25, 50, 75])
    return "%.3f [%.3f, %.3f]" % (q[1], q[0], q[2])


def handle(N, rng, shift):
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True) + shift) + 0.1 * rng.standard_normal((N, 1))
    h = _lib.Handle(0)
    h.set_data(X, (Y - Y.mean()) / Y.std())
    h.set_params(_lib.GP_KERNEL_MATERN52, 0, 1.0, np.array([0.9]), 1e-2)
    h.fit()
    h.set_option("rows_build", 1)
    return h


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [512, 4000, 16384]
    rng = np.random.default_rng(0)
    lines = ["expected hypervolume improvement: wall time in ms, median [quartiles]; D = %d, M = %d table rows" % (D, M), ""]
    Xs = rng.uniform(0, 1, (M, D))
    x1 = Xs[:1]
    for N in sizes:
        hs = [handle(N, rng, float(k)) for k in range(3)]
        h = hs[0]
        h.set_candidates(Xs)
        fmin = h.fmin()
        reps = 20 if N <= 4000 else 6
        lines.append("N = %d" % N)
        for K in (2, 3):
            feas = _lib.FeasPack(hs[1:K], np.zeros(K - 1), np.zeros(K - 1), np.ones(K - 1))
            lines.append("  table    gp_feas_table, %d constraint(s)                    %s" % (K - 1, spread(lambda: h.feas_table(feas), reps)))
            row_feas = spread(lambda: h.acq_rows_feas(feas, x1, EI, 0.01, fmin, grad=True), 200, 5)
            for n in (10, 100):
                front = rng.dirichlet(np.ones(K), n) - 0.5          # points of a plane: none dominates another
                levels, lo, hi = MO.nondominated_cells(front, np.full(K, 1.0))
                pack = _lib.EhviPack(hs[:K], np.zeros(K), np.ones(K))
                pack.set_cells(levels, lo, hi)
                h.set_candidates(Xs)
                lines.append("  table    gp_ehvi_table, K = %d, front of %3d (%4d cells)   %s"
                             % (K, n, lo.shape[0], spread(lambda: pack.table(), reps)))
                lines.append("  one row  gp_ehvi_rows with gradient, K = %d, front of %3d  %s"
                             % (K, n, spread(lambda: pack.rows(x1, grad=True), 200, 5)))
            lines.append("  one row  gp_acq_rows_feas with gradient, %d constraint(s)  %s" % (K - 1, row_feas))
        for o in hs:
            o.close()
        lines.append("")
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
