"""Knowledge gradient: what a call costs -> profiles/kg_timing.txt.

D = 8, Matern-5/2, fixed hyper-parameters, the inverse factor built (option rows_build = 1), ONE handle per N and ONE process.
  table   N = 16384, 10^4 resident candidates: gp_kg_acq at A = 64 and 256 beside gp_es_acq at R = 64 (the same candidate solve
          and cross-covariance GEMM, another scoring kernel), timed alternately
  rows    N = 16384 and 512, M = 1 and 8 locations by value, A = 64 and 256: gp_kg_rows without and with dout beside
          gp_es_acq_rows (R = 64, values only: the same forward pass and one kernel behind it) and gp_acq_rows (EI) with gradient for
          the SAME locations (the same two passes over the inverse factor), timed alternately
  ratio   gp_kg_rows with dout / gp_acq_rows with gradient: what the mix and the closing pass add to two reads of L^-1
Wall time in ms of calls that end in the stream's synchronisation, median [quartiles] after warm-up.  Every figure is measured by
this tool on the machine it runs on; nothing is estimated.

Run on the GPU box:  python tools/kg_timing.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "kg_timing.txt")
D, R = 8, 64
TABLE_N, TABLE_M, TABLE_REPS, TABLE_WARM = 16384, 10000, 12, 2
ROWS_N, ROWS_M, AS, ROWS_REPS, ROWS_WARM = (16384, 512), (1, 8), (64, 256), 200, 10


def quartiles(t):
    q = np.percentile(t, [25, 50, 75])
    return q[1], "%.3f [%.3f, %.3f]" % (q[1], q[0], q[2])


def clocked(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternately(fns, reps, warm):
    for _ in range(warm):
        for f in fns:
            f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            t[i].append(clocked(f))
    return [quartiles(x) for x in t]


def handle(rng, N):
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    h = _lib.Handle(0)
    h.set_data(X, (Y - Y.mean()) / Y.std())
    h.set_params(_lib.GP_KERNEL_MATERN52, 0, 1.0, np.array([0.9]), 1e-2)
    h.fit()
    h.set_option("rows_build", 1)
    # a belief over R representers for the entropy-search entries beside: its numbers do not matter to the time
    h.es_set_representers(rng.uniform(0, 1, (R, D)))
    h.es_set_belief(np.full(R, -np.log(R)), np.zeros(R), 0.1 * np.eye(R), np.zeros((R, R, R)), np.linspace(-2, 2, 50))
    return h


def main():
    rng = np.random.default_rng(7)
    lines = ["knowledge gradient: wall time per call in ms, median [quartiles]; D = %d, Matern-5/2, noise 1e-2" % D, "",
             "table: N = %d, %d resident candidates, %d repetitions after %d, timed alternately" % (TABLE_N, TABLE_M, TABLE_REPS, TABLE_WARM)]
    h = handle(rng, TABLE_N)
    h.set_candidates(rng.uniform(0, 1, (TABLE_M, D)))
    for A in AS:
        h.kg.set_points(rng.uniform(0, 1, (A, D)))
        (mk, sk), (me, se) = alternately([lambda: h.kg.acq(), lambda: h.es_acq()], TABLE_REPS, TABLE_WARM)
        lines.append("A = %-3d  gp_kg_acq %s   gp_es_acq (R = %d) %s   ratio %.2f" % (A, sk, R, se, mk / me))
    lines += ["", "rows: %d repetitions after %d, timed alternately; ratio = gp_kg_rows with dout / gp_acq_rows (EI) with gradient"
              % (ROWS_REPS, ROWS_WARM)]
    for N in ROWS_N:
        if N != TABLE_N:      # (the table's handle serves the first size)
            h.close()
            h = handle(rng, N)
        fmin = h.fmin()
        for A in AS:
            h.kg.set_points(rng.uniform(0, 1, (A, D)))
            for M in ROWS_M:
                x = rng.uniform(0, 1, (M, D))
                res = alternately([lambda: h.kg.rows(x), lambda: h.kg.rows(x, grad=True), lambda: h.es_acq_rows(x),
                                   lambda: h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)], ROWS_REPS, ROWS_WARM)
                (_, sv), (mg, sg), (_, se), (ma, sa) = res
                lines.append("N = %-5d A = %-3d M = %d  kg value %s   kg grad %s   es_acq_rows %s   acq_rows grad %s   ratio %.2f"
                             % (N, A, M, sv, sg, se, sa, mg / ma))
    h.close()
    lines.append("")
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
