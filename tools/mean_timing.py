"""Mean function: what the one-location gradient call costs, with and without one -> a section of profiles/mean_timing.txt.

Per N = 512, 2048, 16384 (D = 8, Matern-5/2, fixed hyper-parameters), after the inverse factor is built: the wall time of
gp_acq_rows (EI, value and gradient, one location) and of gp_predict_rows (posterior and gradients), median and quartiles of 200
calls -- with no mean resident (the instances every model ran before) and, where the library has gp_mean_set, with an affine mean
(the mean-bearing instances of the finishing kernel: D + 1 more multiply-adds in its last workgroup).

The script measures the tree it lies in and prints one section; it does not know what else is in the file.  The record is put
together from one run of this branch and two runs of the parent commit built in the same session (a copy of this script placed in
the parent's tree: it has no gp_mean_set there and measures the no-mean rows alone), the spread of the parent's two runs stated
beside them.

Run on the GPU box:  python tools/mean_timing.py LABEL [out.txt]     (appends; default: stdout only)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402

D = 8
SIZES = (512, 2048, 16384)


def spread(fn, reps=200, warm=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(t, [25, 50, 75])
    return "%.4f [%.4f, %.4f]" % (q[1], q[0], q[2])


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "this tree"
    lines = ["%s: one location, value and gradient (wall ms, median [quartiles] of 200; D = %d, Matern-5/2)" % (label, D)]
    for N in SIZES:
        rng = np.random.default_rng(N)
        X = rng.uniform(0, 1, (N, D))
        Y = np.sin(3 * X.sum(1, keepdims=True)) + X @ rng.standard_normal((D, 1)) + 0.1 * rng.standard_normal((N, 1))
        h = _lib.Handle(0)
        h.set_data(X, Y)
        h.set_params(_lib.GP_KERNEL_MATERN52, 0, 1.0, np.array([0.9]), 1e-2)
        h.set_option("rows_build", 1)
        x1 = rng.uniform(0, 1, (1, D))
        for mean in (False, True):
            if mean and not hasattr(h, "mean_set"):
                continue
            if mean:
                h.mean_set(rng.standard_normal((D, 1)), np.array([0.3]))
            h.fit()
            fmin = h.fmin()
            h.acq_rows(x1, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)          # builds the inverse factor
            before = h.rows_stats()
            t_acq = spread(lambda: h.acq_rows(x1, _lib.GP_ACQ_EI, 0.01, fmin, grad=True))
            t_post = spread(lambda: h.predict_rows(x1, True, grad=True))
            assert h.rows_stats()["fallback"] == before["fallback"]
            lines.append("    N = %5d  %-9s gp_acq_rows %s   gp_predict_rows %s" % (N, "mean" if mean else "no mean", t_acq, t_post))
        h.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
