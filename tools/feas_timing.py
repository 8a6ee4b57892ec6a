"""Black-box constraints: what the probability of feasibility costs, against the unflagged call -> profiles/feas_timing.txt.

Per size N (512, 4000 and the bench size 16384; D = 8, Matern-5/2, fixed hyper-parameters; K = 1 and 3 constraint models of N
points each), median and quartiles after warm-up:
  table     gp_acq_argbest over M = 10^4 resident candidates, posterior cached: unflagged; gp_feas_table (one candidate solve per
            constraint: N^2 M flops, the launches of the objective's own posterior); flagged with the cache resident
  one row   the gradient call L-BFGS makes: gp_acq_rows unflagged against gp_acq_rows_feas (one more fused pass per constraint and
            the fold, one drain), the incumbent given
  classes   the same call through AcquisitionEI.acquisition_function_withGradients without and with feasibility=: what the
            acquisition optimiser pays per location, the Python layer included (the feasible incumbent is cached per fit and
            generation, so it is not in the steady-state figure; `first call` is the one that computes it through gp_fmin_rows)
Both sides are measured on THIS tree: the unflagged calls launch the kernels they launched before the feature (score_rows and
check_acq gained host-side branches only).

Run on the GPU box:  python tools/feas_timing.py [N ...]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_optimization_amd as gpo  # noqa: E402
from gaussian_process_optimization_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "feas_timing.txt")
D, M = 8, 10000
EI, FEAS = _lib.GP_ACQ_EI, _lib.GP_ACQ_TIMES_FEAS


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
    return h


def classes(N, rng, lines):
    """The one-location gradient call through the acquisition classes."""
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(D, variance=1.0, lengthscale=0.9), noise_var=1e-2, max_iters=0, verbose=False)
    gm.updateModel(X, (Y - Y.mean()) / Y.std(), None, None)
    gm.model._ensure_fit()
    gm.model._h.set_option("rows_build", 1)
    x1 = rng.uniform(0, 1, (1, D))
    plain = gpo.AcquisitionEI(gm, jitter=0.01)
    lines.append("  classes  AcquisitionEI with gradient, no feasibility      %s" % spread(lambda: plain.acquisition_function_withGradients(x1), 200, 5))
    for K in (1, 3):
        fm = gpo.FeasibilityModel(K, 0.0, noise_var=1e-2, max_iters=0, verbose=False)
        fm.update(X, np.stack([np.sin(2 * X.sum(1) + k) for k in range(K)], axis=1))
        for m in fm.models:
            m.model._ensure_fit()
            m.model._h.set_option("rows_build", 1)
        acq = gpo.AcquisitionEI(gm, jitter=0.01, feasibility=fm)
        t0 = time.perf_counter()
        acq.acquisition_function_withGradients(x1)
        first = (time.perf_counter() - t0) * 1e3
        lines.append("  classes  AcquisitionEI with gradient, feasibility K = %d  %s   (first call %.3f)"
                     % (K, spread(lambda: acq.acquisition_function_withGradients(x1), 200, 5), first))


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [512, 4000, 16384]
    rng = np.random.default_rng(0)
    lines = ["probability of feasibility: wall time in ms, median [quartiles]; D = %d, M = %d table rows" % (D, M), ""]
    Xs = rng.uniform(0, 1, (M, D))
    for N in sizes:
        h = handle(N, rng, 0.0)
        h.set_option("rows_build", 1)
        cons = [handle(N, rng, 1.0 + k) for k in range(3)]
        for c in cons:
            c.set_option("rows_build", 1)
        h.set_candidates(Xs)
        fmin = h.fmin()
        h.acq(EI, 0.01, fmin)
        reps = 20 if N <= 4000 else 6
        lines.append("N = %d" % N)
        lines.append("  table  unflagged gp_acq_argbest                     %s" % spread(lambda: h.acq_argbest(EI, 0.01, fmin, -1), reps))
        x1 = Xs[:1]
        row_plain = spread(lambda: h.acq_rows(x1, EI, 0.01, fmin, grad=True), 200, 5)
        for K in (1, 3):
            pack = _lib.FeasPack(cons[:K], np.zeros(K), np.zeros(K), np.ones(K))
            lines.append("  table  gp_feas_table, K = %d                          %s" % (K, spread(lambda: h.feas_table(pack), reps)))
            lines.append("  table  flagged gp_acq_argbest, K = %d (cache resident) %s" % (K, spread(lambda: h.acq_argbest(EI | FEAS, 0.01, fmin, -1), reps)))
        lines.append("  one row  gp_acq_rows with gradient, unflagged        %s" % row_plain)
        for K in (1, 3):
            pack = _lib.FeasPack(cons[:K], np.zeros(K), np.zeros(K), np.ones(K))
            lines.append("  one row  gp_acq_rows_feas with gradient, K = %d       %s" % (K, spread(lambda: h.acq_rows_feas(pack, x1, EI, 0.01, fmin, grad=True), 200, 5)))
        for o in [h] + cons:
            o.close()
        classes(N, rng, lines)
        lines.append("")
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
