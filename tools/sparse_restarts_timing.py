"""Writes profiles/sparse_restarts_timing.txt: the sparse GP's hyper-parameter restarts in lockstep against the serial loop, on one
MI355X.  The workload is that of tools/sparse_timing.py: N = 16384, D = 8, RBF ARD, P = 1, Z a subset of X with its second half
moved by 0.03 N(0, 1).

1. ONE ``gp_sparse_fit_grad_batch`` over R members against R single ``gp_sparse_fit_grad`` calls, Mz in {10, 128, 512, 1024} and
   the cap 2048, R in {1, 2, 5, 10}: wall ms, median of CALLS calls after WARM warm-ups.  The members differ (variance, lengthscales, noise and Z
   perturbed per member).  Two baselines, both the parent commit's code path, which this change leaves as it was:
   "fit_grad"  R x the median of ``gp_sparse_fit_grad`` alone on one resident member -- the stricter one, and the one the condition
               below is held to;
   "pushed"    the loop a serial L-BFGS evaluation really runs per member: ``gp_set_params`` + ``gp_sparse_set_inducing`` +
               ``gp_sparse_fit_grad``.
2. The wall time of ``SparseGPRegression.optimize_restarts(5, max_iters=100)``, serial against ``parallel=True``, one run each on
   a fresh model from one seed of ``np.random`` after a two-iteration warm-up of each.

The condition, stated in the file: the lockstep route may be offered only where the R = 5 batch call is faster than five single
calls; an Mz at which it is not is listed, and ``SparseGPRegression._lockstep_applies`` must exclude it.
usage: sparse_restarts_timing.py [out.txt] [all|calls|restarts]        (default: profiles/sparse_restarts_timing.txt, all)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_optimization_amd as gpo  # noqa: E402
from gaussian_process_optimization_amd import _lib  # noqa: E402

N, D = 16384, 8
MZS = (10, 128, 512, 1024)
MZS_CALLS = MZS + (2048,)     # the cap as well: _lockstep_applies offers the route up to it
RS = (1, 2, 5, 10)
CALLS, WARM = 20, 3
RESTARTS, MAX_ITERS = 5, 100
VAR, NOISE = 1.3, 2e-2
LS = np.linspace(0.15, 0.35, D) * np.sqrt(D / 3.0)


def median_ms(call, reps=CALLS, warm=WARM):
    for _ in range(warm):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def problem():
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    return rng, X, Y


def inducing(rng, X, mz):
    Z = X[rng.permutation(N)[:mz]].copy()
    Z[mz // 2:] += 0.03 * rng.standard_normal((mz - mz // 2, D))
    return Z


def members(rng, Z, R):
    var = VAR * 10.0 ** rng.uniform(-0.2, 0.2, R)
    noise = NOISE * 10.0 ** rng.uniform(-0.3, 0.3, R)
    ls = LS[None, :] * 10.0 ** rng.uniform(-0.1, 0.0, (R, D))
    Zs = np.stack([Z + 0.01 * rng.standard_normal(Z.shape) for _ in range(R)])
    return Zs, var, ls, noise


def calls_table(lines):
    rng, X, Y = problem()
    h = _lib.Handle(0)
    h.set_data(X, Y)
    h.set_params(_lib.GP_KERNEL_RBF, True, VAR, LS, NOISE)
    excluded = []
    lines += ["ONE gp_sparse_fit_grad_batch over R members against R single calls: wall ms, median of %d calls after %d warm-ups."
              % (CALLS, WARM), "%5s %3s | %9s | %12s %6s | %12s %6s | %s" % ("Mz", "R", "batch", "R x fit_grad", "ratio", "R x pushed", "ratio",
                                                                           "steps of the ladders (members)")]
    for mz in MZS_CALLS:
        Z = inducing(rng, X, mz)
        for R in RS:
            Zs, var, ls, noise = members(rng, Z, R)
            out = h.sparse_fit_grad_batch(Zs, var, ls, noise)
            stepped = int(np.sum((out[0][1] != 0) | (out[0][2] != 0) | (out[2] != 0)))
            batch = median_ms(lambda: h.sparse_fit_grad_batch(Zs, var, ls, noise))
            h.set_params(_lib.GP_KERNEL_RBF, True, var[0], ls[0], noise[0])
            h.sparse_set_inducing(Zs[0])
            alone = median_ms(lambda: h.sparse_fit_grad(D))

            def pushed():
                for r in range(R):
                    h.set_params(_lib.GP_KERNEL_RBF, True, var[r], ls[r], noise[r])
                    h.sparse_set_inducing(Zs[r])
                    h.sparse_fit_grad(D)

            push = median_ms(pushed)
            lines.append("%5d %3d | %9.3f | %12.3f %5.2fx | %12.3f %5.2fx | %d" % (mz, R, batch, R * alone, R * alone / batch, push,
                                                                                  push / batch, stepped))
            print(lines[-1], flush=True)
            if R == 5 and not batch < 5 * alone:
                excluded.append(mz)
    h.close()
    return excluded


def restarts(X, Y, mz, parallel, max_iters):
    np.random.seed(4321)
    m = gpo.models.SparseGPRegression(X, Y, kernel=gpo.kern.RBF(D, variance=VAR, lengthscale=LS, ARD=True), num_inducing=mz)
    m.likelihood.variance.set(NOISE)
    m.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
    try:
        m._ensure_fit()
        t0 = time.perf_counter()
        runs = m.optimize_restarts(RESTARTS, verbose=False, max_iters=max_iters, parallel=parallel)
        m._ensure_fit()
        return 1e3 * (time.perf_counter() - t0), min(f for f, _ in runs)
    finally:
        m.close()


def restarts_table(lines):
    _, X, Y = problem()
    lines += ["", "SparseGPRegression.optimize_restarts(%d, max_iters=%d), serial against parallel=True: wall ms of one run each, from one"
              % (RESTARTS, MAX_ITERS), "seed, after a two-iteration warm-up of each.",
              "%5s | %10s | %10s | %6s | %s" % ("Mz", "serial", "lockstep", "ratio", "best objective serial / lockstep")]
    for mz in MZS:
        for par in (False, True):
            restarts(X, Y, mz, par, 2)
        s, fs = restarts(X, Y, mz, False, MAX_ITERS)
        p, fp = restarts(X, Y, mz, True, MAX_ITERS)
        lines.append("%5d | %10.1f | %10.1f | %5.2fx | %.9g / %.9g" % (mz, s, p, s / p, fs, fp))
        print(lines[-1], flush=True)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_restarts_timing.txt")
    which = sys.argv[2] if len(sys.argv) > 2 else "all"
    lines = ["Restarts of the sparse GP in lockstep against the serial loop (tools/sparse_restarts_timing.py) on one MI355X:",
             "N = %d, D = %d, RBF ARD, P = 1.  The single call and the serial loop are the parent commit's code path, unchanged." % (N, D), ""]
    excluded = calls_table(lines) if which in ("all", "calls") else []
    if which in ("all", "restarts"):
        restarts_table(lines)
    lines += ["", "ratio = singles / batch, serial / lockstep.  The condition (the R = 5 batch call faster than five gp_sparse_fit_grad calls): "
              + ("HOLDS at every Mz." if not excluded else "FAILS at Mz = %s: _lockstep_applies must exclude it." % excluded)]
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(lines[-1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
