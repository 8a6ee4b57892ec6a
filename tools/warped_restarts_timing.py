"""Writes profiles/warped_restarts_timing.txt: the hyper-parameter restarts of the two warped models in lockstep against the
serial loop, on one MI355X.

For ``InputWarpedGP`` (Matern-5/2 ARD, Kumaraswamy warp of every column) and ``WarpedGP`` (Matern-3/2 ARD, three tanh terms), at
N in {300, 1000, 2000}, D = 8: the wall time of ``optimize_restarts(5, max_iters=50)``, serial against ``parallel=True``, median
of REPS runs, the two alternating, every run on a fresh model from the same seed of ``np.random`` (so both draw the same
starting points), after one short run of each as warm-up.  The serial loop is the code path of the parent commit, which this
change leaves as it was: its figure stands for the parent on the same build.  Each call ends in the device synchronise of the
model's closing fit.

Then one line per entry and size: ONE batch call with R = 5 members against FIVE single calls (``gp_set_data`` +
``gp_fit_grad_x``; ``gp_fit_grad_warp``) on the same members, median of CALLS.

The condition, stated in the file: lockstep is not slower than serial at any of the three sizes, for either model.
usage: warped_restarts_timing.py [out.txt]        (default: profiles/warped_restarts_timing.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_optimization_amd as gpo  # noqa: E402
from gaussian_process_optimization_amd import _lib  # noqa: E402

D, R, MAX_ITERS, REPS, CALLS = 8, 5, 50, 3, 7
SIZES = (300, 1000, 2000)


def problem(N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.exp(np.sin(3 * (X ** 2).sum(1, keepdims=True) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, 1))
    return X, Y


def input_warped(X, Y):
    m = gpo.models.InputWarpedGP(X, Y, kernel=gpo.kern.Matern52(D, variance=1.0, ARD=True), Xmin=[0.0] * D, Xmax=[1.0] * D)
    m.Gaussian_noise.variance.set(1e-2)
    m.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
    return m


def warped(X, Y):
    m = gpo.models.WarpedGP(X, Y, kernel=gpo.kern.Matern32(D, variance=1.0, ARD=True), warping_terms=3)
    m.Gaussian_noise.variance.set(1e-2)
    m.Gaussian_noise.constrain_positive(warning=False)
    return m


def restarts(make, X, Y, parallel, max_iters):
    """(wall ms, best objective) of one search on a fresh model."""
    m = make(X, Y)
    try:
        np.random.seed(4321)
        m._h.synchronize()
        t0 = time.perf_counter()
        runs = m.optimize_restarts(R, verbose=False, max_iters=max_iters, parallel=parallel)
        m._h.synchronize()
        return 1e3 * (time.perf_counter() - t0), min(f for f, _ in runs)
    finally:
        m.close()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def entries(h, X, Y):
    """Medians (batch ms, five singles ms) of the x entry and of the warp entry on R members."""
    rng = np.random.default_rng(7)
    var, noise = 10.0 ** rng.uniform(-0.5, 0.5, R), 10.0 ** rng.uniform(-3, -1.5, R)
    ls = 0.5 * np.sqrt(D) * 10.0 ** rng.uniform(-0.2, 0.2, (R, D))
    Xw = np.stack([1.0 - (1.0 - X ** rng.uniform(0.5, 2.0, D)) ** rng.uniform(0.5, 2.0, D) for _ in range(R)])
    psi = np.stack([rng.uniform(0.3, 1.5, (R, 3)), rng.uniform(0.3, 2.0, (R, 3)), rng.uniform(-1, 1, (R, 3))], axis=2)
    d = rng.uniform(0.5, 1.2, R)
    h.set_data(X, Y)
    h.set_output_warp(None)
    h.set_params(_lib.GP_KERNEL_MATERN52, True, var[0], ls[0], noise[0])

    def x_singles():
        for r in range(R):
            h.set_data(Xw[r], Y)
            h.set_params(_lib.GP_KERNEL_MATERN52, True, var[r], ls[r], noise[r])
            h.fit_grad_x(D)

    def w_singles():
        for r in range(R):
            h.set_params(_lib.GP_KERNEL_MATERN52, True, var[r], ls[r], noise[r])
            h.fit_grad_warp(psi[r], d[r], D)

    out = []
    for batch, singles, reset in ((lambda: h.fit_grad_x_batch(Xw, var, ls, noise), x_singles, lambda: h.set_data(X, Y)),
                                  (lambda: h.fit_grad_warp_batch(psi, d, var, ls, noise), w_singles, lambda: None)):
        reset()
        batch()
        singles()
        rec = np.empty((CALLS, 2))
        for c in range(CALLS):
            reset()
            rec[c, 0] = timed(batch)
            rec[c, 1] = timed(singles)
        out.append(np.median(rec, axis=0))
    h.set_output_warp(None)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "warped_restarts_timing.txt")
    lines = ["Restarts of the warped models in lockstep against the serial loop (tools/warped_restarts_timing.py): D = %d, %d restarts,"
             % (D, R), "max_iters = %d, wall ms, median of %d alternating runs (min .. max); the serial loop is the parent's code path."
             % (MAX_ITERS, REPS), "", "%-14s %5s | %22s | %22s | %6s | %s" % ("model", "N", "serial", "lockstep", "ratio", "best objective serial / lockstep")]
    worst = np.inf
    for name, make in (("InputWarpedGP", input_warped), ("WarpedGP", warped)):
        for N in SIZES:
            X, Y = problem(N, seed=N)
            for par in (False, True):
                restarts(make, X, Y, par, 3)          # warm-up: every launch shape, the batch buffers
            rec = {False: [], True: []}
            best = {}
            for _ in range(REPS):
                for par in (False, True):
                    ms, best[par] = restarts(make, X, Y, par, MAX_ITERS)
                    rec[par].append(ms)
            s, p = np.array(rec[False]), np.array(rec[True])
            ratio = float(np.median(s) / np.median(p))
            worst = min(worst, ratio)
            lines.append("%-14s %5d | %8.1f (%6.1f .. %6.1f) | %8.1f (%6.1f .. %6.1f) | %5.2fx | %.9g / %.9g" % (
                name, N, np.median(s), s.min(), s.max(), np.median(p), p.min(), p.max(), ratio, best[False], best[True]))
            print(lines[-1], flush=True)
    lines += ["", "ONE batch call with R = %d members against FIVE single calls on the same members, wall ms, median of %d:" % (R, CALLS),
              "%5s | %-22s %9s %9s %6s | %-22s %9s %9s %6s" % ("N", "entry", "batch", "singles", "ratio", "entry", "batch", "singles", "ratio")]
    h = _lib.Handle(0)
    for N in SIZES:
        X, Y = problem(N, seed=N)
        (xb, xs), (wb, ws) = entries(h, X, Y)
        lines.append("%5d | %-22s %9.3f %9.3f %5.2fx | %-22s %9.3f %9.3f %5.2fx" % (
            N, "gp_fit_grad_x_batch", xb, xs, xs / xb, "gp_fit_grad_warp_batch", wb, ws, ws / wb))
        print(lines[-1], flush=True)
    h.close()
    lines += ["", "ratio = serial / lockstep; the smallest over the six rows: %.2fx -- the condition (lockstep not slower than serial at any" % worst,
              "of the three sizes) %s." % ("HOLDS" if worst >= 1.0 else "FAILS")]
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))
    return 0 if worst >= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
