"""Entropy search: wall time of the device route against the host route of the same class -> profiles/es_timing.txt.

For N in {500, 4000, 16384} (D = 4, Matern-5/2, noise 1e-2, fixed hyper-parameters) and R = 50 representers, S = 100 quantiles:
  prepare      representers' posterior and EP sweeps (medians of three after a first call), closing algebra (device route), and
               the same steps of the host route (predict + predict_covariance, NumPy sweeps; the closing algebra is shared)
  one location one acquisition_function call of a single row (the optimiser's call), median of 20
  tables       1000 and 10^4 rows; the host route scores candidate by candidate, so it is timed on the first 40 rows of each table
               and scaled to the table (said so in the record)

Run on the GPU box:  python tools/es_timing.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_optimization_amd as gpo  # noqa: E402
from gaussian_process_optimization_amd import entropy_search as E  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "es_timing.txt")
D, R, S, HOST_ROWS = 4, 50, 100, 40


class FixedSampler(E.McmcSampler):
    def __init__(self, space, pts):
        super().__init__(space)
        self.pts = pts

    def get_samples(self, n, log_p, burn_in_steps=50):
        return self.pts, np.asarray(log_p(self.pts), dtype=float).reshape(-1, 1)


def ms(fn, reps=1):
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(best)), out


def main():
    lines = ["entropy search, device route against the host route of the same class (wall ms; D = %d, R = %d, S = %d)" % (D, R, S), ""]
    space = gpo.Design_space([{"name": "x", "type": "continuous", "domain": (0.0, 1.0), "dimensionality": D}])
    for N in (500, 4000, 16384):
        rng = np.random.default_rng(N)
        X = rng.uniform(0, 1, (N, D))
        Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
        gm = gpo.GPModel(kernel=gpo.kern.Matern52(D, variance=1.0, lengthscale=0.5), noise_var=1e-2, max_iters=0, verbose=False)
        gm.updateModel(X, Y, None, None)
        gp = gm.model
        gp._ensure_fit()
        h = gp._h
        pts = rng.uniform(0, 1, (R, D))
        # -- prepare, step by step
        h.es_set_representers(pts)                                          # first use: allocations
        t_rep, (mu, cov) = ms(lambda: h.es_set_representers(pts), 3)
        cov = np.maximum(cov, 1e-10)
        t_ep, sites = ms(lambda: h.es_pmin(mu, cov), 3)
        t_close, belief = ms(lambda: E.joint_min(mu, cov, sites))
        t_hrep, _ = ms(lambda: (gm.predict(pts), gm.predict_covariance(pts)))
        t_hep, hsites = ms(lambda: E.ep_sweeps(mu, cov))
        lines.append("N = %5d  prepare: representers %.2f (host route %.2f)  EP sweeps %.2f (NumPy %.1f)  closing algebra %.1f  "
                     "[chains ended early: %d, sweeps %d..%d]" % (N, t_rep, t_hrep, t_ep, t_hep, t_close, int(np.sum(sites[3] == -1)),
                                                                    sites[4].min(), sites[4].max()))
        dev = gpo.AcquisitionEntropySearch(gm, space, FixedSampler(space, pts), num_samples=S, num_representer_points=R)
        host = gpo.AcquisitionEntropySearch(gm, space, FixedSampler(space, pts), num_samples=S, num_representer_points=R, device=False)
        x1 = rng.uniform(0, 1, (1, D))
        dev.acquisition_function(x1), host.acquisition_function(x1)        # beliefs in place, inverse factor built where the rule says so
        for _ in range(int(gp._h.N // 768) + 2):                            # past the build rule of the inverse factor (N > 4096)
            dev.acquisition_function(x1)
        t1, a = ms(lambda: dev.acquisition_function(x1), 20)
        t1h, b = ms(lambda: host.acquisition_function(x1), 5)
        lines.append("           one location: device %.3f  host %.2f  (x%.0f)   |difference| %.1e" % (t1, t1h, t1h / t1, abs(a - b).max()))
        for M in (1000, 10000):
            Xs = rng.uniform(0, 1, (M, D))
            tM, a = ms(lambda: dev.acquisition_function(Xs), 3)
            th, b = ms(lambda: host.acquisition_function(Xs[:HOST_ROWS]))
            th *= M / HOST_ROWS
            note = "device faster x%.0f" % (th / tM) if th > tM else "DEVICE SLOWER x%.2f" % (tM / th)
            lines.append("           table of %5d: device %.2f  host %.0f (scaled from %d rows)  %s   |difference| %.1e"
                         % (M, tM, th, HOST_ROWS, note, abs(a[:HOST_ROWS] - b).max()))
        lines.append("")
    open(OUT, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
