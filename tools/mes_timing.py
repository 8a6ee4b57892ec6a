"""Max-value entropy search: what the rule and the sampler cost -> profiles/mes_timing.txt.

Wall time in ms after warm-up, median and quartiles; D = 8, Matern-5/2, fixed hyper-parameters:
  one row   gp_acq_rows at one location, value only and with gradient: EI beside MES with K = 10 and K = 64 samples on the SAME
            handle, N = 512 and 16384 (the inverse factor built: option rows_build = 1)
  table     gp_acq over M = 10^4 resident candidates with the posterior cached (the rule's own kernel): EI beside MES
  sampler   one full draw of y* (MinValueSampler.sample: the table made resident, its latent posterior, gp_mes_bracket and the
            rounds of gp_mes_logsurv) at M = 10^4 and 10^6 table rows, N = 512, beside the host sampler -- the same rounds over
            NumPy / SciPy sums in blocks of rows -- fed the same latent posterior (gp_predict's output, the copy to the host not timed)
Every figure is measured by this tool on the machine it runs on; nothing is estimated.  The before / after figures of the existing
kernels are a record of their own: tools/mes_before_after.py -> profiles/mes_before_after.txt.

Run on the GPU box:  python tools/mes_timing.py
"""
import os
import sys
import time

import numpy as np
from scipy.special import log_ndtr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_optimization_amd as gpo  # noqa: E402
from gaussian_process_optimization_amd import _lib, max_value  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mes_timing.txt")
D = 8
EI, MES = _lib.GP_ACQ_EI, _lib.GP_ACQ_MES


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


def handle(N, rng):
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    h = _lib.Handle(0)
    h.set_data(X, (Y - Y.mean()) / Y.std())
    h.set_params(_lib.GP_KERNEL_MATERN52, 0, 1.0, np.array([0.9]), 1e-2)
    h.fit()
    h.set_option("rows_build", 1)
    return h, X


class _Space(object):
    def __init__(self, M, rng):
        self.table = rng.uniform(0, 1, (M, D))

    def samples_uniform(self, n):
        return self.table[:n]


class _Posterior(object):
    """The host sampler's model: a posterior computed once (``predict`` answers with it)."""

    def __init__(self, mu, sd, fmin):
        self.mu, self.sd, self.fmin, self.model = mu, sd, fmin, None

    def predict(self, X):
        return self.mu, self.sd

    def get_fmin(self):
        return self.fmin


def main():
    rng = np.random.default_rng(7)
    lines = ["max-value entropy search: wall time in ms, median [quartiles]; D = 8, Matern-5/2", ""]
    for N in (512, 16384):
        h, X = handle(N, rng)
        fmin = h.fmin()
        x1 = rng.uniform(0, 1, (1, D))
        lines.append("N = %d" % N)
        for grad in (False, True):
            what = "with gradient" if grad else "value only   "
            lines.append("  one row  gp_acq_rows %s  EI            %s" % (what, spread(lambda: h.acq_rows(x1, EI, 0.01, fmin, grad=grad), 300, 10)))
            for K in (10, 64):
                h.mes_set(fmin - 0.05 * np.arange(1, K + 1))
                lines.append("  one row  gp_acq_rows %s  MES, K = %-3d   %s" % (what, K, spread(lambda: h.acq_rows(x1, MES, 0.0, 0.0, grad=grad), 300, 10)))
        Xs = rng.uniform(0, 1, (10000, D))
        h.set_candidates(Xs)
        h.predict(True)
        lines.append("  table    gp_acq, M = 10000, posterior cached   EI            %s" % spread(lambda: h.acq(EI, 0.01, fmin), 50))
        for K in (10, 64):
            h.mes_set(fmin - 0.05 * np.arange(1, K + 1))
            lines.append("  table    gp_acq, M = 10000, posterior cached   MES, K = %-3d   %s" % (K, spread(lambda: h.acq(MES, 0.0, 0.0), 50)))
        lines.append("")
        h.close()
    N = 512
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(D, variance=1.0, lengthscale=0.9), noise_var=1e-2, max_iters=0, verbose=False)
    gm.updateModel(X, (Y - Y.mean()) / Y.std(), None, None)
    lines.append("sampler: one full draw of y* (K = 10), N = %d" % N)
    for M in (10000, 1000000):
        space = _Space(M, rng)
        dev = max_value.MinValueSampler(gm, space, 10, M, seed=1)
        reps = 10 if M <= 10000 else 3
        lines.append("  M = %-8d device  (table upload, latent posterior, bracket, %s)   %s"
                     % (M, "rounds of gp_mes_logsurv", spread(dev.sample, reps, 1)))
        assert dev.last_on_device
        table = dev.table()
        h = gm.model._h
        h.set_candidates(table)
        mean, var = h.predict(False)
        sd = np.sqrt(np.maximum(var, 1e-10))
        host = max_value.MinValueSampler(_Posterior(mean, sd, gm.get_fmin()), space, 10, M, seed=1)
        lines.append("  M = %-8d host    (the same rounds over SciPy's log_ndtr, posterior given)            %s"
                     % (M, spread(lambda: host.sample(table), 3 if M <= 10000 else 1, 0 if M > 10000 else 1)))
        lines.append("  M = %-8d quartiles  device %s   host %s"
                     % (M, " / ".join("%.6f" % dev.last_quantiles[q] for q in max_value.QUANTILES),
                        " / ".join("%.6f" % host.last_quantiles[q] for q in max_value.QUANTILES)))
    lines.append("")
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
