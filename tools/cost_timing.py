"""Cost-aware EI: wall time of the cost pass and of the flagged scoring calls -> profiles/cost_timing.txt.

Table (N = Nc = 16384, D = 8, Matern-5/2 model and cost GP, fixed hyper-parameters), M = 10^4 and 10^6 candidates resident:
  unflagged   gp_acq_argbest over the cached posterior: the scoring epilogue and the selector
  flagged     the same call with GP_ACQ_PER_COST right after gp_cost_set (the table's logc is computed: the cost pass) and again
              (the table's logc is cached)
  cost pass   first flagged call minus second flagged call, against its floor: 55 fp64 vector instructions per (candidate, surface
              point) pair in the loop the compiler made (D = 8, values only: 8 subtractions, 8 + 1 fma of the sums, the rest exp,
              sqrt and the Matern polynomial; one of them v_rsq_f64), at the fp64 vector rate of 78.6 TFLOP/s = 39.3e12
              instruction-lanes per second (half the 157.3 TFLOP/s FP32 vector peak; one instruction-lane = one FMA)
One location (N = Nc = 512 and 16384), the gradient call L-BFGS makes, median and quartiles of 200 after warm-up:
  handle      gp_acq_rows with and without the flag
  classes     AcquisitionEI.acquisition_function_withGradients on the device route, and on the host rule -- the same cost behind a
              plain function: model.predict_withGradients + cost_model.predict_withGradients + NumPy, the code the parent commit
              runs for a callable cost

Run on the GPU box:  python tools/cost_timing.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_optimization_amd as gpo  # noqa: E402
from gaussian_process_optimization_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "cost_timing.txt")
D = 8
EI, F = _lib.GP_ACQ_EI, _lib.GP_ACQ_PER_COST
OPS_PER_PAIR, LANE_RATE = 55, 39.3e12


def spread(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(t, [25, 50, 75])
    return q[1], "%.3f [%.3f, %.3f]" % (q[1], q[0], q[2])


def models(N, rng):
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(D, variance=1.0, lengthscale=0.9), noise_var=1e-2, max_iters=0, verbose=False)
    gm.updateModel(X, Y, None, None)
    cm = gpo.CostModel('evaluation_time')
    cm.cost_model = gpo.GPModel(kernel=gpo.kern.Matern52(D, variance=1.0, lengthscale=1.1), noise_var=1e-2, max_iters=0, verbose=False)
    Xc = rng.uniform(0, 1, (N, D))
    cm.update_cost_model(Xc, np.exp(0.3 * np.sin(2 * Xc.sum(1)) + 0.05 * rng.standard_normal(N)))
    return gm, cm


def main():
    lines = ["cost-aware EI (wall ms, median [quartiles]; D = %d, Matern-5/2 model and cost GP)" % D, ""]
    for N in (512, 16384):
        rng = np.random.default_rng(N)
        gm, cm = models(N, rng)
        dev = gpo.AcquisitionEI(gm, cost_withGradients=cm.cost_withGradients)
        host = gpo.AcquisitionEI(gm, cost_withGradients=lambda x: cm.cost_withGradients(x))
        assert dev._device_ok() and dev._per_cost and not host._device_ok()
        x1 = rng.uniform(0, 1, (1, D))
        h = gm.model._h
        fmin = gm.get_fmin()
        for _ in range(N // 768 + 3):                                     # past the build rule of the inverse factor, both handles
            dev.acquisition_function_withGradients(x1), host.acquisition_function_withGradients(x1)
        a, b = dev.acquisition_function_withGradients(x1), host.acquisition_function_withGradients(x1)
        _, t_plain = spread(lambda: h.acq_rows(x1, EI, 0.01, fmin, grad=True), 200)
        _, t_flag = spread(lambda: h.acq_rows(x1, EI | F, 0.01, fmin, grad=True), 200)
        m_dev, t_dev = spread(lambda: dev.acquisition_function_withGradients(x1), 200)
        m_host, t_host = spread(lambda: host.acquisition_function_withGradients(x1), 200)
        note = "device route faster x%.2f" % (m_host / m_dev) if m_host > m_dev else "DEVICE ROUTE SLOWER x%.2f" % (m_dev / m_host)
        lines += ["N = Nc = %5d, one location, value and gradient:" % N,
                  "    gp_acq_rows             %s" % t_plain,
                  "    gp_acq_rows, flagged    %s" % t_flag,
                  "    class, device route     %s" % t_dev,
                  "    class, host rule        %s   %s" % (t_host, note),
                  "    |difference| value %.1e  gradient %.1e" % (abs(a[0] - b[0]).max(), abs(a[1] - b[1]).max()), ""]
        if N < 16384:
            continue
        for M in (10 ** 4, 10 ** 6):
            Xs = rng.uniform(0, 1, (M, D))
            gm.model._stage(Xs)
            t0 = time.perf_counter()
            h.acq_argbest(EI, 0.01, fmin, -1)                              # the posterior of the table, once
            t_post = (time.perf_counter() - t0) * 1e3
            key = h.cost_key

            def first():
                gp = cm.cost_model.model
                h.cost_set(gp.X, gp._h.alpha(), gp.kern._kernel_id, gp.kern.ARD, float(gp.kern.variance), gp.kern.lengthscale.values, key=key)
                t0 = time.perf_counter()
                h.acq_argbest(EI | F, 0.01, fmin, -1)
                return (time.perf_counter() - t0) * 1e3
            firsts = [first() for _ in range(5)][1:]
            m_plain, t_plain = spread(lambda: h.acq_argbest(EI, 0.01, fmin, -1), 10)
            m_cached, t_cached = spread(lambda: h.acq_argbest(EI | F, 0.01, fmin, -1), 10)
            t_pass = float(np.median(firsts)) - m_cached
            floor = M * N * OPS_PER_PAIR / LANE_RATE * 1e3
            lines += ["N = Nc = %d, table of %d rows (posterior of the table, once: %.0f):" % (N, M, t_post),
                      "    gp_acq_argbest                               %s" % t_plain,
                      "    flagged, logc of the table cached            %s" % t_cached,
                      "    flagged, first call after gp_cost_set        %.3f [%.3f, %.3f]" % (np.median(firsts), min(firsts), max(firsts)),
                      "    cost pass (first - cached)                   %.3f   floor %.3f (%d fp64 vector instructions a pair at %.1fe12 lanes/s)"
                      "   fraction reached %.2f" % (t_pass, floor, OPS_PER_PAIR, LANE_RATE / 1e12, floor / t_pass), ""]
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
