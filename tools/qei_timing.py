"""Joint expected improvement: what a call costs -> profiles/qei_timing.txt.

Per N = 512, 4096, 16384 (D = 8, Matern-5/2, fixed hyper-parameters, the inverse factor built: option rows_build = 1), q = 1, 4, 8
and S = 256, 4096, on ONE handle and in ONE process:
  value     gp_qei_rows without dout            (forward pass, Gram, joint step)
  grad      gp_qei_rows with dout               (+ backward pass, closing pass)
  acq_rows  gp_acq_rows (EI) with gradient for the SAME q locations: the existing call, the yardstick
  ratio     grad / acq_rows
Wall time in ms of calls that end in the stream's synchronisation, median [quartiles] after warm-up; the two gradient calls are
timed alternately, repetition by repetition.  Then, with gp_profile on (events around every launch: a run of its own, its wall
times are not used), the per-launch device times of a gradient call from gp_last_phases, medians.  Where a ratio exceeds 1.5 the
line names the launch of the call's own that takes the most device time.  Every figure is measured by this tool on the machine it
runs on; nothing is estimated.

Run on the GPU box:  python tools/qei_timing.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "qei_timing.txt")
D = 8
SIZES, QS, SS = (512, 4096, 16384), (1, 4, 8), (256, 4096)
REPS, WARM, PROFILED = 200, 10, 20
OWN = ("qei_gram", "qei_joint", "qei_close")


def quartiles(t):
    q = np.percentile(t, [25, 50, 75])
    return q[1], "%.3f [%.3f, %.3f]" % (q[1], q[0], q[2])


def clocked(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    rng = np.random.default_rng(7)
    lines = ["joint expected improvement: wall time per call in ms, median [quartiles], %d repetitions after %d; D = %d, Matern-5/2"
             % (REPS, WARM, D),
             "ratio = gp_qei_rows with gradient / gp_acq_rows (EI) with gradient for the same q locations, timed alternately", ""]
    kernels = ["", "device time per launch of a gradient call in ms (gp_profile on, medians of %d calls)" % PROFILED, ""]
    for N in SIZES:
        X = rng.uniform(0, 1, (N, D))
        Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
        h = _lib.Handle(0)
        h.set_data(X, (Y - Y.mean()) / Y.std())
        h.set_params(_lib.GP_KERNEL_MATERN52, 0, 1.0, np.array([0.9]), 1e-2)
        h.fit()
        h.set_option("rows_build", 1)
        fmin = h.fmin()
        for q in QS:
            x = rng.uniform(0, 1, (q, D))
            for S in SS:
                h.qei_set(rng.standard_normal((S, q)))
                value = lambda: h.qei_rows(x, 0.01, fmin)                                    # noqa: E731
                grad = lambda: h.qei_rows(x, 0.01, fmin, grad=True)                          # noqa: E731
                acq = lambda: h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)           # noqa: E731
                for _ in range(WARM):
                    value(), grad(), acq()
                tv = [clocked(value) for _ in range(REPS)]
                tg, ta = [], []
                for _ in range(REPS):
                    tg.append(clocked(grad))
                    ta.append(clocked(acq))
                (_, sv), (mg, sg), (ma, sa) = quartiles(tv), quartiles(tg), quartiles(ta)
                h.profile(1)
                per = {}
                for _ in range(PROFILED):
                    grad()
                    for p in h.phases():
                        per.setdefault(p["name"], []).append(p["ms"])
                acq()
                rows_ms = sum(p["ms"] for p in h.phases())
                h.profile(0)
                med = {k: float(np.median(v)) for k, v in per.items()}
                note = ""
                if mg / ma > 1.5:
                    worst = max(OWN, key=lambda k: med.get(k, 0.0))
                    note = "   ratio > 1.5: of the call's own launches %s takes the most (%.3f ms)" % (worst, med.get(worst, 0.0))
                lines.append("N = %-5d q = %d S = %-4d  value %s   grad %s   acq_rows %s   ratio %.2f%s" % (N, q, S, sv, sg, sa, mg / ma, note))
                kernels.append("N = %-5d q = %d S = %-4d  %s   | gp_acq_rows' three launches %.3f"
                               % (N, q, S, "  ".join("%s %.3f" % (k[4:], med[k]) for k in
                                                     ("qei_forward", "qei_gram", "qei_joint", "qei_backward", "qei_close") if k in med), rows_ms))
        h.close()
    lines += kernels + [""]
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
