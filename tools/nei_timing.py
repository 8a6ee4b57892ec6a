"""Noisy expected improvement: what a call costs -> profiles/nei_timing.txt.

D = 8, Matern-5/2, fixed hyper-parameters, model noise 1e-2, twin noise 1e-6, the twin's inverse factor built (option
rows_build = 1), ONE pair of handles per N and ONE process.  At N = 512 and N = 16384, S = 16 and 64 fantasies:
  set     gp_nei_set: the draws through both factors (one read of L0's triangle, four substitutions of S right-hand sides)
  rows    8 locations by value: gp_nei_rows without and with dout beside gp_acq_rows (EI) without and with gradient for the SAME
          locations on the SAME (twin) handle, timed alternately
  table   10^4 resident candidates: gp_nei_table beside gp_acq (EI) over the same table on the same handle, timed alternately (both
          reuse the table's cached posterior after the first call: what is timed is the S means and the scoring against EI's
          scoring alone; the first call of each, posterior included, is given beside)
Wall time in ms of calls that end in the stream's synchronisation, median [quartiles] after warm-up.  Every figure is measured by
this tool on the machine it runs on; nothing is estimated.

Run on the GPU box:  python tools/nei_timing.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "nei_timing.txt")
D, M_ROWS, TABLE_M = 8, 8, 10000
NS, SS = (512, 16384), (16, 64)
SET_REPS, SET_WARM, ROWS_REPS, ROWS_WARM, TABLE_REPS, TABLE_WARM = 10, 2, 200, 10, 12, 2


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


def handle(X, Y, noise):
    h = _lib.Handle(0)
    h.set_data(X, Y)
    h.set_params(_lib.GP_KERNEL_MATERN52, 0, 1.0, np.array([0.9]), noise)
    h.fit()
    h.set_option("rows_build", 1)
    return h


def main():
    rng = np.random.default_rng(7)
    lines = ["noisy expected improvement: wall time per call in ms, median [quartiles]; D = %d, Matern-5/2, model noise 1e-2, twin "
             "noise 1e-6" % D, ""]
    for N in NS:
        X = rng.uniform(0, 1, (N, D))
        Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
        Y = (Y - Y.mean()) / Y.std()
        h, h0 = handle(X, Y, 1e-2), handle(X, Y, 1e-6)
        x = rng.uniform(0, 1, (M_ROWS, D))
        tab = rng.uniform(0, 1, (TABLE_M, D))
        for S in SS:
            Z, E = rng.standard_normal((S, N)), rng.standard_normal((S, N))
            (_, sset), = alternately([lambda: h0.nei.set(h, Z, E)], SET_REPS, SET_WARM)
            lines.append("N = %-5d S = %-2d  gp_nei_set %s" % (N, S, sset))
            fstar = float(h0.nei.get()[1].min())
            res = alternately([lambda: h0.nei.rows(x, 0.01), lambda: h0.nei.rows(x, 0.01, grad=True),
                               lambda: h0.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fstar),
                               lambda: h0.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fstar, grad=True)], ROWS_REPS, ROWS_WARM)
            (mv, sv), (mg, sg), (mav, sav), (mag, sag) = res
            lines.append("N = %-5d S = %-2d  M = %d rows: nei value %s   acq_rows value %s   ratio %.2f" % (N, S, M_ROWS, sv, sav, mv / mav))
            lines.append("N = %-5d S = %-2d  M = %d rows: nei grad  %s   acq_rows grad  %s   ratio %.2f" % (N, S, M_ROWS, sg, sag, mg / mag))
            h0.set_candidates(tab)
            first_nei = clocked(lambda: h0.nei.table(0.01))
            h0.set_candidates(tab)
            first_ei = clocked(lambda: h0.acq(_lib.GP_ACQ_EI, 0.01, fstar))
            (mt, st), (me, se) = alternately([lambda: h0.nei.table(0.01), lambda: h0.acq(_lib.GP_ACQ_EI, 0.01, fstar)], TABLE_REPS, TABLE_WARM)
            lines.append("N = %-5d S = %-2d  table of %d: gp_nei_table %s   gp_acq (EI) %s   ratio %.2f   (first calls, posterior "
                         "included: %.3f and %.3f)" % (N, S, TABLE_M, st, se, mt / me, first_nei, first_ei))
        lines.append("")
        h.close()
        h0.close()
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
