"""Writes profiles/append_timing.txt: gp_append against the refit it replaces, on one MI355X.

For N in {4096, 16384} (D = 8, RBF ARD, noise 1e-2), k in {1, 5, 8} new rows, with and without a valid explicit inverse
factor, and for both routes -- N0 = N (a multiple of 128: the border opens a new tile and every buffer moves to the new leading
dimension) and N0 = N - 64 (the border is written in place) -- the wall time of

    append : Handle.append(Xnew, Yall)                       and the first gradient gp_acq_rows call after it
    refit  : Handle.set_data(Xall, Yall) + set_params + fit  and the same call

median of REPS runs each, every run from a freshly fitted model of N0 rows.  The refit is the path gp_set_data + gp_fit took
before gp_append existed; this change leaves it as it was, so the figure stands for the parent commit on the same data.  With
the inverse factor ("Li"), option rows_build is 1 on both sides: the appended model keeps and extends it, the refitted one
rebuilds it at that first call.  Without it, rows_build is 0 on both sides.

One condition, stated in the file: append + call is faster than refit + call at both sizes, in every row.
usage: append_timing.py [out.txt]        (default: profiles/append_timing.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402

D, REPS, NOISE = 8, 3, 1e-2
PASS_TBS = 5.6      # what the one-row streaming kernels reach over the inverse factor (profiles/r05_rows_traffic.json), TB/s


def problem(N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = (np.sin(3 * X.sum(1) / np.sqrt(D)) + 0.1 * rng.standard_normal(N))[:, None]
    return X, Y, 0.5 * np.sqrt(D) * 10.0 ** rng.uniform(-0.2, 0.2, D)


def fitted(h, X, Y, ls, li):
    h.set_option("rows_build", 1 if li else 0)
    h.set_data(X, Y)
    h.set_params(0, 1, 1.0, ls, NOISE)
    h.fit()
    if li:
        h.predict_rows(X[:1] + 0.01, True)     # builds the inverse factor
    h.synchronize()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def one(h, X, Y, ls, N0, k, li):
    """(append ms, call ms, refit ms, call ms), medians of REPS."""
    x = np.full((1, D), 0.37)
    Yall = Y[:N0 + k] * 1.01
    call = lambda: h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, 0.0, grad=True)
    rec = np.empty((REPS, 4))
    for r in range(REPS):
        fitted(h, X[:N0], Y[:N0], ls, li)
        rec[r, 0] = timed(lambda: h.append(X[N0:N0 + k], Yall))
        rec[r, 1] = timed(call)
        fitted(h, X[:N0], Y[:N0], ls, li)

        def refit():
            h.set_data(X[:N0 + k], Yall)
            h.set_params(0, 1, 1.0, ls, NOISE)
            h.fit()
        rec[r, 2] = timed(refit)
        rec[r, 3] = timed(call)
    return np.median(rec, axis=0)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "append_timing.txt")
    lines = ["gp_append against gp_set_data + gp_fit (tools/append_timing.py): D = %d, RBF ARD, noise %g, median of %d, wall ms" % (D, NOISE, REPS),
             "call = the first gradient gp_acq_rows (EI, one location) afterwards; pass = one read of the lower triangle of L^-1 at %.1f TB/s" % PASS_TBS,
             "",
             "%6s %6s %2s %3s %-9s | %9s %8s | %9s %8s | %7s %11s" % ("N", "N0", "k", "Li", "route", "append", "call", "refit", "call", "ratio", "append/pass")]
    worst = np.inf
    h = _lib.Handle(0)
    for N in (4096, 16384):
        X, Y, ls = problem(N + 8)
        pass_ms = 8.0 * N * N / 2 / (PASS_TBS * 1e12) * 1e3
        for N0, route in ((N, "new tile"), (N - 64, "in place")):
            for li in (1, 0):
                for k in (1, 5, 8):
                    a, ac, f, fc = one(h, X, Y, ls, N0, k, li)
                    ratio = (f + fc) / (a + ac)
                    worst = min(worst, ratio)
                    lines.append("%6d %6d %2d %3s %-9s | %9.3f %8.3f | %9.3f %8.3f | %6.1fx %11.1f" % (
                        N, N0, k, "yes" if li else "no", route, a, ac, f, fc, ratio, a / pass_ms))
                    print(lines[-1], flush=True)
        lines.append("  (one pass at N = %d: %.3f ms)" % (N, pass_ms))
    # where an append's time goes: the library's own phase events (gp_last_phases) of one call per route at the larger size
    lines += ["", "phases of one append at N = 16384, k = 8 (HIP events on the stream, ms; the rest of the wall time is host: allocation,",
              "hand-overs of the pivots and the scalars):"]
    X, Y, ls = problem(16384 + 8)
    for N0, route in ((16384, "new tile"), (16320, "in place")):
        for li in (1, 0):
            fitted(h, X[:N0], Y[:N0], ls, li)
            wall = timed(lambda: h.append(X[N0:N0 + 8], Y[:N0 + 8]))
            lines.append("  %-8s Li %-3s wall %6.3f | %s" % (route, "yes" if li else "no", wall,
                                                           "  ".join("%s %.3f" % (p["name"].replace("append_", ""), p["ms"]) for p in h.phases())))
    s = h.append_stats()
    h.close()
    lines += ["", "ratio = (refit + call) / (append + call); the smallest over all rows: %.1fx -- the condition (append faster than the refit at" % worst,
              "both sizes) %s.  Borders written: %d in place, %d into a new tile, %d refused." % ("HOLDS" if worst > 1.0 else "FAILS", s[0], s[1], s[2])]
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))
    return 0 if worst > 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
