"""Writes profiles/ens_timing.txt: one integrated-EI gradient call over a resident ensemble (gp_ens_acq_rows, one location, S = 10)
at N = 300, 1000, 2000 against what the library offered before for the same result -- ten contexts with resident fits, one
gp_acq_rows each, averaged on the host -- in the same session: median of 200 calls after 20 warm-ups.  Also the kernel launches
per call at S = 1 and S = 10, from kernel traces of child processes of this script (rocprofv3 --kernel-trace; a run of 11 calls
minus a run of 1 call, over 10), when rocprofv3 is at hand.  A record, with one condition stated in it: the ensemble call is not
slower than the ten single calls at any of the three sizes.
usage: ens_timing.py [out.txt]        (default: profiles/ens_timing.txt)
       ens_timing.py --calls S K      (child mode: fit S members at N = 300, make K gradient calls)"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402

D, S, WARM, REPS = 8, 10, 20, 200
EI, JITTER = _lib.GP_ACQ_EI, 0.01


def problem(N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = (np.sin(3 * X.sum(1) / np.sqrt(D)) + 0.1 * rng.standard_normal(N))[:, None]
    return X, Y


def members(n, seed=1):
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(-0.3, 0.3, n), 0.5 * np.sqrt(D) * 10.0 ** rng.uniform(-0.2, 0.2, (n, D)), 10.0 ** rng.uniform(-2.5, -1.5, n))


def median_ms(fn):
    for _ in range(WARM):
        fn()
    t = np.empty(REPS)
    for i in range(REPS):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return 1e3 * float(np.median(t))


def child(n_members, calls):
    X, Y = problem(300)
    var, ls, noise = members(n_members)
    h = _lib.Handle(0)
    h.set_data(X, Y)
    h.set_params(0, 1, var[0], ls[0], noise[0])
    h.ens_fit(var, ls, noise)
    x = np.full((1, D), 0.37)
    for _ in range(calls):
        h.ens_acq_rows(x, EI, JITTER, grad=True)
    h.close()


def traced_launches(n_members, calls):
    """Kernel dispatches of a child run, or None when no trace could be taken."""
    if shutil.which("rocprofv3") is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--calls",
               str(n_members), str(calls)]
        try:
            run = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        except (OSError, subprocess.TimeoutExpired):
            return None
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if run.returncode != 0 or not files:
            return None
        n = 0
        for f in files:
            with open(f) as fh:
                n += sum(1 for _ in csv.DictReader(fh))
        return n


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--calls":
        child(int(sys.argv[2]), int(sys.argv[3]))
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ens_timing.txt")
    text = ["Integrated-EI gradient call over a resident ensemble on an MI355X: tools/ens_timing.py.",
            "One location, D = %d, RBF ARD, S = %d members; median of %d calls after %d warm-ups, host wall time per call (ms)." % (D, S, REPS, WARM),
            "'ten singles': ten contexts with resident fits (inverse factors built), one gp_acq_rows (gradient) each and the mean on the host --",
            "what the library offered for the same result before the ensemble entries.", "",
            "%6s %14s %14s %8s %14s %14s" % ("N", "gp_ens_acq_rows", "ten singles", "ratio", "value call", "ens_fit (ms)")]
    slower = []
    x = np.full((1, D), 0.37)
    for N in (300, 1000, 2000):
        X, Y = problem(N)
        var, ls, noise = members(S)
        h = _lib.Handle(0)
        h.set_data(X, Y)
        h.set_params(0, 1, var[0], ls[0], noise[0])
        t0 = time.perf_counter()
        _, _, _, fmin = h.ens_fit(var, ls, noise)
        t_fit = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        h.ens_fit(var, ls, noise)
        t_fit = min(t_fit, 1e3 * (time.perf_counter() - t0))
        singles = []
        for z in range(S):
            hz = _lib.Handle(0)
            hz.set_data(X, Y)
            hz.set_params(0, 1, var[z], ls[z], noise[z])
            hz.fit()
            singles.append((hz, hz.fmin()))

        def ensemble():
            return h.ens_acq_rows(x, EI, JITTER, grad=True)

        def ten():
            tot, dtot = 0.0, 0.0
            for hz, fz in singles:
                a, da = hz.acq_rows(x, EI, JITTER, fz, grad=True)
                tot, dtot = tot + a, dtot + da
            return tot / S, dtot / S

        a, b = ensemble(), ten()
        agree = max(float(np.max(np.abs(a[0] - b[0]))), float(np.max(np.abs(a[1] - b[1]))))
        t_e, t_s = median_ms(ensemble), median_ms(ten)
        t_v = median_ms(lambda: h.ens_acq_rows(x, EI, JITTER))
        text.append("%6d %14.4f %14.4f %8.2f %14.4f %14.2f   (the two results differ by %.1e)" % (N, t_e, t_s, t_s / t_e, t_v, t_fit, agree))
        if t_e > t_s:
            slower.append(N)
        for hz, _ in singles:
            hz.close()
        h.close()
    text += ["", "Condition (the ensemble call is not slower than the ten single calls at any of the three sizes): %s."
             % ("MET" if not slower else "NOT MET at N = %s" % ", ".join(map(str, slower))), ""]
    counts = {}
    for n_members in (1, 10):
        a, b = traced_launches(n_members, 1), traced_launches(n_members, 11)
        counts[n_members] = None if a is None or b is None else (b - a) / 10.0
    if None in counts.values():
        text.append("Kernel launches per gradient call: no kernel trace could be taken here; by construction (csrc/ens_rows.hip, launch_ens_rows) "
                    "a pass is ens_forward_kernel, ens_backward_kernel, ens_finish_kernel with the member in blockIdx.y: 3 at any S.")
    else:
        text.append("Kernel launches per gradient call (rocprofv3 --kernel-trace of child runs, N = 300: 11 calls minus 1 call, over 10): "
                    "S = 1: %.1f, S = 10: %.1f." % (counts[1], counts[10]))
    with open(out_path, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
