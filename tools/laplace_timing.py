"""GP classification (Laplace): what the fit costs against its factorisations alone -> profiles/laplace_timing.txt.

Per size N (512, 4096, 16384; D = 8, Matern-5/2, variance 4, fixed hyper-parameters; labels the sign of a smooth function plus
noise), median and quartiles after warm-up, each call drained (the entries return after their last hand-over):
  gp_laplace_fit        the Newton iteration and the Laplace-fitted state
  gp_laplace_fit_grad   ... and d log Z / d (variance, lengthscale): R = (K + W^-1)^-1 as Ky^-1 is built, two products, the tile pass
  steps x gp_fit        (Newton steps of that fit) x (gp_fit at the same N, kernel and parameters, noise 1): what the
                        factorisations alone cost -- the figure to beat down to.  With --parent ROOT (a checkout of the parent
                        commit with its library built) gp_fit is timed there, in a process of its own in the same run; without
                        it, on this tree (the feature adds host-side branches to gp_fit and no launch)
The ratio fit / (steps x gp_fit) is what a step spends beside its factorisation: the scaling pass that writes B (N^2, reads K),
the two matrix-vector products with K (N^2 each, one wavefront a row), the site, direction and objective kernels (N), and the
per-step hand-over -- one small copy and one stream drain, after which the host decides on halving and stopping.  gp_fit's own
K build is in its figure once per step, the Laplace fit builds K once per call.

Run on the GPU box:  python tools/laplace_timing.py [--parent ROOT] [N ...]
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_optimization_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "laplace_timing.txt")
D = 8


def spread(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(t, [25, 50, 75])
    return q[1], "%.3f [%.3f, %.3f]" % (q[1], q[0], q[2])


PARENT_SNIPPET = """
import sys, time, numpy as np
from gaussian_process_optimization_amd import _lib
N, D, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
rng = np.random.default_rng(0)
X = rng.uniform(0, 1, (N, D))
h = _lib.Handle(0)
h.set_data(X, np.sign(np.sin(3 * X.sum(1)))[:, None])
h.set_params(_lib.GP_KERNEL_MATERN52, 0, 4.0, np.array([0.9]), 1.0)
h.fit()
t = []
for _ in range(reps):
    t0 = time.perf_counter(); h.fit(); t.append((time.perf_counter() - t0) * 1e3)
print(" ".join("%.6f" % v for v in np.percentile(t, [25, 50, 75])))
"""


def parent_fit(root, N, reps):
    """gp_fit of the checkout at ``root`` (its own package and library), in a fresh process: quartiles in ms."""
    env = dict(os.environ, PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", PARENT_SNIPPET, str(N), str(D), str(reps)], cwd=root, env=env, check=True,
                         stdout=subprocess.PIPE, text=True).stdout.split()
    q = [float(v) for v in out[-3:]]
    return q[1], "%.3f [%.3f, %.3f]" % (q[1], q[0], q[2])


def main():
    args = sys.argv[1:]
    parent = None
    if "--parent" in args:
        i = args.index("--parent")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    sizes = [int(a) for a in args] or [512, 4096, 16384]
    rng = np.random.default_rng(0)
    lines = ["GP classification, Laplace probit fit: wall time in ms, median [quartiles]; D = %d, Matern-5/2, variance 4" % D, ""]
    for N in sizes:
        X = rng.uniform(0, 1, (N, D))
        lat = np.sin(3 * X.sum(1)) + 0.5 * np.cos(5 * X[:, 0]) + 0.3 * rng.standard_normal(N)
        y = np.where(lat > 0, 1.0, -1.0)
        h = _lib.Handle(0)
        h.set_data(X, (y[:, None] + 1) / 2)
        h.set_params(_lib.GP_KERNEL_MATERN52, 0, 4.0, np.array([0.9]), 1.0)
        reps = 10 if N <= 4096 else 3
        steps = h.laplace_fit(y)[2]
        t_fit, s_fit = spread(lambda: h.laplace_fit(y), reps)
        t_grad, s_grad = spread(lambda: h.laplace_fit_grad(y, 1), reps)
        it, hv, wmin, wmax = h.laplace_info()
        t_reg, s_reg = parent_fit(parent, N, reps) if parent else spread(lambda: h.fit(), reps)
        lines.append("N = %d: %d Newton steps, %d halvings, W in [%.3g, %.3g]" % (N, it, hv, wmin, wmax))
        lines.append("  gp_laplace_fit                 %s" % s_fit)
        lines.append("  gp_laplace_fit_grad            %s" % s_grad)
        lines.append("  gp_fit (%s)%s%s" % ("parent commit" if parent else "this tree", " " * (17 if parent else 21), s_reg))
        lines.append("  steps x gp_fit                 %.3f" % (steps * t_reg))
        lines.append("  fit / (steps x gp_fit)         %.2f   (the remainder: scaling pass, two K products, vector kernels, "
                     "the per-step hand-over)" % (t_fit / (steps * t_reg)))
        lines.append("  gradient part                  %.3f" % (t_grad - t_fit))
        lines.append("")
        h.close()
    open(OUT, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
