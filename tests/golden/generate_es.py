"""Generate tests/golden/es_epmgp.npz (BUILD CONTAINER ONLY: needs the reference tree, GP_REFERENCE_ROOT).

Runs the reference's ``epmgp.joint_min(mu, cov, with_derivatives=True)`` live (GPyOpt/GPyOpt/util/epmgp.py: numpy and scipy only;
under NumPy 2 the names np.NaN / np.NAN / np.Infinity it uses are aliased here first) on posteriors of small exact GPs and stores
its inputs and outputs.  Every case is the posterior -- with noise, every entry floored at 1e-10 as GPModel.predict_covariance
does -- of an oracle GP at R representer points:

  R2, R3, R8, R33     noise 1e-2: all outputs
  R20m1               N = 40, D = 2, Matern-5/2, lengthscale 0.3: some chains end with exit_flag -1 (logP = -500)
  R33m1               a 1-D model with noise 1e-3: most chains end with exit_flag -1
  R50, R64            logP, dlogPdMu and the reference's deterministic change (ES.py:145-154) for four fixed innovations m,
                      instead of the R^3 tensors

For every case tests/_es_truth.py's sweeps must stay clear of the branches a rounding difference could flip: no chain's last
sum |d| within 10 % of 1e-3, no |z| within 1e-6 of 6.  A seed that violates this is skipped for the next one.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import cpu_ref as O  # noqa: E402
from oracle import ref_leaf  # noqa: E402
import _es_truth as T  # noqa: E402

OUT = os.path.join(HERE, "es_epmgp.npz")


def reference_epmgp():
    for alias, value in (("NaN", np.nan), ("NAN", np.nan), ("Infinity", np.inf)):
        if not hasattr(np, alias):
            setattr(np, alias, value)
    path = os.path.join(ref_leaf.REF, "GPyOpt", "GPyOpt", "util", "epmgp.py")
    spec = importlib.util.spec_from_file_location("reference_epmgp", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def posterior(seed, N, D, R, kernel, lengthscale, noise):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.3 * rng.standard_normal((N, 1))
    gp = O.OracleGP(X, Y, O.make_kernel(kernel, D, 1.0, lengthscale), noise_var=noise)
    Xr = rng.uniform(0, 1, (R, D))
    mu, cov = gp.predict(Xr, full_cov=True)
    return mu.ravel().copy(), np.maximum(cov, 1e-10)


def clear_of_branches(sw):
    last = sw["last_diff"][np.isfinite(sw["last_diff"])]
    return bool(np.all(np.abs(last - 1e-3) > 1e-4) and sw["z_margin"] > 1e-6)


CASES = [  # tag, N, D, R, kernel, lengthscale, noise, compact, wants chains with exit_flag -1
    ("R2", 12, 2, 2, "rbf", 0.4, 1e-2, False, None),
    ("R3", 12, 2, 3, "Mat52", 0.5, 1e-2, False, None),
    ("R8", 25, 3, 8, "rbf", 0.6, 1e-2, False, None),
    ("R33", 40, 2, 33, "Mat52", 0.8, 1e-2, False, None),
    ("R20m1", 40, 2, 20, "Mat52", 0.3, 1e-2, False, "some"),
    ("R33m1", 30, 1, 33, "rbf", 0.2, 1e-3, False, "most"),
    ("R50", 60, 3, 50, "Mat52", 0.7, 1e-2, True, None),
    ("R64", 60, 3, 64, "rbf", 0.7, 1e-2, True, None),
]


def main():
    if not ref_leaf.available():
        raise SystemExit("reference tree absent")
    ep = reference_epmgp()
    keep = {}
    for tag, N, D, R, kernel, ls, noise, compact, minus in CASES:
        for seed in range(100, 200):
            mu, cov = posterior(seed, N, D, R, kernel, ls, noise)
            sw = T.sweeps(mu, cov)
            if not clear_of_branches(sw) or np.any(sw["status"] == -2):
                continue
            ended = int(np.sum(sw["status"] == -1))
            if minus == "some" and not 0 < ended < R // 2:
                continue
            if minus == "most" and not ended > R // 2:
                continue
            if minus is None and R <= 8 and ended:     # the small cases: every chain runs to convergence
                continue
            break
        else:
            raise SystemExit("no seed for case %s" % tag)
        with np.errstate(all="ignore"):
            logP, dMu, dSigma, dMuMu = ep.joint_min(mu, cov, with_derivatives=True)
        keep[tag + "/mu"], keep[tag + "/cov"], keep[tag + "/logP"], keep[tag + "/dlogPdMu"] = mu, cov, logP, dMu
        if compact:
            rng = np.random.RandomState(7)
            ms = 0.3 * rng.standard_normal((4, R))
            keep[tag + "/m"] = ms
            keep[tag + "/det"] = np.array([T.det_reference_style(m, dSigma, dMuMu) for m in ms])
        else:
            keep[tag + "/dlogPdSigma"], keep[tag + "/dlogPdMudMu"] = dSigma, dMuMu
        print("%-6s seed %d  R %d  chains ended %d  sweeps %d..%d  z margin %.2e" % (
            tag, seed, R, ended, sw["sweeps"].min(), sw["sweeps"].max(), sw["z_margin"]))
    np.savez_compressed(OUT, **keep)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(keep), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
