"""The members of the sparse batch's cases, shared by tests/test_sparse_batch_host.py (their conditions, on the CPU) and
tests/test_gpu_sparse_batch.py (the device against the single call and against the long-double truth).

A case of tests/_sparse_ref.py (``case_inputs`` / ``case_lengthscale``) gets five members r = 0..4:
  variance     [0.65, 0.92, 1.3, 1.84, 2.6][r]
  lengthscale  the case's x [1.0, 0.8, 0.85, 0.75, 0.7][r]
  noise        [2e-2, 5e-3, 1e-2, 5e-2, 1e-1][r]
  Z_0 = the case's Z;  Z_r = Z + 0.02 RandomState(7000 + r).standard_normal(Z.shape) for r > 0
With these every run of the sparse GPU suite's RUNS has, for all five members in the float64 reference, cond(Kmm) <= 4.94e4
(inside that suite's cap of 8.9e4) and no step of either jitter ladder; longer lengthscales do not stay inside the cap (asserted in
tests/test_sparse_batch_host.py).

The stepped member: Z[1] = Z[0] and variance 2^30.  In float64 K(Z) + 1e-8 I is then K(Z) itself and its second pivot is exactly 0,
so the Kmm ladder steps exactly once, to 1e-6 x 2^30 = 1073.741824, B's ladder not at all, and the gradients stay finite; with
maxtries = 0 the member fails outright.
"""
import numpy as np

import _sparse_ref as R

VARIANCES = [0.65, 0.92, 1.3, 1.84, 2.6]
LS_FACTORS = [1.0, 0.8, 0.85, 0.75, 0.7]
NOISES = [2e-2, 5e-3, 1e-2, 5e-2, 1e-1]
NMEMBERS = 5
STEPPED_VARIANCE = 2.0 ** 30
STEPPED_JITTER = 1073.741824            # 1e-6 x (2^30 + 1e-8) in float64

FAMS = ["rbf", "Mat52", "Mat32", "Exponential"]
RUNS = [("S1", f, True) for f in FAMS] + [("S2", f, True) for f in FAMS] + [("S3", f, False) for f in FAMS] + \
       [("S5", f, False) for f in FAMS] + [("S4", f, a) for f in ("rbf", "Exponential") for a in (False, True)]
IDS = ["%s-%s-%s" % (c, f, "ard" if a else "iso") for c, f, a in RUNS]


def members_of(Z, ls):
    """(Z [5, Mz, D], variance [5], lengthscale [5, nls], noise [5]) over a base Z and a base lengthscale vector."""
    Z = np.asarray(Z, dtype=float)
    Zs = np.stack([Z if r == 0 else Z + 0.02 * np.random.RandomState(7000 + r).standard_normal(Z.shape) for r in range(NMEMBERS)])
    lss = np.stack([np.asarray(ls, dtype=float) * f for f in LS_FACTORS])
    return Zs, np.array(VARIANCES), lss, np.array(NOISES)


def members(case, ard):
    """X, Y and the five members of a case."""
    X, Y, Z, _ = R.case_inputs(case)
    return (X, Y) + members_of(Z, R.case_lengthscale(X.shape[1], ard))


def with_stepped(Zs, var, lss, noise, slot=2):
    """The same members with the stepped member in ``slot`` (its lengthscale and noise stay)."""
    Zs, var = Zs.copy(), var.copy()
    Zs[slot, 1] = Zs[slot, 0]
    var[slot] = STEPPED_VARIANCE
    return Zs, var, lss, noise


# Two shapes beyond the S cases, both RBF ARD: N crosses two 512-column chunks of the gradient pass with padding (the S cases all
# have N <= 300: one chunk); and the cap on Mz, where every tile loop over the inducing inputs runs its full length.
EXTRA = {"N1100": (1100, 40, 3, 1, 3), "MZ2048": (256, 2048, 3, 1, 2)}     # N, Mz, D, P, R


def extra_inputs(name):
    """X, Y and R members of an EXTRA shape.  Z is a subset of X moved by 0.03 N(0, 1) where Mz <= N, else uniform in the cube (with
    lengthscales a third of the cases': 2048 points in [0, 1]^3 are 0.08 apart)."""
    N, Mz, D, P, nm = EXTRA[name]
    rng = np.random.RandomState(4242 + N)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] * np.linspace(1.0, 0.5, P)[None, :] + 0.1 * rng.standard_normal((N, P))
    if Mz <= N:
        Z = X[rng.permutation(N)[:Mz]] + 0.03 * rng.standard_normal((Mz, D))
        ls = R.case_lengthscale(D, True)
    else:
        Z = rng.uniform(0, 1, (Mz, D))
        ls = R.case_lengthscale(D, True) / 3.0
    Zs, var, lss, noise = members_of(Z, ls)
    return X, Y, Zs[:nm], var[:nm], lss[:nm], noise[:nm]
