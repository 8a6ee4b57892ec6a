"""The sparse GP's oracle: ``VarDTC.inference`` and the sparse prediction restated over the oracle's kernels, in two precisions.

Reference, line for line: GPy/GPy/inference/latent_function_inference/var_dtc.py:66-277 (``inference``, ``_compute_dL_dpsi``,
``_compute_dL_dR``, ``_compute_log_marginal_likelihood``; homoscedastic, certain inputs, no mean function),
GPy/GPy/core/sparse_gp.py:108-118 (the gradients' assembly), posterior.py:225-248 (prediction through ``woodbury_inv``),
GPy/GPy/core/gp.py:432-453 (``predictive_gradients`` over Z), GPyOpt/GPyOpt/models/gpmodel.py:125-129 (``get_fmin``).

* ``F64``: float64 with the oracle's LAPACK wrappers (``oracle.cpu_ref.jitchol`` / ``dtrtrs``).
* ``LD``: ``np.longdouble`` (x87 80-bit, eps 1.1e-19) with a hand-written Cholesky and substitutions as in
  tests/golden/generate_truth.py -- the truth.

Distances are the direct-difference ones of ``tests/_kernel_families.make(..., direct=True)`` in both precisions
(``extended=True`` for the truth): with Z a subset of X the Gram trick leaves r ~ 1e-8 instead of 0 on coincident pairs, which
the Exponential family's kink at r = 0 turns into an O(1) error of the lengthscale gradient.  ``K_of_r`` / ``dK_dr`` are
restated here with their constants in the working precision (the oracle's classes carry float64 constants such as
``np.sqrt(5.)``, which would cap the truth at 1e-16); tests/test_sparse_gp_host.py holds the float64 ones to the oracle's.
"""
import numpy as np

from oracle import cpu_ref as O
import _kernel_families as KF

CONST_JITTER = 1e-8      # var_dtc.py:32


# ---- the two arithmetics ---------------------------------------------------------------------------------------------------
class F64(object):
    dtype = np.float64

    @staticmethod
    def chol(A):
        """(L, jitter the ladder ended with)."""
        return O.jitchol(np.ascontiguousarray(A, dtype=np.float64))

    @staticmethod
    def solve(L, B, trans=0):
        """L X = B (trans 0) or L^T X = B (trans 1)."""
        return O.dtrtrs(L, np.asarray(B, dtype=np.float64), lower=1, trans=trans)[0]


class LD(object):
    dtype = np.longdouble

    @staticmethod
    def chol(A):
        """Unblocked left-looking Cholesky; no ladder: a non-positive pivot is an error of the test's inputs."""
        n = A.shape[0]
        L = np.zeros_like(A)
        for j in range(n):
            v = A[j:, j] - L[j:, :j] @ L[j, :j]
            if not v[0] > 0:
                raise np.linalg.LinAlgError("not positive definite in long double")
            L[j, j] = np.sqrt(v[0])
            L[j + 1:, j] = v[1:] / L[j, j]
        return L, 0.0

    @staticmethod
    def solve(L, B, trans=0):
        X = np.array(B, dtype=np.longdouble, copy=True)
        n = L.shape[0]
        if trans == 0:
            for i in range(n):
                X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
        else:
            for i in range(n - 1, -1, -1):
                X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
        return X


def backsub_both_sides(lin, L, X):
    """L^-T X L^-1 (linalg.py:381-387)."""
    tmp = lin.solve(L, X, 1)
    return lin.solve(L, tmp.T, 1).T


# ---- the four families in the working precision ------------------------------------------------------------------------------
def k_of_r(name, variance, r):
    t = r.dtype.type
    if name == "rbf":               # rbf.py:50-51
        return variance * np.exp(-t(0.5) * r * r)
    if name == "Mat52":             # stationary.py:575-576
        s5 = np.sqrt(t(5))
        return variance * (1 + s5 * r + t(5) / 3 * r * r) * np.exp(-s5 * r)
    if name == "Mat32":             # stationary.py:478-479
        s3 = np.sqrt(t(3))
        return variance * (1 + s3 * r) * np.exp(-s3 * r)
    assert name == "Exponential"    # stationary.py:388-389
    return variance * np.exp(-r)


def dk_dr(name, variance, r):
    t = r.dtype.type
    if name == "rbf":               # rbf.py:53-54
        return -r * k_of_r(name, variance, r)
    if name == "Mat52":             # stationary.py:578-579
        s5 = np.sqrt(t(5))
        return variance * (t(10) / 3 * r - 5 * r - 5 * s5 / 3 * r * r) * np.exp(-s5 * r)
    if name == "Mat32":             # stationary.py:481-482
        s3 = np.sqrt(t(3))
        return -3 * variance * r * np.exp(-s3 * r)
    return -k_of_r(name, variance, r)


class Kern(object):
    """A stationary covariance in the arithmetic ``lin``: distances from the oracle's direct-difference kernel."""

    def __init__(self, name, D, variance, lengthscale, ARD, lin):
        self.name, self.D, self.ARD, self.lin = name, D, bool(ARD), lin
        t = lin.dtype
        self.variance = t(float(variance))
        ls = np.asarray(lengthscale, dtype=float).reshape(-1)
        self.ls = np.asarray(ls if ls.size == D else np.full(D, ls[0]), dtype=t)
        self._dist = KF.make(name, D, float(variance), ls if ARD else ls[:1], ARD, direct=True, extended=lin is LD)

    def r(self, X, X2=None):
        return np.asarray(self._dist._scaled_dist(X, X2), dtype=self.lin.dtype)

    def K(self, X, X2=None):
        return k_of_r(self.name, self.variance, self.r(X, X2))

    def _tmp(self, dL_dK, X, X2):
        r = self.r(X, X2)
        inv = np.where(r != 0, 1 / np.where(r != 0, r, 1), 0)            # _inv_dist, stationary.py:251-258
        return r, dk_dr(self.name, self.variance, r) * dL_dK, inv

    def update_gradients_full(self, dL_dK, X, X2=None):
        """stationary.py:218-238: (dvariance, dlengthscale [1 or D])."""
        r, dL_dr, inv = self._tmp(dL_dK, X, X2)
        dvar = np.sum(k_of_r(self.name, self.variance, r) * dL_dK) / self.variance
        if not self.ARD:
            return dvar, np.array([-np.sum(dL_dr * r) / self.ls[0]])
        tmp = dL_dr * inv
        X2 = X if X2 is None else X2
        return dvar, np.array([-np.sum(tmp * (X[:, q:q + 1] - X2[:, q:q + 1].T) ** 2) / self.ls[q] ** 3 for q in range(self.D)])

    def gradients_X(self, dL_dK, X, X2=None):
        """stationary.py:336-352."""
        _, dL_dr, inv = self._tmp(dL_dK, X, X2)
        tmp = inv * dL_dr
        if X2 is None:
            tmp = tmp + tmp.T
            X2 = X
        grad = np.empty(X.shape, dtype=self.lin.dtype)
        for q in range(self.D):
            grad[:, q] = np.sum(tmp * (X[:, q][:, None] - X2[:, q][None, :]), axis=1) / self.ls[q] ** 2
        return grad


# ---- VarDTC ------------------------------------------------------------------------------------------------------------------
def inference(name, X, Z, Y, variance, lengthscale, ARD, noise, lin, grads=True):
    """``VarDTC.inference`` + ``SparseGP._update_gradients``.  Returns a dict: lml, woodbury_vector [Mz, P], woodbury_inv
    [Mz, Mz], dvariance, dlengthscale, dnoise, dZ, the ladders' jitters, and the pieces the reference pin compares."""
    t = lin.dtype
    X, Z, Y = (np.asarray(a, dtype=t) for a in (X, Z, Y))
    N, P = Y.shape
    Mz, D = Z.shape
    kern = Kern(name, D, variance, lengthscale, ARD, lin)
    eye = np.eye(Mz, dtype=t)
    beta = 1 / max(t(float(noise)), t(CONST_JITTER))                      # var_dtc.py:80
    VVT_factor = beta * Y                                                 # :88
    trYYT = np.sum(np.square(Y))                                          # :89 (get_trYYT)
    Kmm = kern.K(Z) + t(CONST_JITTER) * eye                               # :93-94
    Lm, jit_kmm = lin.chol(Kmm)                                           # :95
    psi0 = np.full(N, kern.variance, dtype=t)                             # :123
    psi1 = kern.K(X, Z)                                                   # :125
    tmp = lin.solve(Lm, (psi1 * np.sqrt(beta)).T, 0)                      # :129-130
    A = tmp @ tmp.T                                                       # :131
    B = eye + A                                                           # :134
    LB, jit_b = lin.chol(B)                                               # :135
    tmp = lin.solve(Lm, psi1.T, 0)                                        # :138
    LBi_Lmi_psi1 = lin.solve(LB, tmp, 0)                                  # :139
    LBi_Lmi_psi1Vf = LBi_Lmi_psi1 @ VVT_factor                            # :140
    tmp = lin.solve(LB, LBi_Lmi_psi1Vf, 1)                                # :141
    Cpsi1Vf = lin.solve(Lm, tmp, 1)                                       # :142
    delit = LBi_Lmi_psi1Vf @ LBi_Lmi_psi1Vf.T                             # :148
    data_fit = np.trace(delit)                                            # :149
    DBi_plus_BiPBi = backsub_both_sides(lin, LB, P * eye + delit)         # :150
    delit = -t(0.5) * DBi_plus_BiPBi - t(0.5) * B * P + P * eye           # :152-154
    dL_dKmm = backsub_both_sides(lin, Lm, delit)                          # :156
    # _compute_dL_dpsi, :218-234
    dL_dpsi0 = -t(0.5) * P * (beta * np.ones(N, dtype=t))
    dL_dpsi1 = VVT_factor @ Cpsi1Vf.T
    dL_dpsi2_beta = t(0.5) * backsub_both_sides(lin, Lm, P * eye - DBi_plus_BiPBi)
    dL_dpsi1 = dL_dpsi1 + 2 * (psi1 @ (beta * dL_dpsi2_beta))
    # _compute_log_marginal_likelihood, :266-277
    lik_1 = -t(0.5) * N * P * (np.log(2 * (np.arctan(t(1)) * 4)) - np.log(beta)) - t(0.5) * beta * trYYT
    lik_2 = -t(0.5) * P * (np.sum(beta * psi0) - np.trace(A))
    lik_3 = -P * np.sum(np.log(np.diag(LB)))
    lik_4 = t(0.5) * data_fit
    lml = lik_1 + lik_2 + lik_3 + lik_4
    # _compute_dL_dR, :261-263
    dL_dR = -t(0.5) * N * P * beta + t(0.5) * trYYT * beta ** 2
    dL_dR += t(0.5) * P * (psi0.sum() * beta ** 2 - np.trace(A) * beta)
    dL_dR += beta * (t(0.5) * np.sum(A * DBi_plus_BiPBi) - data_fit)
    # posterior, :209-212
    Bi = eye - lin.solve(LB, lin.solve(LB, eye, 0), 1)
    woodbury_inv = backsub_both_sides(lin, Lm, Bi)
    out = dict(lml=lml, woodbury_vector=Cpsi1Vf, woodbury_inv=woodbury_inv, dnoise=dL_dR, jitter_kmm=jit_kmm, jitter_b=jit_b,
               beta=beta, Kmm=Kmm, Lm=Lm, LB=LB, A=A, psi0=psi0, psi1=psi1, VVT_factor=VVT_factor, trYYT=trYYT, data_fit=data_fit,
               DBi_plus_BiPBi=DBi_plus_BiPBi, LBi_Lmi_psi1Vf=LBi_Lmi_psi1Vf, dL_dKmm=dL_dKmm, dL_dpsi0=dL_dpsi0,
               dL_dpsi1=dL_dpsi1, dL_dpsi2_beta=dL_dpsi2_beta, kern=kern)
    if grads:
        # sparse_gp.py:110-118
        dv_nm, dl_nm = kern.update_gradients_full(dL_dpsi1, X, Z)
        dv_mm, dl_mm = kern.update_gradients_full(dL_dKmm, Z, None)
        out["dvariance"] = np.sum(dL_dpsi0) + dv_nm + dv_mm                # update_gradients_diag: stationary.py:240-242
        out["dlengthscale"] = dl_nm + dl_mm
        out["dZ"] = kern.gradients_X(dL_dKmm, Z) + kern.gradients_X(dL_dpsi1.T, Z, X)
    return out


def predict(fit, Z, Xs, noise, include_noise, lin, grads=True):
    """posterior.py:225-248 and gp.py:432-453 on a fit of ``inference``: mean [M, P], var [M], dmdx [M, D, P], dvdx [M, D]."""
    t = lin.dtype
    kern = fit["kern"]
    Z, Xs = np.asarray(Z, dtype=t), np.asarray(Xs, dtype=t)
    w, Wi = fit["woodbury_vector"], fit["woodbury_inv"]
    Kx = kern.K(Xs, Z)                                                    # [M, Mz] = Kx^T of the reference
    mean = Kx @ w
    var = kern.variance - np.sum((Kx @ Wi) * Kx, axis=1)                  # posterior.py:242 (woodbury_inv.T Kx)
    var = np.clip(var, t(1e-15), np.inf)                                  # :248
    if include_noise:
        var = var + t(float(noise))
    if not grads:
        return mean, var
    M, D = Xs.shape
    dmdx = np.empty((M, D, w.shape[1]), dtype=t)
    for p in range(w.shape[1]):
        dmdx[:, :, p] = kern.gradients_X(np.broadcast_to(w[:, p][None, :], Kx.shape), Xs, Z)
    dvdx = kern.gradients_X(-2 * (Kx @ Wi), Xs, Z)                        # gp.py:451-453 (gradients_X_diag is zero)
    return mean, var, dmdx, dvdx


def fmin(fit, X):
    """gpmodel.py:125-129 on the sparse posterior: the smallest posterior mean over the training inputs, first output."""
    return np.min((fit["psi1"] @ fit["woodbury_vector"])[:, 0])


# ---- the GPU cases' inputs (tests/test_gpu_sparse_gp.py; their conditions are checked on the CPU by tests/test_sparse_gp_host.py)
CASES = {"S1": (96, 10, 3, 1), "S2": (300, 130, 3, 2), "S3": (130, 128, 3, 1), "S4": (200, 40, 17, 1), "S5": (64, 1, 2, 1)}
VARIANCE, NOISE = 1.3, 2e-2


def case_inputs(case, seed=1):
    """X, Y, Z, Xs (130 candidate rows) of a case: inputs uniform in [0, 1]^D, the first half of Z on data rows, the second
    half moved by 0.03 N(0, 1).  The default seed is one at which every run of the GPU suite has cond(Kmm) <= 8.9e4, no step of
    either jitter ladder and a smallest predictive variance at the data >= 2.9e-3 (asserted in tests/test_sparse_gp_host.py)."""
    N, Mz, D, P = CASES[case]
    rng = np.random.RandomState(1000 + seed + 17 * sorted(CASES).index(case))
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] * np.linspace(1.0, 0.5, P)[None, :] + 0.1 * rng.standard_normal((N, P))
    Z = X[rng.permutation(N)[:Mz]].copy()
    half = Mz // 2
    Z[half:] += 0.03 * rng.standard_normal((Mz - half, D))
    Xs = rng.uniform(0, 1, (130, D))
    return X, Y, Z, Xs


def case_lengthscale(D, ard):
    ls = np.linspace(0.15, 0.35, D) * np.sqrt(D / 3.0)
    return ls if ard else ls[:1]
