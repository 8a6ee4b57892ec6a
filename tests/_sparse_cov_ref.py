"""The sparse GP's JOINT posterior restated on a fit of ``_sparse_ref.inference``, in both precisions (``R.F64``, ``R.LD``).

Reference: Posterior._raw_predict with ``full_cov`` (posterior.py:229-232) over ``_predictive_variable = Z``,

    cov = K(Xs, Xs) - K(Xs, Z) woodbury_inv K(Z, Xs)     (+ noise I: gaussian.py:104-105),

in the reference's own form -- one subtraction of the full product.  The covariance between two point sets is the off-diagonal
block of that matrix over the stacked points (what ``GPRegression.posterior_covariance_between_points`` defines; the reference's
own gp.py:721 hands the training inputs to an Mz x Mz factor and cannot serve as the definition).  ``factored`` is the form the
device sums in, ``Kss - U U^T + T T^T``, for the host test that holds the two together.
"""
import numpy as np

import _sparse_ref as R


def _as(lin, *arrays):
    return [np.asarray(a, dtype=lin.dtype) for a in arrays]


def full_cov(fit, Z, Xs, noise, include_noise, lin):
    """(mean [M, P], cov [M, M], var [M]: the diagonal by posterior.py:242, before the clip of :248 and without the noise)."""
    t = lin.dtype
    kern = fit["kern"]
    Z, Xs = _as(lin, Z, Xs)
    w, Wi = fit["woodbury_vector"], fit["woodbury_inv"]
    Kx = kern.K(Xs, Z)
    cov = kern.K(Xs) - Kx @ Wi @ Kx.T
    if include_noise:
        cov = cov + t(float(noise)) * np.eye(Xs.shape[0], dtype=t)
    var = kern.variance - np.sum((Kx @ Wi) * Kx, axis=1)
    return Kx @ w, cov, var


def cov_between(fit, Z, X1, X2, lin):
    """[M1, M2]: K(X1, X2) - K(X1, Z) woodbury_inv K(Z, X2)."""
    kern = fit["kern"]
    Z, X1, X2 = _as(lin, Z, X1, X2)
    return kern.K(X1, X2) - kern.K(X1, Z) @ fit["woodbury_inv"] @ kern.K(X2, Z).T


def factored(fit, Z, Xs, lin):
    """K(Xs, Xs) - U U^T + T T^T with U = K(Xs, Z) Lm^-T and T = U LB^-T (woodbury_inv = Lm^-T (I - B^-1) Lm^-1)."""
    kern = fit["kern"]
    Z, Xs = _as(lin, Z, Xs)
    Ut = lin.solve(fit["Lm"], kern.K(Xs, Z).T, 0)
    Tt = lin.solve(fit["LB"], Ut, 0)
    return kern.K(Xs) - Ut.T @ Ut + Tt.T @ Tt


def second_draw(case, M=130):
    """A second set of locations for a case, independent of ``R.case_inputs``' draws."""
    D = R.CASES[case][2]
    return np.random.RandomState(7000 + 13 * sorted(R.CASES).index(case)).uniform(0, 1, (M, D))
