"""CPU: the long-double truth of the probability of feasibility (tests/_feas_truth.py) against float64 SciPy and against central
differences, at and around the branch points of the device's log Phi (z = -20 and z = 6) and deep in the tail (z = -45)."""
import numpy as np
import pytest
from scipy.stats import norm

import _feas_truth as FT

T = FT.T
ZS = (-45.0, -25.0, -20.0 - 1e-9, -20.0, -20.0 + 1e-9, -10.0, -1.0, 0.0, 2.5, 6.0 - 1e-9, 6.0, 6.0 + 1e-9, 8.0)


@pytest.mark.parametrize("z", ZS)
def test_log_ndtr_against_scipy(z):
    got, ref = float(FT.log_ndtr(z)), norm.logcdf(z)
    # scipy's log_ndtr is good to a few ulp of its value (1e-15 relative); 1e-13 leaves room for its series below -20
    assert abs(got - ref) <= 1e-13 * abs(ref)


@pytest.mark.parametrize("z0", (-20.0, 6.0))
def test_the_branch_points_join(z0):
    """Across a branch point the truth moves by lambda(z0) dz, not by a jump."""
    dz = T(1e-7)
    lo, hi = FT.log_ndtr(T(z0) - dz), FT.log_ndtr(T(z0) + dz)
    lam = FT.mills(z0)
    assert abs((hi - lo) - 2 * dz * lam) <= 1e-6 * 2 * dz * lam


@pytest.mark.parametrize("z", ZS)
def test_mills_is_the_derivative(z):
    h = T(1e-6) * max(1.0, abs(z))
    num = (FT.log_ndtr(T(z) + h) - FT.log_ndtr(T(z) - h)) / (2 * h)
    lam = FT.mills(z)
    # central differences, also ACROSS the truth's branch at -20: truncation h^2 |third derivative| / 6 ~ 1e-12, cancellation
    # 1e-16 |log Phi| / h <= 1e-9 (erfc comes in double above -20), both relative to lambda >= |z|
    assert abs(num - lam) <= 1e-8 * lam
    if z <= -20:
        assert abs(float(lam) + z) < 0.06                         # lambda ~ -z in the tail: finite where Phi underflows


def _posterior(x, K):
    """An analytic 'posterior' over x [M, D]: means, variances and their gradients per constraint."""
    D = x.shape[1]
    mean, var, dm, dv = [], [], [], []
    for k in range(K):
        w = np.cos(0.9 * (k + 1) * np.arange(1, D + 1))
        mean.append(np.sin(x @ w) + 0.1 * k)
        dm.append(np.cos(x @ w)[:, None] * w)
        var.append(0.05 + ((x - 0.2 * k) ** 2).sum(1))
        dv.append(2 * (x - 0.2 * k))
    return tuple(np.stack(a) for a in (mean, var, dm, dv))


@pytest.mark.parametrize("K,D,shift", [(1, 1, 0.0), (3, 4, -3.0), (8, 2, -30.0), (2, 3, 5.0)])
def test_fold_gradient_against_central_differences(K, D, shift):
    rng = np.random.default_rng(K * 10 + D)
    x = rng.uniform(0, 1, (4, D))
    c_mean, c_std = rng.uniform(-1, 1, K), rng.uniform(0.5, 2.0, K)
    bound = c_mean + shift
    f = FT.fold(*_posterior(x, K), c_mean, c_std, bound)
    assert f.logF.shape == (4,) and f.dlogF.shape == (4, D)
    assert np.all(f.bound_logF > 0) and np.all(f.bound_dlogF > 0)
    h = 1e-5
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        up = FT.fold(*_posterior(x + e, K)[:2], None, None, c_mean, c_std, bound).logF
        dn = FT.fold(*_posterior(x - e, K)[:2], None, None, c_mean, c_std, bound).logF
        num = (up - dn) / (2 * h)
        assert np.max(np.abs(num - f.dlogF[:, d])) <= 1e-7 * max(1.0, float(np.max(np.abs(f.dlogF[:, d]))))
    # the sum runs in index order over the constraints' own terms
    assert np.array_equal(f.logF, np.add.reduce(f.terms, axis=0)) or np.allclose(np.asarray(f.logF - f.terms.sum(0), float), 0, atol=1e-15)


def test_the_clip_and_the_far_tail():
    f = FT.fold(np.array([[0.0]]), np.array([[1e-14]]), np.array([[[1.0]]]), np.array([[[0.5]]]), [0.0], [1.0], [-45e-5])
    assert float(f.s[0, 0]) == pytest.approx(1e-5) and float(f.z[0, 0]) == pytest.approx(-45.0)
    assert np.isfinite(float(f.logF[0])) and float(f.logF[0]) < -1000 and np.exp(float(f.logF[0])) == 0.0
    assert np.isfinite(float(f.dlogF[0, 0]))


def test_the_case_table():
    assert {c.D for c in FT.TABLE} == {1, 6, 20} and {c.K for c in FT.TABLE} == {1, 3, 8}
    assert {c.M for c in FT.TABLE} == {1, 3, 4, 5, 8, 20} and {c.Mtab for c in FT.TABLE} == {1, 9, 257}
    assert {n for c in FT.TABLE for n in c.Nc} == {33, 200, 300} and {c.fam for c in FT.TABLE} == {"Mat52", "Exponential"}
    for c in FT.TABLE:
        p = FT.problem(c.id)
        assert len(p.Xc) == c.K and p.Xs.shape == (c.M, c.D) and p.Xtab.shape == (c.Mtab, c.D) and p.X.shape == (FT.N_SCORED, c.D)
        assert all(x.shape == (n, c.D) for x, n in zip(p.Xc, c.Nc))
        if c.clip:
            assert np.array_equal(p.Xs[0], p.Xc[0][7]) and p.noise[0] == 1e-12 and p.c_std[0] < 0.1
