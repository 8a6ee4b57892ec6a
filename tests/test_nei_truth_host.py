"""CPU: noisy expected improvement's truth (tests/_nei_truth.py) held to what does not depend on it -- central differences of its
value, the closed-form moments of the fantasies, the reference's EI on a model of each fantasy -- and the conditions every case of
the table must satisfy so that the GPU tests test something: substantial NEI, and a model much noisier than its twin."""
import numpy as np
import pytest

import _nei_truth as NT
from oracle import cpu_ref as O

T = NT.T
CASE_IDS = [c.id for c in NT.TABLE]


@pytest.mark.parametrize("cid", CASE_IDS)
def test_conditions(cid):
    sv = NT.truth(cid)
    c = sv.p.case
    share, share_grad, ratio = NT.conditions(sv)
    v = np.asarray(sv.truth.value, dtype=float)
    print("nei conditions[%s]: share of locations with NEI >= 1000 allowances %.2f (gradient rows %.2f); (d - d0) / d0 = %.1f; NEI "
          "median %.3e, max %.3e; floored locations %d" % (cid, share, share_grad, ratio, np.median(v), v.max(), int(sv.truth.floored.sum())))
    assert share >= 0.5 and share_grad >= 0.5
    assert ratio >= NT.NOISE_RATIO
    assert sv.truth.value.shape == (c.Mt,) and sv.truth.grad.shape == (c.Mr, c.D)
    assert sv.truth.F.shape == (c.S, c.N) and sv.truth.fstar.shape == (c.S,) and sv.truth.p.shape == (c.Mt, c.S)
    assert np.all(v >= 0.0) and np.all(np.isfinite(v)) and np.all(np.isfinite(np.asarray(sv.truth.grad, dtype=float)))
    assert np.all(sv.allowance > 0) and sv.tol_F == NT.rel_tol(c.noise) * max(1.0, float(np.max(np.abs(sv.truth.F))))


def test_the_special_locations_are_what_they_claim():
    d, e = NT.truth("d"), NT.truth("e")
    assert np.array_equal(d.p.Xs[2], d.p.X[17]) and not d.truth.floored[2] and d.p.case.Mr > 2      # on a training input, above the floor at y_std 1.7
    assert np.array_equal(e.p.Xs[2], e.p.X[17]) and e.truth.floored[2] and e.truth.floored.sum() == 1 and e.p.case.Mr > 2
    assert float(e.truth.s[2]) == 1e-5                                            # the floor's standard deviation
    assert {c.S for c in NT.TABLE} == {1, 16, 17, 64} and {c.N for c in NT.TABLE} == {130, 300, 1100}
    assert {c.fam for c in NT.TABLE} == set(NT.FAMILY_ID) and {c.Mr for c in NT.TABLE} == {1, 4, 8}
    assert max(c.Mr * c.D for c in NT.TABLE) == 128


@pytest.mark.parametrize("cid", ["b", "e"])
def test_truth_gradient_against_central_differences(cid):
    sv = NT.truth(cid)
    c, p = sv.p.case, sv.p
    h = 1e-6
    pts = []
    for m in range(c.Mr):
        for d in range(c.D):
            for sgn in (+1, -1):
                x = np.asarray(p.Xs[m], dtype=T).copy()
                x[d] += sgn * T(h)
                pts.append(x)
    v = NT.evaluate(c.fam, NT.VARIANCE, c.twin_noise, sv.fan, np.array(pts, dtype=T), 0, par=c.par, y_std=c.y_std).value.reshape(c.Mr, c.D, 2)
    num = (v[:, :, 0] - v[:, :, 1]) / (2 * T(h))
    g = sv.truth.grad
    scale = float(np.max(np.abs(g)))
    err = float(np.max(np.abs(num - g)))
    print("nei central differences[%s]: max |g| %.3e  max |difference quotient - gradient| %.3e" % (cid, scale, err))
    # the quotient's own error: h^2 / 6 |f'''| ~ 1e-12 |g| / l^2 at lengthscales ~ 0.05 .. 0.5 (the Exponential's kink lies ON a
    # training input, which no gradient row of case b is), and rounding 1e-19 NEI / h
    assert err <= 1e-6 * scale
    if cid == "e":      # the floored location: s is constant there, the means still move
        assert sv.truth.floored[2] and float(np.max(np.abs(num[2] - g[2]))) <= 1e-6 * scale


def test_fantasies_have_the_posterior_moments():
    """N = 40, 10^5 draws in float64: the sample mean and covariance of F match K0 Ky^-1 y and K0 - K0 Ky^-1 K0 within five
    Monte-Carlo standard errors, computed here from the closed-form covariance."""
    rng = np.random.default_rng(5)
    N, D, S = 40, 2, 100_000
    X = rng.uniform(0, 1, (N, D))
    y = NT.response(X) + 0.3 * rng.standard_normal(N)
    y = (y - y.mean()) / y.std()
    ls = np.full(D, 0.25)
    noise, twin = 4e-2, 1e-6
    d, d0 = NT.sigma2(noise), NT.sigma2(twin)
    fa = NT.fantasies("Mat52", NT.VARIANCE, ls, d, d0, X, y, rng.standard_normal((S, N)), rng.standard_normal((S, N)), np.float64)
    F = fa.F                                                              # [N, S]
    K0, Ky = fa.fit0.L @ fa.fit0.L.T, fa.fit.L @ fa.fit.L.T
    mean = K0 @ np.linalg.solve(Ky, y)
    cov = K0 - K0 @ np.linalg.solve(Ky, K0)
    var = np.diag(cov)
    se_mean = np.sqrt(var / S)
    se_cov = np.sqrt((np.outer(var, var) + cov * cov) / S)               # Var of a Gaussian sample covariance entry
    m_hat = F.mean(1)
    c_hat = (F - m_hat[:, None]) @ (F - m_hat[:, None]).T / (S - 1)
    r_mean, r_cov = float(np.max(np.abs(m_hat - mean) / se_mean)), float(np.max(np.abs(c_hat - cov) / se_cov))
    print("nei fantasies' moments: worst |mean error| / se = %.2f   worst |covariance error| / se = %.2f   (scale of the covariance %.1e)"
          % (r_mean, r_cov, float(var.max())))
    assert r_mean <= 5.0 and r_cov <= 5.0
    assert np.array_equal(fa.fstar, F.min(0))


def test_pin_to_the_reference_ei():
    """NEI is the mean over s of the reference's EI on a model of (X, F_s) at the twin's noise with f_min = fstar_s (normaliser
    (0, 1): the oracle's GP carries no constant).  Case c: the reference's RBF with ARD."""
    sv = NT.truth("c")
    c, p = sv.p.case, sv.p
    tr = NT.evaluate(c.fam, NT.VARIANCE, c.twin_noise, sv.fan, p.Xs, 0, par=c.par, y_mean=0.0, y_std=1.0)
    allow = NT.allowance(c._replace(y_std=1.0), tr, y_mean=0.0)
    kern = O.make_kernel("rbf", c.D, NT.VARIANCE, p.ls_arg, ARD=True)
    F = np.asarray(sv.fan.F, dtype=float)
    total = np.zeros(c.Mt)
    for s in range(c.S):
        gp = O.OracleGP(p.X, F[:, s:s + 1], kern, c.twin_noise)
        total += O.acq_EI(O.OracleGPModel(gp), p.Xs, c.par, fmin=float(sv.fan.fstar[s]))[:, 0]
    ratio = np.abs(total / c.S - np.asarray(tr.value, dtype=float)) / allow
    print("nei pin to the reference's EI[c]: worst |mean of EI - NEI| / allowance = %.3e" % float(ratio.max()))
    assert np.all(ratio <= 1.0)


def test_a_model_no_noisier_than_its_twin_is_refused():
    p = NT.problem("a")
    for d, d0 in ((NT.sigma2(1e-6), NT.sigma2(1e-6)), (NT.sigma2(1e-7), NT.sigma2(1e-6))):
        with pytest.raises(ValueError, match="d > d0"):
            NT.fantasies("Mat52", NT.VARIANCE, p.ls, d, d0, p.X, p.Y, p.Z[:1], p.E[:1], np.float64)
