"""CPU: the long-double truth of the Laplace probit fit (tests/_laplace_truth.py) checked against itself -- its gradient against
central differences of its own log Z, its posterior against a long-double exact GP on K + W^-1 with the pseudo-targets
f + W^-1 g (the identity the device's Laplace-fitted state rests on), its sites against closed forms at z = 0 and the asymptotics
of both tails, its log Phi against tests/_feas_truth.py -- and the float64 replica of the device's iteration on every case."""
import numpy as np
import pytest

import _feas_truth as FT
import _laplace_truth as LT

T = LT.T
PI = T("3.14159265358979323846264338327950288")
BASE = [c.id for c in LT.TABLE if not c.lookahead]


def test_log_phi_agrees_with_the_feasibility_truth():
    z = np.array([-45, -25, -20, -19.9, -10, -3, -1.5, -1.2, -0.3, 0, 0.4, 1.3, 1.5, 3, 8, 12.0], dtype=T)
    a, b = LT.log_ndtr(z), FT.log_ndtr(z)
    assert np.all(np.abs(a - b) <= T(1e-13) * np.abs(b) + T(1e-16))       # (that one takes erfc in double)


def test_sites_at_zero_and_in_both_tails():
    for y in (1.0, -1.0):
        s = LT.sites(np.array([y]), np.array([0.0]))
        n0 = np.sqrt(T(2) / PI)
        assert abs(s.logp[0] - np.log(T(0.5))) < T(1e-18)
        assert abs(s.n[0] - n0) < T(1e-18) and abs(s.g[0] - y * n0) < T(1e-18)
        assert abs(s.W[0] - T(2) / PI) < T(1e-18)
        assert abs(s.t[0] - y * (2 * n0 ** 3 - n0)) < T(1e-18)
    # far right: Phi -> 1, n -> phi(z), W -> z phi(z) (1 + O(phi)), floored at 1e-20 from z ~ 9.5 on
    for z in (7.0, 9.0):
        s = LT.sites(np.array([1.0]), np.array([z]))
        phi = np.exp(-T(z) ** 2 / 2 - LT.HALF_LOG_2PI)
        assert abs(s.n[0] / phi - 1) < T(1e-10)
        assert abs(s.W[0] / (z * phi) - 1) < T(1e-10) and s.W[0] > LT.W_FLOOR
        assert abs(s.logp[0] + phi / z * (1 - 1 / T(z) ** 2)) < 4 * phi / T(z) ** 5
    for z in (10.0, 12.0, 30.0):
        s = LT.sites(np.array([1.0, -1.0]), np.array([z, -z]))
        assert np.all(s.W == LT.W_FLOOR) and np.all(np.isfinite(s.t)) and np.all(np.isfinite(s.g))
    # far left: n = -z / (1 - 1/z^2 + 3/z^4 - 15/z^6 + ...), W -> 1, everything finite where Phi underflows
    for z in (-30.0, -45.0, -200.0):
        s = LT.sites(np.array([1.0]), np.array([z]))
        zz = T(z)
        R = 1 - 1 / zz ** 2 + 3 / zz ** 4 - 15 / zz ** 6 + 105 / zz ** 8
        # (n = exp(-z^2 / 2 - ... - log Phi): two terms of size z^2 / 2 meet, an absolute 1e-19 z^2 in the exponent)
        assert abs(s.n[0] / (-zz / R) - 1) < 1000 / zz ** 10 + T(4e-19) * zz ** 2
        assert abs(s.logp[0] - (-zz * zz / 2 - np.log(-zz) - LT.HALF_LOG_2PI + np.log(R))) < 1000 / zz ** 10 + T(4e-19) * zz ** 2
        assert abs(s.W[0] - (1 - 1 / zz ** 2)) < 20 / zz ** 4      # W = (1 - 3 / z^2 + ...) / R^2
        assert np.isfinite(s.t[0])


@pytest.mark.parametrize("cid", BASE)
def test_mode_is_stationary(cid):
    ft = LT.fit(cid)
    resid = np.abs(ft.a - LT.sites(LT.problem(cid).y, LT.matvec(ft.K, ft.a)).g).max()
    assert resid <= T(1e-16) * np.abs(ft.a).max(), (float(resid), float(np.abs(ft.a).max()))
    assert ft.iters <= LT.CAP


def test_edge_cases_are_what_the_table_says():
    assert float(LT.fit("f").W.min()) < 1e-10 and float(LT.fit("f").W.min()) == 1e-20     # separated labels reach the floor
    share = float((LT.problem("e").y > 0).mean())
    assert min(share, 1 - share) < 0.2
    X = LT.problem("d").X
    assert np.array_equal(X[5], X[3]) and np.array_equal(X[77], X[3]) and LT.problem("d").y[77] == -LT.problem("d").y[3]
    fams = {(c.fam, c.ard) for c in LT.TABLE}
    assert fams == {(f, a) for f in LT.FAMILIES for a in (False, True)}
    assert {c.N for c in LT.TABLE} >= {40, 127, 128, 129, 300} and any(c.lookahead for c in LT.TABLE)


@pytest.mark.parametrize("cid", ["a", "g", "h", "b", "d", "f"])      # every family, iso and ARD among them; N = 40 ... 300
def test_gradient_agrees_with_central_differences_of_log_z(cid):
    p = LT.problem(cid)
    c = p.case
    g = LT.gradient(cid)
    th = np.r_[c.variance, p.ls_arg].astype(T)
    for i in range(th.size):
        h = T(1e-6) * th[i]
        vals = []
        for sgn in (1, -1):
            t2 = th.copy()
            t2[i] += sgn * h
            ls = t2[1:] if c.ard else np.repeat(t2[1:], c.D)
            vals.append(LT.params_fit(c.fam, t2[0], ls, p.X, p.y).logZ)
        cd = (vals[0] - vals[1]) / (2 * h)
        # the difference quotient's own error: h^2 / 6 f''' ~ 1e-12 relative, rounding of log Z 1e-19 / 1e-6
        assert abs(cd - g[i]) <= T(1e-9) * max(abs(g[i]), 1), (i, float(cd), float(g[i]))


@pytest.mark.parametrize("cid", BASE)
def test_posterior_is_that_of_an_exact_gp_on_k_plus_w_inverse(cid):
    p = LT.problem(cid)
    c = p.case
    ft, po = LT.fit(cid), LT.posterior(cid)
    Ky = ft.K + np.diag(1 / ft.W)
    Lt = LT.chol(Ky)
    ytilde = ft.f + ft.g / ft.W
    alpha = LT.solve_upper_t(Lt, LT.solve_lower(Lt, ytilde))
    ks = LT.cov(c.fam, c.variance, p.ls, p.Xs, p.X)
    V = LT.solve_lower(Lt, ks.T)
    mean, var = ks @ alpha, T(c.variance) - (V * V).sum(0)
    # W^-1 up to 1e20 beside K ~ 1e2: the sum drops 1e-18 of K there, and alpha = a only to the conditioning of that system
    assert np.all(np.abs(mean - po.mean) <= T(1e-10) * np.maximum(1, np.abs(po.mean)))
    assert np.all(np.abs(var - po.var) <= T(1e-10) * po.var + T(1e-14))
    # diag(W^-1/2) L is the lower factor of K + W^-1
    Ltilde = ft.L / np.sqrt(ft.W)[:, None]
    assert np.abs(Ltilde @ Ltilde.T - Ky).max() <= T(1e-15) * np.abs(Ky).max()
    # and p(y = 1 | x) lies in (0, 1) with a positive propagated tolerance
    assert np.all((po.p > 0) & (po.p < 1)) and np.all(po.tol_p > 0)


@pytest.mark.parametrize("case", LT.TABLE, ids=[c.id for c in LT.TABLE])
def test_every_case_converges_within_the_cap_in_float64(case):
    r = LT.newton_f64(case.id)
    print("case %s: %d Newton steps, %d halvings in float64 (truth: %d)" % (case.id, r.iters, r.halvings, LT.fit(case.id).iters))
    assert r.converged and r.iters <= LT.CAP
    assert r.iters <= 16        # 5 ... 12 observed; well inside the cap of 40
    ft = LT.fit(case.id)
    assert abs(r.logZ - float(ft.logZ)) <= 1e-10 * abs(float(ft.logZ))
    assert np.abs(r.a - np.asarray(ft.a, float)).max() <= 1e-8 * float(np.abs(ft.a).max())
