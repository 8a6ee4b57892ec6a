"""CPU: the long-double truth of max-value entropy search (tests/_mes_truth.py) against fixed values and central differences, the
Gumbel fit's closed form, ``max_value.MinValueSampler`` over a device-free model against a direct bisection, and the host rule
``acquisitions._MaxValueEntropy``."""
import types

import numpy as np
import pytest
from scipy.special import log_ndtr

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import max_value
from gaussian_process_optimization_amd.acquisitions import _RULES
from oracle import cpu_ref as O

import _feas_truth as FT
import _mes_truth as MT

T = MT.T


# h and h' from 50-digit arithmetic, checked there against numerical differentiation
FIXED = ((0.0, np.log(2.0), -0.398942280401), (3.0, 0.00800756852794, -0.0222187368337),
         (-25.0, 3.6409953573, -0.0397470244087), (8.0, 2.08311803916e-14, -1.64198810215e-13))


@pytest.mark.parametrize("g,h,hp", FIXED)
def test_truth_reproduces_the_fixed_values(g, h, hp):
    assert abs(float(MT.h(T(g))) - h) <= 2e-12 * abs(h)
    assert abs(float(MT.hprime(T(g))) - hp) <= 2e-12 * abs(hp)


def test_log_ndtr_agrees_with_the_feasibility_truth_and_with_itself_across_its_branches():
    z = np.array([-30.0, -20.5, -19.9, -12.0, -5.0, -2.9, -2.7, 0.0, 1.0, 2.7, 2.9, 7.0, 12.0], dtype=T)
    a, b = MT.log_ndtr(z), FT.log_ndtr(z)
    # (_feas_truth's erfc is SciPy's, in double: its argument's rounding times z^2, and erfc's own few ulp)
    assert np.all(np.abs(a - b) <= (z * z + 16) * 2.0 ** -52)
    # the series (at and below -20) against the continued fraction just above it; the Maclaurin series against the fraction at
    # erfc's own switch (x = 1, z = sqrt 2)
    assert abs(float(MT.log_ndtr(T(-20) + T(1e-15)) - FT._series(T(-20) + T(1e-15)))) < 1e-16
    x = np.array([1.0], dtype=T)
    lo, hi = MT.erfc_ld(x - T(1e-18)), MT.erfc_ld(x)
    assert abs(float((lo - hi)[0] / hi[0])) < 1e-17          # (erfc' / erfc = -2.6 there: 1e-18 apart moves it by 3e-18)


@pytest.mark.parametrize("g", [-40.0, -25.0, -20.0, -12.0, -11.0, -5.0, -1.0, 0.0, 0.5, 3.0, 6.0, 8.0, 12.0])
def test_derivatives_against_long_double_central_differences(g):
    e = T(2.0) ** -14
    g = T(g) + T(1e-3)               # (clear of the branch points themselves: those are the next test)
    d1 = (MT.h(g + e) - MT.h(g - e)) / (2 * e)
    d2 = (MT.hprime(g + e) - MT.hprime(g - e)) / (2 * e)
    # truncation e^2 |f'''| / (6 |f'|) ~ 4e-9 x O(1); just above the truth's own switch at -12 the three-term forms lose g^4 / 4
    # = 5e3 long-double ulp (5e-16), which the difference quotient divides by 2 e |f'| ~ 1e-5 ... 1e-6
    assert abs(float(d1 / MT.hprime(g)) - 1.0) < 1e-7
    # (h'' changes sign next to 0: on the scale of h' there)
    assert abs(float(d2 - MT.hsecond(g))) < 1e-7 * max(abs(float(MT.hsecond(g))), abs(float(MT.hprime(g))))


@pytest.mark.parametrize("at", [-20.0, -12.0, 6.0, -np.sqrt(2.0), np.sqrt(2.0)])
def test_continuity_across_the_branch_points(at):
    """-20 and 6: where the device's log Phi (and, at -20, its B) change branch; -12: where the truth's B does; +-sqrt 2: where
    the truth's erfc does.  Either side of each, one long-double ulp of the argument apart, the values agree to rounding."""
    e = abs(T(at)) * T(2.0) ** -62
    for f, rel in ((MT.h, 1e-15), (MT.hprime, 1e-13)):
        a, b = f(T(at) - e), f(T(at) + e)
        assert abs(float((a - b) / b)) < rel, (f.__name__, float(a), float(b))


def test_score_sums_in_index_order_and_bounds_are_sane():
    rng = np.random.default_rng(1)
    mean, var = rng.standard_normal(5), rng.uniform(0.01, 1.0, 5)
    dm, dv = rng.standard_normal((5, 3)), rng.standard_normal((5, 3))
    ystar = np.array([-2.5, -2.0, -3.0])
    f = MT.score(mean, var, dm, dv, ystar, 0.3, 1.7)
    m, s = mean * 1.7 + 0.3, np.sqrt(var) * 1.7
    g = (m[None, :] - ystar[:, None]) / s[None, :]
    lam = np.exp(-g * g / 2 - 0.5 * np.log(2 * np.pi) - log_ndtr(g))
    alpha = (g * lam / 2 - log_ndtr(g)).mean(0)
    assert np.max(np.abs(f.alpha.astype(float) - alpha)) < 1e-13
    hp = -(lam / 2) * (1 + g * g + g * lam)
    want = (hp.mean(0) / s)[:, None] * 1.7 * dm - ((hp * g).mean(0) / s)[:, None] * (1.7 ** 2 / (2 * s))[:, None] * dv
    assert np.max(np.abs(f.dalpha.astype(float) - want)) < 1e-12
    assert np.all(f.bound_alpha > 0) and np.all(f.bound_alpha < 1e-12) and np.all(f.bound_dalpha < 1e-11)
    # the series keeps the derived relative bound on h' at g = -25 far below 1e-9; the three-term bracket would not
    one = MT.score(np.array([0.0]), np.array([1.0]), np.array([[1.0]]), np.array([[0.0]]), np.array([25.0]), 0.0, 1.0)
    assert float(one.g[0, 0]) == -25.0
    rel = float(one.bound_dalpha[0, 0] / abs(one.dalpha[0, 0]))
    print("MES truth: derived relative bound on h' at g = -25 with the series: %.3g" % rel)
    assert rel < 1e-11
    el = 3600 * 2.0 ** -53
    assert (4 * 2.0 ** -53 * (1 + 625 + 626) + 626 * el) / (2.0 / 625) > 1e-9


def test_propagation_is_the_first_order_move():
    rng = np.random.default_rng(2)
    mean, var = rng.standard_normal(4), rng.uniform(0.05, 1.0, 4)
    dm, dv = rng.standard_normal((4, 2)), 0.1 * rng.standard_normal((4, 2))
    ystar = np.array([-1.5, -2.0])
    f = MT.score(mean, var, dm, dv, ystar, 0.0, 1.0)
    eps = 1e-7
    sd = np.sqrt(var)
    g = MT.score(mean + eps, (sd * (1 + eps)) ** 2, dm + eps, dv + eps, ystar, 0.0, 1.0)
    tl, td = MT.propagate(f, 1.0, np.full(4, eps), eps * sd, np.full((4, 2), eps), np.full((4, 2), eps))
    assert np.all(np.abs(g.alpha - f.alpha) <= tl * (1 + 1e-4)) and np.all(np.abs(g.alpha - f.alpha) >= 1e-3 * tl)
    assert np.all(np.abs(g.dalpha - f.dalpha) <= td * (1 + 1e-4))


def test_gumbel_fit_closed_form():
    a, b = -4.0, 0.3
    y = {q: a + b * np.log(-np.log(1 - q)) for q in MT.QUANTILES}
    for fit in (MT.gumbel_fit, max_value.gumbel_fit):
        a1, b1 = fit(y[0.25], y[0.5], y[0.75])
        assert abs(a1 - a) < 1e-14 and abs(b1 - b) < 1e-14
    u = np.random.RandomState(4).uniform(size=6)
    s = MT.gumbel_samples(a, b, 6, 4, -4.1)
    assert np.array_equal(s, np.minimum(a + b * np.log(-np.log(u)), -4.1)) and np.all(s <= -4.1) and np.any(s < -4.1)


# ---- the sampler and the class over a device-free model ------------------------------------------------------------------------------
class _HostModel(gpo.GPModel):
    """GPModel's prediction contract answered by the oracle on the host; ``sparse`` keeps every acquisition off the device."""

    def __init__(self, noise=1e-2):
        super().__init__(max_iters=0, verbose=False)
        self.sparse, self.noise, self.model, self.fits = True, noise, None, 0

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        self.fits += 1
        self.gp = O.OracleGP(np.asarray(X_all, dtype=float), np.asarray(Y_all, dtype=float),
                             O.make_kernel("Mat52", X_all.shape[1], 1.0, 0.5), noise_var=self.noise)
        self.om = O.OracleGPModel(self.gp)
        self.model = types.SimpleNamespace(output_dim=1, normalizer=None, _data_epoch=self.fits, param_array=np.array([1.0, 0.5]),
                                           X=self.gp.X, Y=self.gp.Y)

    def predict(self, X, with_noise=True):
        return self.om.predict(np.atleast_2d(X), with_noise)

    def predict_withGradients(self, X):
        return self.om.predict_withGradients(np.atleast_2d(X))

    def get_fmin(self):
        return self.om.get_fmin()


def _host_problem(N=20):
    rng = np.random.RandomState(2)
    X = rng.uniform(0, 1, (N, 2))
    Y = np.sin(4 * X[:, :1]) + np.cos(3 * X[:, 1:])
    gm = _HostModel()
    gm.updateModel(X, Y, None, None)
    space = gpo.Design_space([{"name": "v%d" % i, "type": "continuous", "domain": (0.0, 1.0)} for i in range(2)])
    return gm, space, X, Y


def test_sampler_against_a_direct_bisection_and_the_clip():
    gm, space, X, Y = _host_problem()
    smp = max_value.MinValueSampler(gm, space, num_samples=12, grid_size=300, seed=7)
    np.random.seed(1)
    table = smp.table()
    assert table.shape == (320, 2) and np.array_equal(table[300:], X)
    ystar = smp.sample(table)
    assert not smp.last_on_device and smp.last_latent and ystar.shape == (12,)
    mu, sd = gm.predict(table, with_noise=False)          # the host sums take the latent posterior where the model offers it
    mu, sd = mu[:, 0], sd[:, 0]
    lo0, hi0 = smp.last_first
    assert lo0 == np.min(mu - 8 * sd) and hi0 == np.min(mu + 8 * sd)
    for q in max_value.QUANTILES:
        lo, hi = smp.last_brackets[q]
        assert 0 < hi - lo <= 1e-9 * (hi0 - lo0)
        a, b = lo0, hi0                      # the direct bisection on the same sums
        for _ in range(80):
            mid = 0.5 * (a + b)
            if log_ndtr((mu - mid) / sd).sum() >= np.log1p(-q):
                a = mid
            else:
                b = mid
        assert lo - 1e-12 <= 0.5 * (a + b) <= hi + 1e-12
        yq = float(MT.quantile(mu, sd ** 2, 0.0, 1.0, q))
        assert lo - 1e-10 <= yq <= hi + 1e-10
    fit = max_value.gumbel_fit(*[smp.last_quantiles[q] for q in max_value.QUANTILES])
    assert fit == smp.last_fit and fit[1] > 0
    fmin = gm.get_fmin()
    assert np.array_equal(ystar, MT.gumbel_samples(fit[0], fit[1], 12, 7, fmin)) and np.all(ystar <= fmin)
    # a Gumbel law placed high above the incumbent: every sample is the incumbent
    high = max_value.MinValueSampler(gm, space, num_samples=5, grid_size=10, seed=1)
    high.brackets = lambda table=None: {0.25: (9.0, 9.0), 0.5: (10.0, 10.0), 0.75: (11.0, 11.0)}
    assert np.array_equal(high.sample(), np.full(5, fmin))
    # the fitted law describes the minimum: its quartiles against 4000 joint draws of independent marginals
    draws = (mu[None, :] + sd[None, :] * np.random.RandomState(0).standard_normal((4000, mu.size))).min(axis=1)
    for q in max_value.QUANTILES:
        assert abs(smp.last_quantiles[q] - np.quantile(draws, q)) < 0.1 * (hi0 - lo0) / 16
    # a foreign model whose predict takes the locations alone: its own (noisy) prediction, in blocks of rows
    foreign = types.SimpleNamespace(predict=lambda X: gm.predict(X), get_fmin=gm.get_fmin)
    fs = max_value.MinValueSampler(foreign, space, num_samples=3, grid_size=10, seed=1)
    old_rows, max_value._HOST_ROWS = max_value._HOST_ROWS, 64
    try:
        fs.sample(table)
    finally:
        max_value._HOST_ROWS = old_rows
    assert not fs.last_latent and not fs.last_on_device
    nm, ns = gm.predict(table)
    for q in max_value.QUANTILES:
        lo, hi = fs.last_brackets[q]
        assert log_ndtr((nm[:, 0] - lo) / ns[:, 0]).sum() >= np.log1p(-q) - 1e-9 > log_ndtr((nm[:, 0] - hi) / ns[:, 0]).sum() - 2e-9
    assert fs.last_quantiles[0.5] < smp.last_quantiles[0.5]          # the noise spreads the law of the minimum downwards
    with pytest.raises(ValueError):
        max_value.MinValueSampler(gm, space, num_samples=65)
    with pytest.raises(ValueError):
        max_value.MinValueSampler(gm, space, grid_size=0)


def test_samples_are_redrawn_on_a_changed_fit_only():
    gm, space, X, Y = _host_problem()
    acq = gpo.AcquisitionMES(gm, space, num_samples=6, grid_size=200, seed=3)
    assert acq._route() is None and acq.analytical_gradient_acq and acq._fmin() == 0.0
    Xs = np.random.RandomState(5).uniform(0, 1, (7, 2))
    np.random.seed(2)
    a = acq.acquisition_function(Xs)
    y0 = acq.ystar.copy()
    acq.acquisition_function_withGradients(Xs[:2])
    acq.acquisition_function(Xs[:3])
    assert acq.draws == 1 and np.array_equal(acq.ystar, y0) and a.shape == (7, 1)
    assert np.all(a <= 0.0) and np.all(y0 <= gm.get_fmin())
    gm.updateModel(X, Y + 0.3 * X[:, :1], None, None)
    acq.acquisition_function(Xs[:3])
    assert acq.draws == 2 and not np.array_equal(acq.ystar, y0)
    acq.acquisition_function(Xs[:3])
    assert acq.draws == 2
    # the scores are the rule over the model's predictions and the resident samples, negated
    mu, sd = gm.predict(Xs)
    want = _RULES["MES"].value(acq.ystar, 0.0, mu, sd)
    assert np.array_equal(acq.acquisition_function(Xs), -want)
    t = MT.score(mu[:, 0], sd[:, 0] ** 2, None, None, acq.ystar, 0.0, 1.0)
    assert np.max(np.abs(want[:, 0] - t.alpha.astype(float))) < 1e-12
    assert acq.argbest(Xs) == (int(np.argmax(want)), float(-want.max()))


def test_host_rule_gradient_against_finite_differences():
    rule = _RULES["MES"]
    assert rule.device_id == gpo._lib.GP_ACQ_MES and rule.needs_fmin is False
    ystar = np.array([-1.0, -0.4, 0.3])
    mu = np.array([[0.2], [-0.9], [5.0], [-8.0], [0.0]])
    sd = np.array([[0.5], [0.05], [0.3], [0.25], [0.03]])      # g from about -33 (the series) to +20
    dmu, dsd = np.array([[1.0, -2.0]] * 5), np.array([[0.3, 0.1]] * 5)
    val, grad = rule.gradient(ystar, 0.0, mu, sd, dmu, dsd)
    assert val.shape == (5, 1) and grad.shape == (5, 2) and np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    t = MT.score(mu[:, 0], sd[:, 0] ** 2, dmu, 2 * sd * dsd, ystar, 0.0, 1.0)
    # (in double h loses g^2 / 2 times the few thousand u of lambda: 1e-10 at g = -33)
    assert np.all(np.abs(val[:, 0] - t.alpha.astype(float)) <= 1e-8 * np.abs(val[:, 0]) + 1e-300)
    assert np.all(np.abs(grad - t.dalpha.astype(float)) <= 1e-8 * np.abs(grad).max(axis=1, keepdims=True) + 1e-300)
    eps = 1e-6
    for d in range(2):
        up = rule.value(ystar, 0.0, mu + eps * dmu[:, d:d + 1], sd + eps * dsd[:, d:d + 1])
        dn = rule.value(ystar, 0.0, mu - eps * dmu[:, d:d + 1], sd - eps * dsd[:, d:d + 1])
        fd = (up - dn)[:, 0] / (2 * eps)
        assert np.all(np.abs(fd - grad[:, d]) <= 2e-5 * np.abs(grad[:, d]) + 1e-12), (d, fd, grad[:, d])
    # far out on the improving side h underflows towards 0 and stays finite, with a finite gradient
    v, g = rule.gradient(np.array([0.0]), 0.0, np.array([[40.0]]), np.array([[1.0]]), np.array([[1.0]]), np.array([[1.0]]))
    assert v[0, 0] >= 0.0 and v[0, 0] < 1e-300 and np.isfinite(g).all()
