"""Host side of the input-warped GP (no GPU): the Kumaraswamy warping function against its closed form and against central
differences, its validation errors, the log-Gaussian prior, the warping indices of a design space, and the BO surface's
``model_type='input_warped_GP'`` (construction only: nothing here touches the device).

Reference: GPy/GPy/util/input_warping_functions.py:60-258, GPy/GPy/core/parameterization/priors.py:142-182,
GPyOpt/GPyOpt/models/input_warped_gpmodel.py:47-57, GPyOpt/GPyOpt/util/arguments_manager.py:32-34,137-147.
"""
import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd.bayesian_optimization import InvalidConfigError
from gaussian_process_optimization_amd.input_warped_gp import warping_indices_of
from gaussian_process_optimization_amd.input_warping import KumarWarping, LogGaussian

EPS = 1e-6
A, B = (0.6, 1.7, 3.0), (2.2, 0.8, 0.4)


def _data(n=40, d=3, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 2.0, (n, d))
    X[0], X[1] = -1.0, 2.0           # the extremes: u = eps-scale and 1 - eps-scale
    return X


def _warp(X, idx=None, **kw):
    w = KumarWarping(X, idx, **kw)
    for (pa, pb), a, b in zip(w.params, A, B):
        pa.set(a)
        pb.set(b)
    return w


def _closed_form(X, lo, hi, cols):
    out = X.copy()
    for k, q in enumerate(cols):
        u = (X[:, q] - (lo[q] - EPS)) / ((hi[q] + EPS) - (lo[q] - EPS))
        out[:, q] = 1 - (1 - u ** A[k]) ** B[k]
    return out


def test_f_is_the_closed_form_on_the_warped_columns_only():
    X = _data()
    w = _warp(X, [0, 2])
    got = w.f(X)
    ref = _closed_form(X, X.min(0), X.max(0), [0, 2])
    assert np.array_equal(got[:, 1], X[:, 1])
    assert np.max(np.abs(got - ref)) <= 1e-14
    assert np.all((got[:, [0, 2]] > 0) & (got[:, [0, 2]] < 1))
    # test data are normalised with the training bounds; outside them a fractional power of a negative number is NaN
    Xt = np.array([[0.5, 0.1, 0.2], [-1.5, 0.0, 0.0]])
    gt = w.f(Xt, test_data=True)
    assert np.max(np.abs(gt[0] - _closed_form(Xt, X.min(0), X.max(0), [0, 2])[0])) <= 1e-14
    assert np.isnan(gt[1, 0])
    # the identity at a = b = 1 (normalised)
    w1 = KumarWarping(X)
    assert np.max(np.abs(w1.f(X) - (X - w1.Xmin) / (w1.Xmax - w1.Xmin))) <= 1e-15


def test_user_bounds_and_set_X():
    X = _data()
    lo, hi = np.full(3, -2.0), np.full(3, 3.0)
    w = _warp(X, None, Xmin=lo, Xmax=hi)
    assert np.max(np.abs(w.f(X) - _closed_form(X, lo, hi, [0, 1, 2]))) <= 1e-14
    X2 = _data(seed=8)[:11]
    w.set_X(X2)
    assert np.max(np.abs(w.f(X2) - _closed_form(X2, lo, hi, [0, 1, 2]))) <= 1e-14
    assert np.max(np.abs(w.f(X2) - w.f(X2, test_data=True))) == 0.0


def test_fgrad_X_against_central_differences():
    X = _data()[2:]                   # (the extremes sit on the edge of the domain: no room for a step)
    w = _warp(_data(), [0, 2])
    h = 1e-6
    for test_data, W in ((True, w), (False, _warp(X, [0, 2], Xmin=_data().min(0), Xmax=_data().max(0)))):
        g = W.fgrad_X(X, test_data=test_data)
        assert np.all(g[:, 1] == 0.0)
        for q in (0, 2):
            e = np.zeros(3)
            e[q] = h
            num = (W.f(X + e, test_data=True)[:, q] - W.f(X - e, test_data=True)[:, q]) / (2 * h)
            err = np.max(np.abs(g[:, q] - num) / np.maximum(np.abs(num), 1.0))
            print("fgrad_X column %d (test_data=%s): %.2e" % (q, test_data, err))
            assert err <= 1e-6


def test_update_grads_against_central_differences():
    X = _data()
    rng = np.random.default_rng(3)
    dL_dW = rng.standard_normal(X.shape)
    w = _warp(X, [0, 2])
    w.update_grads(X, dL_dW)
    h = 1e-6
    for k in range(2):
        for j in range(2):
            p = w.params[k][j]
            v = float(p)
            p.set(v + h)
            fp = np.sum(dL_dW * w.f(X))
            p.set(v - h)
            fm = np.sum(dL_dW * w.f(X))
            p.set(v)
            num = (fp - fm) / (2 * h)
            print("d/d%s: analytic %.9e numeric %.9e" % (p.name, p.gradient[0], num))
            assert abs(p.gradient[0] - num) <= 1e-6 * max(abs(num), 1.0)


def test_parameters_bounds_priors_and_order():
    w = KumarWarping(_data(), [2, 0])
    assert w.warping_dim == 2 and w.num_parameters == 4 and w.epsilon == 1e-6
    ps = w.flattened_parameters()
    assert [p.name for p in ps] == ["a0", "b0", "a1", "b1"]
    for p in ps:
        assert float(p) == 1.0
        assert (p.transform.lower, p.transform.upper) == (0.0, 10.0)
        assert (p.prior.mu, p.prior.sigma) == (0.0, 0.75)
    warp, a, b, lo, hi = _warp(_data(), [2, 0]).device_arguments(3)
    assert warp.tolist() == [1, 0, 1] and a.tolist() == [A[1], 1.0, A[0]] and b.tolist() == [B[1], 1.0, B[0]]
    assert np.array_equal(lo, _data().min(0) - 1e-6) and np.array_equal(hi, _data().max(0) + 1e-6)


def test_validation_errors():
    X = _data()
    with pytest.raises(ValueError, match="exceed feature dimension"):
        KumarWarping(X, [0, 3])
    with pytest.raises(ValueError, match="larger than 0"):
        KumarWarping(X, [-1, 1])
    with pytest.raises(ValueError, match="should be integer"):
        KumarWarping(X, [0, 1.0])
    with pytest.raises(ValueError, match="at the same time"):
        KumarWarping(X, None, Xmin=[0, 0, 0])
    with pytest.raises(ValueError, match="n_feature values"):
        KumarWarping(X, None, Xmin=[0, 0], Xmax=[1, 1])


def test_log_gaussian():
    p = LogGaussian(0.3, 0.75)
    x = np.array([0.05, 0.7, 1.0, 4.2, 9.9])
    ref = -0.5 * np.log(2 * np.pi * 0.75 ** 2) - 0.5 * (np.log(x) - 0.3) ** 2 / 0.75 ** 2 - np.log(x)
    assert np.max(np.abs(p.lnpdf(x) - ref)) <= 1e-15
    h = 1e-6
    num = (p.lnpdf(x + h) - p.lnpdf(x - h)) / (2 * h)
    assert np.max(np.abs(p.lnpdf_grad(x) - num) / np.maximum(np.abs(num), 1.0)) <= 1e-7
    # a density on the positive reals: it integrates to one
    grid = np.exp(np.linspace(-12, 12, 200001))
    dens = np.exp(p.lnpdf(grid))
    assert abs(np.sum(0.5 * (dens[1:] + dens[:-1]) * np.diff(grid)) - 1.0) <= 1e-6


DOMAIN = [{'name': 'x', 'type': 'continuous', 'domain': (0.0, 1.0), 'dimensionality': 2},
          {'name': 'k', 'type': 'discrete', 'domain': (1, 2, 4, 8)},
          {'name': 'y', 'type': 'continuous', 'domain': (-3.0, 5.0)}]


def test_warping_indices_of_a_mixed_space():
    space = gpo.Design_space(DOMAIN)
    assert warping_indices_of(space) == [0, 1, 2, 3]
    m = gpo.models.InputWarpedGPModel(space)
    assert m.warping_indices == [0, 1, 2, 3] and m.analytical_gradient_prediction and not isinstance(m, gpo.GPModel)

    class _Var(object):
        def __init__(self, type_, dimensionality):
            self.type, self.dimensionality = type_, dimensionality

    class _Space(object):     # the reference's layout: space.space holds variables with a type and a dimensionality
        space = [_Var('continuous', 2), _Var('categorical', 3), _Var('discrete', 1), _Var('bandit', 2), _Var('continuous', 1)]
    assert warping_indices_of(_Space()) == [0, 1, 5, 8]


def _xy(n=6):
    rng = np.random.default_rng(0)
    X = np.c_[rng.uniform(0, 1, (n, 2)), rng.choice([1., 2., 4., 8.], n), rng.uniform(-3, 5, n)]
    return X, rng.standard_normal((n, 1))


def test_model_type_input_warped_GP_constructs(capsys):
    X, Y = _xy()
    bo = gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model_type='input_warped_GP', exact_feval=True, ARD=True,
                                  max_iters=17, optimize_restarts=2, noise_var=0.3, kernel='Matern32')
    m = bo.model
    assert isinstance(m, gpo.models.InputWarpedGPModel) and not isinstance(m, gpo.GPModel)
    assert (m.exact_feval, m.ARD, m.max_iters, m.optimize_restarts, m.noise_var, m.optimizer) == (True, True, 17, 2, 0.3, 'lbfgs')
    assert isinstance(m.kernel, gpo.kern.Matern32) and m.kernel.ARD
    assert m.space is bo.space and m.warping_indices == [0, 1, 2, 3] and m.model is None
    assert not bo.acquisition._device_ok()
    assert capsys.readouterr().out == ""
    gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model_type='input_warped_GP',
                             input_warping_function_type='something_else')
    assert "Only support kumar_warping for input!" in capsys.readouterr().out
    # batches without the penaliser are fine
    gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model_type='input_warped_GP', evaluator_type='thompson_sampling',
                             batch_size=3)
    gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model_type='input_warped_GP', evaluator_type='local_penalization',
                             batch_size=1)


def test_local_penalization_refuses_the_input_warped_model():
    X, Y = _xy()
    with pytest.raises(InvalidConfigError, match="local_penalization evaluator can only be used with GP models"):
        gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model_type='input_warped_GP',
                                 evaluator_type='local_penalization', batch_size=2)


@pytest.mark.parametrize("model_type", ["sparseGP", "GP_MCMC", "warpedGP", "RF", "nonsense"])
def test_other_model_types_still_raise(model_type):
    X, Y = _xy()
    with pytest.raises(NotImplementedError, match="outside the accelerated path"):
        gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model_type=model_type)
