"""CPU: the host side of GP classification -- label validation and the constructor's refusals, the bookkeeping of
``FeasibilityModel(kinds=...)`` (feasible, violation, no standardisation of a binary column), the NumPy fold of a binary column
against the long-double truth, and the argument checks of ``BayesianOptimization(constraint_kinds=...)``.  No GPU: every refusal
comes before a handle is created, and the constraint models are stand-ins fed the truth's posterior."""
import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib

import _laplace_truth as LT

X4 = np.array([[0.1, 0.2], [0.3, 0.9], [0.7, 0.4], [0.8, 0.8]])
Y4 = np.array([[0.0], [1.0], [1.0], [0.0]])


def test_symbols_and_namespace():
    names = {n for n, _, _ in _lib.SIGNATURES}
    assert {"gp_laplace_fit", "gp_laplace_fit_grad", "gp_laplace_info", "gp_laplace_get_mode"} <= names
    assert gpo.models.GPClassification is gpo.GPClassification and gpo.models.GPClassModel is gpo.GPClassModel
    assert _lib.LAPLACE_MAX_ITER == 40 and _lib.GP_LAPLACE_NOT_CONVERGED > 0


def test_label_validation():
    with pytest.raises(ValueError, match="0 or 1"):
        gpo.GPClassification(X4, np.array([[0.0], [1.0], [2.0], [0.0]]))
    with pytest.raises(ValueError, match="0 or 1"):
        gpo.GPClassification(X4, np.array([[-1.0], [1.0], [1.0], [-1.0]]))
    with pytest.raises(ValueError, match="0 or 1"):
        gpo.GPClassification(X4, np.array([[0.0], [np.nan], [1.0], [0.0]]))
    with pytest.raises(NotImplementedError, match="one column"):
        gpo.GPClassification(X4, np.hstack([Y4, Y4]))


def test_constructor_refusals():
    with pytest.raises(NotImplementedError, match="expectation propagation"):
        gpo.GPClassification(X4, Y4, inference_method='EP')
    with pytest.raises(NotImplementedError, match="mean function"):
        gpo.GPClassification(X4, Y4, mean_function=gpo.mappings.Constant(2, 1))
    with pytest.raises(NotImplementedError, match="normaliser"):
        gpo.GPClassification(X4, Y4, normalizer=True)
    k = gpo.kern.RBF(2)
    k.Gower = True
    with pytest.raises(NotImplementedError, match="Gower"):
        gpo.GPClassification(X4, Y4, kernel=k)
    with pytest.raises(TypeError):
        gpo.GPClassification(X4, Y4, kernel="rbf")


def test_feasibility_kinds_bookkeeping():
    fm = gpo.FeasibilityModel(2, bounds=[0.5, 3.0], kinds=['value', 'binary'], device=3, max_iters=0, exact_feval=True)
    assert fm.kinds == ('value', 'binary') and list(fm.binary) == [False, True]
    assert fm.bounds[1] == 0.0 and fm.bounds[0] == 0.5          # a binary column's bound is 0
    assert type(fm.models[0]) is gpo.GPModel and type(fm.models[1]) is gpo.GPClassModel
    assert fm.models[1].device == 3 and fm.models[1].max_iters == 0
    C = np.array([[0.4, 0.0], [0.6, 0.0], [0.4, 1.0], [0.9, 1.0]])
    assert list(fm.feasible(C)) == [True, False, False, False]
    v = fm.violation(C)
    sd = C[:, 0].std()
    assert np.allclose(v, [0.0, 0.1 / sd, 1.0, 0.4 / sd + 1.0], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="binary"):
        fm.feasible(np.array([[0.4, 0.5]]))
    with pytest.raises(ValueError, match="kinds"):
        gpo.FeasibilityModel(2, kinds=['value'])
    with pytest.raises(ValueError, match="kinds"):
        gpo.FeasibilityModel(1, kinds=['crash'])
    assert gpo.FeasibilityModel(2, kinds='binary').kinds == ('binary', 'binary')
    assert gpo.FeasibilityModel(2).kinds == ('value', 'value')


class _Recorder(object):
    def __init__(self):
        self.Y = None

    def updateModel(self, X, Y, Xn, Yn):
        self.Y = np.array(Y)


def test_binary_column_is_not_standardised():
    fm = gpo.FeasibilityModel(2, bounds=0.5, kinds=['value', 'binary'], max_iters=0)
    fm.models = [_Recorder(), _Recorder()]
    C = np.array([[0.4, 0.0], [0.6, 0.0], [0.2, 1.0], [0.9, 1.0], [0.1, 0.0]])
    fm.update(np.zeros((5, 2)), C)
    assert fm.c_mean[1] == 0.0 and fm.c_std[1] == 1.0
    assert np.array_equal(fm.models[1].Y, C[:, 1:2])            # the labels as they came
    assert np.allclose(fm.models[0].Y[:, 0], (C[:, 0] - C[:, 0].mean()) / C[:, 0].std())
    assert list(fm.feasible_rows) == [0, 4] and fm.generation == 1
    with pytest.raises(ValueError, match="binary"):
        fm.update(np.zeros((5, 2)), C + 0.5)


class _Truth(object):
    """A constraint model that answers with the truth's latent posterior at the case's locations, as GPClassModel shapes it."""

    def __init__(self, cid):
        po = LT.posterior(cid)
        self.mean = np.asarray(po.mean, float)[:, None]
        self.sd = np.sqrt(np.asarray(po.var, float) + 1.0)[:, None]
        self.dm = np.asarray(po.dmdx, float)
        self.dsd = np.asarray(po.dvdx, float) / (2 * self.sd)

    def predict_withGradients(self, x):
        return self.mean, self.sd, self.dm, self.dsd


@pytest.mark.parametrize("cid", ["a", "d", "f"])
def test_host_fold_of_a_binary_column_is_the_probability_of_label_zero(cid):
    p, po = LT.problem(cid), LT.posterior(cid)
    fm = gpo.FeasibilityModel(1, kinds=['binary'], max_iters=0)
    fm.models = [_Truth(cid)]
    fm.generation = 1
    logF, dlogF = fm._host(p.Xs, True)
    sd = np.sqrt(1 + po.var)
    z = po.mean / sd
    want = LT.log_ndtr(-z)                                     # log p(label 0 | x) = log(1 - p(y = 1 | x))
    assert np.all(np.abs(logF - want) <= 1e-13 * np.maximum(1, np.abs(want)))
    assert np.all(np.abs(np.exp(want) - (1 - po.p)) <= 1e-15)
    lam = np.exp(-z * z / 2 - LT.HALF_LOG_2PI - want)          # phi(-z) / Phi(-z)
    dz = po.dmdx / sd[:, None] - (po.mean / sd ** 2)[:, None] * po.dvdx / (2 * sd[:, None])
    gwant = -lam[:, None] * dz
    assert np.all(np.abs(dlogF - gwant) <= 1e-12 * np.maximum(1e-3, np.abs(gwant).max()))


def test_bayesian_optimization_argument_checks():
    dom = [{'name': 'x', 'type': 'continuous', 'domain': (0, 1)}, {'name': 'y', 'type': 'continuous', 'domain': (0, 1)}]
    with pytest.raises(ValueError, match="constraint_kinds"):
        gpo.BayesianOptimization(f=None, domain=dom, X=X4, Y=Y4, constraint_kinds=['binary'])
    with pytest.raises(ValueError, match="constraint_kinds"):
        gpo.BayesianOptimization(f=None, domain=dom, X=X4, Y=Y4, C=Y4, constraint_kinds=['crash'])
    with pytest.raises(ValueError, match="constraint_kinds"):
        gpo.BayesianOptimization(f=None, domain=dom, X=X4, Y=Y4, C=Y4, constraint_kinds='maybe')
