"""``GPClassification``: a GP with a Bernoulli likelihood and a probit link, on one MI355X (GPy.models.GPClassification).

Inference is Laplace's approximation (Rasmussen & Williams, Algorithms 3.1 and 5.1) run by the device's ``gp_laplace_fit``: a Newton
iteration whose every step is one N x N Cholesky factorisation.  One stated deviation from GPy: its ``GPClassification`` defaults
to expectation propagation; here Laplace is the default and the only method (``inference_method='EP'`` raises
NotImplementedError).

After the fit the handle is an exact GP in disguise -- the factor of K + W^-1, alpha = K^-1 f at the mode, noise 1 -- so the
latent posterior, its gradients, the candidate tables and the constraint fold (``FeasibilityModel(kinds=['binary'])``) are the
regression entries unchanged.  ``predict`` returns p(y = 1 | x) = Phi(m / sqrt(1 + s^2)) (bernoulli.py:120-123).
"""
import numpy as np
from scipy.special import ndtr

from . import _lib
from .gp_regression import GPRegression, _PosteriorView
from .kern import RBF, Stationary
from .parameterization import Parameterized


class Bernoulli(Parameterized):
    """The likelihood's place in the model: a probit link, no parameter (bernoulli.py:45-57)."""

    def __init__(self, name="Bernoulli"):
        super(Bernoulli, self).__init__(name)


class GPClassification(GPRegression):
    """:param X: inputs [N, D]
    :param Y: labels in {0, 1}, [N, 1]
    :param kernel: one of the ``kern.Stationary`` classes (defaults to RBF); its variance and lengthscale(s) are the model's
        parameters -- the probit has none
    :param device: HIP device ordinal"""

    _appendable = False
    _takes_mean_function = False
    max_newton_iters = _lib.LAPLACE_MAX_ITER

    def __init__(self, X, Y, kernel=None, Y_metadata=None, mean_function=None, inference_method=None, likelihood=None,
                 normalizer=None, device=0, name="gp_classification"):
        Parameterized.__init__(self, name)
        if inference_method is not None and str(getattr(inference_method, "__name__", inference_method)).upper() not in ("LAPLACE",):
            raise NotImplementedError("GPClassification runs Laplace's approximation on the device; expectation propagation "
                                      "(GPy's default, inference_method=%r) is not implemented" % (inference_method,))
        if mean_function is not None:
            raise NotImplementedError("GPClassification takes no mean function (the Laplace fit refuses a resident one)")
        if normalizer not in (None, False):
            raise NotImplementedError("GPClassification takes no normaliser: the targets are labels")
        if likelihood is not None and not isinstance(likelihood, Bernoulli):
            raise NotImplementedError("GPClassification: the Bernoulli likelihood with a probit link only")
        X = np.asarray(X, dtype=float)
        if kernel is None:
            kernel = RBF(X.shape[1])
        if not isinstance(kernel, Stationary):
            raise TypeError("kernel must be one of the kern.Stationary classes (RBF, ExpQuad, Matern52, Matern32, Exponential, OU)")
        if kernel.Gower:
            raise NotImplementedError("GPClassification: the Gower kernel is not available under the Laplace fit")
        self._check_labels(Y)
        self.kern = kernel
        self.kern._device = int(device)
        self.likelihood = likelihood if likelihood is not None else Bernoulli()
        self.mean_function = None
        self.link_parameters(self.kern)
        self.normalizer = None
        self.Y_metadata = Y_metadata
        self.max_jitter_tries = 0      # no jitter ladder: B = I + W^1/2 K W^1/2 has eigenvalues >= 1
        self.gower_gradients = 'exact'
        self._h = _lib.Handle(device)
        self._groups = {}
        self._data_epoch = 0
        self._dirty = True
        self._lml = None
        self._jitter = 0.0
        self.newton_iters_ = self.newton_halvings_ = 0
        self.posterior = _PosteriorView(self)
        self.set_XY(X, Y)

    @staticmethod
    def _check_labels(Y):
        Y = np.asarray(Y, dtype=float)
        if Y.ndim == 1:
            Y = Y[:, None]
        if Y.ndim != 2 or Y.shape[1] != 1:
            raise NotImplementedError("GPClassification takes one column of labels, got shape %s" % (Y.shape,))
        if not np.all((Y == 0.0) | (Y == 1.0)):
            raise ValueError("GPClassification: the labels must be 0 or 1 (bernoulli.py:45-57)")
        return Y

    # -- data -----------------------------------------------------------------------------
    def set_XY(self, X=None, Y=None):
        if Y is not None:
            self.Y = self.Y_normalized = self._check_labels(Y)
            self._labels = 2.0 * self.Y[:, 0] - 1.0      # {0, 1} -> {-1, +1}
        if X is not None:
            X = np.asarray(X, dtype=float)
            assert X.ndim == 2
            self.X = X
        assert self.X.shape[0] == self.Y.shape[0]
        assert self.X.shape[1] == self.kern.input_dim
        self.num_data, self.input_dim = self.X.shape
        self.output_dim = 1
        self._h.set_data(self.X, self.Y)
        self._data_epoch += 1
        self._dirty = True

    def append_XY(self, X_new, Y_all):
        """The mode moves with every new label: always the ``set_XY`` route."""
        X_new = np.atleast_2d(np.asarray(X_new, dtype=float))
        return self.set_XY(np.concatenate([self.X, X_new], axis=0), Y_all)

    # -- (re)fit --------------------------------------------------------------------------
    def _push_params(self):
        k = self.kern
        self._h.set_params(k._kernel_id, bool(k.ARD), float(k.variance), np.ravel(k.lengthscale.values), 1.0)

    def _ensure_fit(self):
        if not self._dirty:
            return
        self._push_params()
        self._lml, self._logdet, self.newton_iters_, self.newton_halvings_ = self._h.laplace_fit(self._labels, self.max_newton_iters)
        self._dirty = False

    def _predict_resident(self, include_noise):
        self._ensure_fit()
        return self._h.predict(include_noise=include_noise)

    def _device_group(self, devices):
        raise NotImplementedError("replica groups replicate regression models only")

    def _log_likelihood_gradients_natural(self):
        """The natural gradients of log Z.  There is no gradient-only entry: gp_laplace_fit_grad always runs the whole Newton fit
        first, so ``objective_function_gradients()`` or ``.gradient`` on a model whose fit is current costs a second full fit
        (the optimiser's evaluations, which change the parameters every time, pay nothing extra)."""
        self._push_params()
        (self._lml, self._logdet, self.newton_iters_, self.newton_halvings_), (dv, dl) = self._h.laplace_fit_grad(
            self._labels, self.kern.lengthscale.size, self.max_newton_iters)
        self._dirty = False
        self.kern.variance.gradient = np.atleast_1d(dv)
        self.kern.lengthscale.gradient = dl
        return [(self.kern.variance, dv), (self.kern.lengthscale, dl)]

    def _obj_grad(self, x):
        try:
            self.optimizer_array = x
            g = self.objective_function_gradients()
            return self.objective_function(), g
        except (np.linalg.LinAlgError, RuntimeError) as e:
            if isinstance(e, RuntimeError) and "did not converge" not in str(e) and "line search failed" not in str(e):
                raise
            return 1e10, np.zeros_like(x)   # a parameter vector the Newton iteration cannot handle is a wall

    def _lockstep_applies(self, num_restarts):
        return False     # restarts are serial: the batched fits are regression fits

    # -- prediction -----------------------------------------------------------------------
    def predict(self, Xnew, full_cov=False, Y_metadata=None, kern=None, likelihood=None, include_likelihood=True):
        """(p(y = 1 | x) [M, 1], nan): the Bernoulli predictive mean through the probit, Phi(m / sqrt(1 + s^2)), and the
        reference's not-a-number in the variance's place (bernoulli.py:120-136).  ``include_likelihood=False``: the latent
        (m, s^2), as ``predict_noiseless``."""
        if full_cov and include_likelihood:
            raise NotImplementedError("GPClassification.predict: no full covariance of class probabilities")
        if not include_likelihood:
            return GPRegression.predict(self, Xnew, full_cov, Y_metadata, kern, None, False)
        m, v1 = GPRegression.predict(self, Xnew, False, Y_metadata, kern, None, True)     # noise 1: s^2 + 1
        if m.shape[0] == 0:
            return m, np.nan
        return ndtr(m / np.sqrt(v1)), np.nan

    def predict_quantiles(self, X, quantiles=(2.5, 97.5), Y_metadata=None, kern=None, likelihood=None):
        raise NotImplementedError("GPClassification: a Bernoulli predictive has no quantiles")

    def posterior_paths(self, *a, **kw):
        raise NotImplementedError("GPClassification: posterior paths condition on real-valued targets")
