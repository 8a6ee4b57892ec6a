"""Input warping functions: the Kumaraswamy CDF of the input-warped GP, and the log-Gaussian prior on its parameters.

Reference: GPy/GPy/util/input_warping_functions.py:60-258 (KumarWarping), GPy/GPy/core/parameterization/priors.py:142-182
(LogGaussian); Snoek, Swersky, Zemel & Adams, "Input Warping for Bayesian Optimization of Non-stationary Functions" (2014).

Host bookkeeping only: the N x D training inputs are warped here (2 N D ``pow``), a candidate table is warped on the device
(``gp_set_candidates_kumar``), and the gradient of the LML with respect to the warped inputs that ``update_grads`` consumes
comes from the device (``gp_lml_grad_x``).
"""
import numpy as np

from .parameterization import Logistic, Param, Parameterized


class LogGaussian(object):
    """Univariate log-Gaussian density on the positive reals (priors.py:142-182)."""

    def __init__(self, mu=0., sigma=1.):
        self.mu = float(mu)
        self.sigma = float(sigma)
        self.sigma2 = np.square(self.sigma)
        self.constant = -0.5 * np.log(2 * np.pi * self.sigma2)

    def __str__(self):
        return "lnN({:.2g}, {:.2g})".format(self.mu, self.sigma)

    def lnpdf(self, x):
        return self.constant - 0.5 * np.square(np.log(x) - self.mu) / self.sigma2 - np.log(x)

    def lnpdf_grad(self, x):
        return -((np.log(x) - self.mu) / self.sigma2 + 1.) / x


class InputWarpingFunction(Parameterized):
    """What an input warping offers the model (input_warping_functions.py:9-24)."""

    def f(self, X, test_data=False):
        raise NotImplementedError

    def fgrad_X(self, X, test_data=False):
        raise NotImplementedError

    def update_grads(self, X, dL_dW):
        raise NotImplementedError


class KumarWarping(InputWarpingFunction):
    """Kumaraswamy-CDF warping of the numerical inputs: w(x) = 1 - (1 - u^a)^b with u = (x - Xmin) / (Xmax - Xmin) on the
    columns ``warping_indices`` (default: all), one (a, b) pair per warped column (input_warping_functions.py:60-258).

    ``Xmin`` / ``Xmax`` default to the extremes of ``X`` and are widened by ``epsilon`` (default 1e-6), so that the training
    inputs normalise into (0, 1).  The parameters start at 1 (the identity), live in (0, 10) through the ``Logistic``
    transform and carry ``LogGaussian(0, 0.75)`` priors (``param.prior``), as in the reference.

    ``f`` and ``fgrad_X`` take ``test_data=True`` to normalise the ``X`` they are given; without it they use the training
    inputs the object holds (``X_normalized``), whatever ``X`` is -- the reference's convention.  ``fgrad_X`` with
    ``test_data=True`` is an addition (the reference differentiates at the training inputs only); like the reference's, it is
    zero in the columns that are not warped.  ``set_X`` (an addition) replaces the training inputs under the same bounds."""

    def __init__(self, X, warping_indices=None, epsilon=None, Xmin=None, Xmax=None):
        super(KumarWarping, self).__init__(name='input_warp_kumar')
        X = np.asarray(X, dtype=float)
        if warping_indices is not None and np.max(warping_indices) > X.shape[1] - 1:
            raise ValueError("Kumar warping indices exceed feature dimension")
        if warping_indices is not None and np.min(warping_indices) < 0:
            raise ValueError("Kumar warping indices should be larger than 0")
        if warping_indices is not None and np.any([not isinstance(i, int) for i in warping_indices]):
            raise ValueError("Kumar warping indices should be integer")
        if Xmin is None and Xmax is None:
            Xmin = X.min(axis=0)
            Xmax = X.max(axis=0)
        else:
            if Xmin is None or Xmax is None:
                raise ValueError("Xmin and Xmax need to be provide at the same time!")
            if len(Xmin) != X.shape[1] or len(Xmax) != X.shape[1]:
                raise ValueError("Xmin and Xmax should have n_feature values!")
        self.epsilon = 1e-6 if epsilon is None else epsilon
        self.Xmin = np.asarray(Xmin, dtype=float) - self.epsilon
        self.Xmax = np.asarray(Xmax, dtype=float) + self.epsilon
        self.scaling = 1.0 / (self.Xmax - self.Xmin)
        self.set_X(X)
        if warping_indices is None:
            warping_indices = range(X.shape[1])
        self.warping_indices = list(warping_indices)
        self.warping_dim = len(self.warping_indices)
        self.num_parameters = 2 * self.warping_dim
        self.params = [[Param('a%d' % i, 1.0, Logistic(0.0, 10.0)), Param('b%d' % i, 1.0, Logistic(0.0, 10.0))]
                       for i in range(self.warping_dim)]
        for pair in self.params:
            for p in pair:
                p.prior = LogGaussian(0.0, 0.75)
                self.link_parameter(p)

    def set_X(self, X):
        """New training inputs, normalised with the bounds fixed at construction."""
        self.X_normalized = (np.asarray(X, dtype=float) - self.Xmin) / (self.Xmax - self.Xmin)

    def _normalized(self, X, test_data):
        return (np.asarray(X, dtype=float) - self.Xmin) / (self.Xmax - self.Xmin) if test_data else self.X_normalized

    def values(self):
        """(a [warping_dim], b [warping_dim]) as plain arrays."""
        return (np.array([float(p[0]) for p in self.params]), np.array([float(p[1]) for p in self.params]))

    def device_arguments(self, input_dim):
        """(warp, a, b, xmin, xmax), one entry per input column: what ``gp_set_candidates_kumar`` takes."""
        warp = np.zeros(input_dim, dtype=np.int32)
        a, b = np.ones(input_dim), np.ones(input_dim)
        for i_seq, i_fea in enumerate(self.warping_indices):
            warp[i_fea] = 1
            a[i_fea], b[i_fea] = float(self.params[i_seq][0]), float(self.params[i_seq][1])
        return warp, a, b, np.array(self.Xmin, dtype=float), np.array(self.Xmax, dtype=float)

    def f(self, X, test_data=False):
        """f(x) = 1 - (1 - u^a)^b on the warped columns, the value itself elsewhere (input_warping_functions.py:171-199)."""
        X_warped = np.array(X, dtype=float)
        Xn = self._normalized(X, test_data)
        for i_seq, i_fea in enumerate(self.warping_indices):
            a, b = float(self.params[i_seq][0]), float(self.params[i_seq][1])
            X_warped[:, i_fea] = 1 - np.power(1 - np.power(Xn[:, i_fea], a), b)
        return X_warped

    def fgrad_X(self, X, test_data=False):
        """df/dx = a b u^(a-1) (1 - u^a)^(b-1) / (Xmax - Xmin) on the warped columns, 0 elsewhere (:201-223)."""
        Xn = self._normalized(X, test_data)
        grad = np.zeros(Xn.shape)
        for i_seq, i_fea in enumerate(self.warping_indices):
            a, b = float(self.params[i_seq][0]), float(self.params[i_seq][1])
            u = Xn[:, i_fea]
            grad[:, i_fea] = a * b * np.power(u, a - 1) * np.power(1 - np.power(u, a), b - 1) * self.scaling[i_fea]
        return grad

    def update_grads(self, X, dL_dW):
        """The parameters' gradients from dL/dW [N, D], the gradient with respect to the warped training inputs (:225-258):
        dW/da = b (1 - u^a)^(b-1) u^a ln u,  dW/db = -(1 - u^a)^b ln(1 - u^a), summed over the data."""
        Xn = self.X_normalized
        for i_seq, i_fea in enumerate(self.warping_indices):
            ai, bi = float(self.params[i_seq][0]), float(self.params[i_seq][1])
            x_pow_a = np.power(Xn[:, i_fea], ai)
            dz_dai = bi * np.power(1 - x_pow_a, bi - 1) * x_pow_a * np.log(Xn[:, i_fea])
            dz_dbi = -np.power(1 - x_pow_a, bi) * np.log(1 - x_pow_a)
            self.params[i_seq][0].gradient[:] = np.sum(dL_dW[:, i_fea] * dz_dai)
            self.params[i_seq][1].gradient[:] = np.sum(dL_dW[:, i_fea] * dz_dbi)
