"""Priors on hyper-parameters: what ``GPModel_MCMC`` puts on the kernel and the noise.

Reference: GPy/GPy/core/parameterization/priors.py (``Gamma``: density, ``from_EV``), used through ``set_prior`` /
``log_prior`` / ``_log_prior_gradients`` (GPy/GPy/core/parameterization/priorizable.py:25-82), which live in
``parameterization.py`` here.
"""
import numpy as np
from scipy.special import gammaln

POSITIVE = "positive"


class Gamma(object):
    """Gamma density with shape ``a`` and rate ``b``: ln p(x) = a ln b - ln Gamma(a) + (a - 1) ln x - b x."""
    domain = POSITIVE

    def __init__(self, a, b):
        self.a, self.b = float(a), float(b)
        self.constant = -gammaln(self.a) + self.a * np.log(self.b)

    @staticmethod
    def from_EV(E, V):
        """The Gamma with expectation ``E`` and variance ``V``: a = E^2 / V, b = E / V."""
        return Gamma(np.square(E) / V, E / V)

    def lnpdf(self, x):
        x = np.asarray(x, dtype=float)
        return self.constant + (self.a - 1.0) * np.log(x) - self.b * x

    def lnpdf_grad(self, x):
        x = np.asarray(x, dtype=float)
        return (self.a - 1.0) / x - self.b

    def rvs(self, n):
        return np.random.gamma(scale=1.0 / self.b, shape=self.a, size=n)

    def __repr__(self):
        return "Ga(%.2g, %.2g)" % (self.a, self.b)
