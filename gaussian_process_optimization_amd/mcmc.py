"""Hybrid Monte Carlo over a model's unfixed hyper-parameters, in the optimiser's (transformed) space.

Reference: GPy/GPy/inference/mcmc/hmc.py:7-68.  The model is anything with ``optimizer_array`` (get / set),
``unfixed_param_array``, ``objective_function()`` (the negative log posterior) and ``objective_function_gradients()`` (its
gradient with respect to ``optimizer_array``); on ``GPRegression`` every leapfrog gradient is one ``gp_fit_grad`` on the device,
which leaves the objective of the same point behind.  Draws come from the global ``np.random`` in the reference's order: one
``multivariate_normal`` for the momentum, then one ``rand`` for the accept test, per sample.
"""
import numpy as np


class HMC(object):
    """``HMC(model, M=None, stepsize=1e-1)``: ``M`` is the mass matrix (identity by default)."""

    def __init__(self, model, M=None, stepsize=1e-1):
        self.model = model
        self.stepsize = stepsize
        self.p = np.empty_like(np.asarray(model.optimizer_array, dtype=float).copy())
        self.M = np.eye(self.p.size) if M is None else M
        self.Minv = np.linalg.inv(self.M)
        self.accepted = []          # the accept decision of every sample of the last ``sample`` call

    def sample(self, num_samples=1000, hmc_iters=20):
        """``num_samples`` rows of the unfixed parameters (hmc.py:30-59).  Row i is recorded BEFORE the trajectory and
        overwritten when the proposal is accepted (hmc.py:46,56): a rejected proposal repeats the previous state."""
        params = np.empty((num_samples, self.p.size))
        self.accepted = []
        for i in range(num_samples):
            self.p[:] = np.random.multivariate_normal(np.zeros(self.p.size), self.M)
            H_old = self._computeH()
            theta_old = np.array(self.model.optimizer_array, dtype=float)
            params[i] = self.model.unfixed_param_array
            self._update(hmc_iters)
            H_new = self._computeH()
            k = 1. if H_old > H_new else np.exp(H_old - H_new)
            accept = bool(np.random.rand() < k)
            self.accepted.append(accept)
            if accept:
                params[i] = self.model.unfixed_param_array
            else:
                self.model.optimizer_array = theta_old
        return params

    def _update(self, hmc_iters):
        """Leapfrog: half a momentum step, a position step, half a momentum step (hmc.py:61-65)."""
        for _ in range(hmc_iters):
            self.p[:] += -self.stepsize / 2. * self.model.objective_function_gradients()
            self.model.optimizer_array = self.model.optimizer_array + self.stepsize * np.dot(self.Minv, self.p)
            self.p[:] += -self.stepsize / 2. * self.model.objective_function_gradients()

    def _computeH(self):
        """Potential (the model's objective) plus the Gaussian kinetic term with its normaliser (hmc.py:67-68)."""
        kinetic = np.dot(self.p, np.dot(self.Minv, self.p[:, None])) / 2.
        return float(np.ravel(self.model.objective_function() + self.p.size * np.log(2 * np.pi) / 2.
                              + np.log(np.linalg.det(self.M)) / 2. + kinetic)[0])
