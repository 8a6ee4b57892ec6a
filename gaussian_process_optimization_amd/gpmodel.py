"""``GPModel`` -- host mirror of ``GPyOpt.models.GPModel`` on top of the HIP ``GPRegression`` / ``SparseGPRegression``.

Reference: GPyOpt/GPyOpt/models/base.py:7-33 (BOModel contract),
GPyOpt/GPyOpt/models/gpmodel.py:9-177 (GPModel).  Same constructor keywords, same
return conventions: ``predict`` returns (mean, **std**) with the variance clipped at
1e-10 (:95-112), ``get_fmin`` is the minimum posterior mean over the training inputs
(:125-129; cached per fit on the device -- the reference recomputes the identical
value on every acquisition call), ``predict_withGradients`` (:131-142).
"""
import numpy as np

from . import kern as _kern
from . import priors as _priors
from .gp_regression import GPRegression
from .mcmc import HMC
from .sparse_gp import SparseGPRegression


_VAR_FLOOR = 1e-10      # the reference clips predictive variances here before taking the root (gpmodel.py:99)


class BOModel(object):
    """What a surrogate offers the BO loop (GPyOpt/GPyOpt/models/base.py:7-33): subclasses fill these four in."""
    MCMC_sampler = False
    analytical_gradient_prediction = False

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        """Take the data set (``X_all``, ``Y_all``) over and re-estimate the hyper-parameters."""

    def predict(self, X):
        """(mean, standard deviation) at the rows of ``X``."""

    def predict_withGradients(self, X):
        """(mean, standard deviation, d mean / dx, d std / dx)."""

    def get_fmin(self):
        """Smallest posterior mean over the training inputs."""


class GPModel(BOModel):
    """GP surrogate on the device: exact, or with ``sparse=True`` variational DTC over ``num_inducing`` inducing inputs
    (``SparseGPRegression``, gpmodel.py:66-71).  Keyword arguments, attributes and return conventions are GPyOpt's
    (gpmodel.py:9-177); ``device`` (HIP ordinal) and ``parallel_restarts`` (the restarts in lockstep,
    GPRegression.optimize_restarts(parallel=True); default False, exact model only) are the additions.  A sparse model is
    scored by the acquisitions through ``predict`` / ``predict_withGradients`` unless ``device_acquisitions=True`` (sparse models
    only; default False): the acquisitions then score it on the device (``gp_sparse_acq*``, ``gp_sparse_acq_rows``), and ``predict``,
    ``predict_withGradients`` and the mean's gradients of up to eight locations -- the hammer precompute and ``estimate_L`` of the
    local penalisation -- go down as ONE ``gp_sparse_predict_rows`` call each.  The two routes agree to rounding, not bitwise.
    ``incremental=True`` (exact model only; default False) lets ``updateModel`` append new observations to the fitted factor
    when the hyper-parameters are kept (``max_iters <= 0``), see there.
    ``lockstep_restarts=True`` (sparse models only; default False) runs the sparse model's restarts in lockstep, one
    ``gp_sparse_fit_grad_batch`` per round of L-BFGS steps (``SparseGPRegression.optimize_restarts(parallel=True)``).  There are
    two flags because ``parallel_restarts`` was defined, and is tested, as the exact model's batch: with ``sparse=True`` it keeps
    raising, so that a configuration written for the exact model never silently changes meaning, and the sparse route is asked
    for by name.
    ``mean_function=<mappings.Mapping>`` (exact model only; an addition) gives the GP an affine trend (``GPRegression(mean_function=
    ...)``: ``mappings.Linear``, ``Constant`` or an ``Additive`` of those).  The device acquisition routes stay on and see the
    full mean."""
    analytical_gradient_prediction = True

    def __init__(self, kernel=None, noise_var=None, exact_feval=False, optimizer='bfgs', max_iters=1000,
                 optimize_restarts=5, sparse=False, num_inducing=10, verbose=True, ARD=False, Gower=False,
                 space=None, device=0, parallel_restarts=False, device_acquisitions=False, incremental=False,
                 lockstep_restarts=False, mean_function=None):
        if sparse and mean_function is not None:
            raise NotImplementedError("the sparse GP does not take a mean function")
        if sparse and incremental:
            raise ValueError("incremental appends to the exact model's factor: not available with sparse=True")
        if device_acquisitions and not sparse:
            raise ValueError("device_acquisitions selects the sparse model's device route: it needs sparse=True (the exact model "
                             "is always scored on the device)")
        if sparse and parallel_restarts:
            raise ValueError("parallel_restarts runs the exact model's batched restarts: not available with sparse=True")
        if lockstep_restarts and not sparse:
            raise ValueError("lockstep_restarts selects the sparse model's batched restarts: it needs sparse=True (the exact "
                             "model's are parallel_restarts)")
        if sparse and Gower and space is not None:
            raise NotImplementedError("the sparse GP does not take the Gower kernel")
        vars(self).update(kernel=kernel, noise_var=noise_var, exact_feval=exact_feval, optimizer=optimizer,
                          max_iters=max_iters, optimize_restarts=optimize_restarts, sparse=sparse,
                          num_inducing=num_inducing, verbose=verbose, ARD=ARD, Gower=Gower, space=space, device=device,
                          parallel_restarts=parallel_restarts, device_acquisitions=bool(device_acquisitions),
                          incremental=bool(incremental), lockstep_restarts=bool(lockstep_restarts), mean_function=mean_function,
                          model=None)

    @staticmethod
    def fromConfig(config):
        return GPModel(**config)

    def _gower(self):
        return bool(self.Gower and self.space is not None)

    def _create_model(self, X, Y):
        """First data: build the GP.  Default kernel Matern-5/2 (with the fork's Gower option passed through); default noise
        1 % of Var(Y); ``exact_feval`` pins the noise at 1e-6, otherwise it is kept inside [1e-9, 1e6] (gpmodel.py:50-76)."""
        self.input_dim = X.shape[1]
        chosen, self.kernel = self.kernel, None      # a user kernel is consumed by the first model, as in the reference
        if chosen is None:
            chosen = _kern.Matern52(self.input_dim, variance=1., ARD=self.ARD, Gower=self.Gower, space=self.space)
        if self.sparse:     # noise_var is not passed on: the likelihood starts at 1 (gpmodel.py:69-71)
            gp = SparseGPRegression(X, Y, kernel=chosen, num_inducing=self.num_inducing, device=self.device)
            gp.device_rows = self.device_acquisitions
        else:
            noise = 0.01 * Y.var() if self.noise_var is None else self.noise_var
            gp = GPRegression(X, Y, kernel=chosen, noise_var=noise, mean_function=self.mean_function, device=self.device)
        if self.exact_feval:
            gp.Gaussian_noise.constrain_fixed(1e-6, warning=False)
        else:
            gp.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
        self.model = gp

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        """New data in, then the hyper-parameter search: one L-BFGS run, or ``optimize_restarts`` of them (gpmodel.py:78-93);
        ``max_iters = 0`` keeps the hyper-parameters.  With ``incremental=True`` a model whose hyper-parameters stay
        (``max_iters <= 0``) and whose inputs are, bit for bit, the head of ``X_all`` takes the new rows by ``append_XY``: the
        factor on the device grows instead of being rebuilt."""
        if self.model is not None:
            if self.incremental and self.max_iters <= 0 and self._is_head(X_all):
                self.model.append_XY(np.asarray(X_all, dtype=float)[self.model.X.shape[0]:], Y_all)
            else:
                self.model.set_XY(X_all, Y_all)
        else:
            self._create_model(X_all, Y_all)
        if self.max_iters <= 0:
            return
        search = dict(optimizer=self.optimizer, max_iters=self.max_iters)
        if self.optimize_restarts == 1:
            self.model.optimize(messages=False, ipython_notebook=False, **search)
        else:
            # the restarts in lockstep: one gp_fit_grad_batch per round (GPRegression.optimize_restarts), or, for the sparse
            # model, one gp_sparse_fit_grad_batch (SparseGPRegression)
            if self.parallel_restarts or self.lockstep_restarts:
                search["parallel"] = True
            self.model.optimize_restarts(num_restarts=self.optimize_restarts, verbose=self.verbose, **search)

    def _is_head(self, X_all):
        """``X_all`` is the model's inputs, bit for bit, with at least one more row under them."""
        X_all, X = np.asarray(X_all, dtype=float), self.model.X
        N = X.shape[0]
        return (X_all.ndim == 2 and X_all.shape[1] == X.shape[1] and X_all.shape[0] > N and
                np.ascontiguousarray(X_all[:N]).tobytes() == np.ascontiguousarray(X).tobytes())

    def _predict(self, X, full_cov, include_likelihood):
        mean, var = self.model.predict(np.atleast_2d(X), full_cov=full_cov, include_likelihood=include_likelihood)
        return mean, np.maximum(var, _VAR_FLOOR)

    def predict(self, X, with_noise=True):
        mean, var = self._predict(X, False, with_noise)
        return mean, np.sqrt(var)

    def predict_covariance(self, X, with_noise=True):
        return self._predict(X, True, with_noise)[1]

    def get_fmin(self):
        """``self.model.predict(self.model.X)[0].min()`` (gpmodel.py:125-129), evaluated on the device and cached per fit."""
        gp = self.model
        gp._ensure_fit()
        lowest = gp._h.sparse_fmin() if self.sparse else gp._h.fmin()
        if gp.normalizer is not None:
            lowest = float(gp.normalizer.inverse_mean(np.array([[lowest]]))[0, 0])
        return lowest

    def predict_withGradients(self, X):
        """Mean, std and their input gradients (gpmodel.py:131-142); with a normaliser the gradients are those of the
        un-normalised mean / variance."""
        X = np.atleast_2d(X)
        gp = self.model
        few = None if self.sparse else gp._few_rows(X)
        if self.sparse:         # posterior and gradients in ONE device call (gp_sparse_predict)
            mean, var, jac_mean, jac_var = gp._sparse_predict(X, True, grad=True)
            if gp.normalizer is not None:
                mean, var = gp.normalizer.inverse_mean(mean), gp.normalizer.inverse_variance(var)
        elif few is not None:   # posterior and gradients of a handful of locations in ONE device call (gp_predict_rows)
            mean, var, jac_mean, jac_var = gp._h.predict_rows(few, include_noise=True, grad=True)
            if gp.normalizer is not None:
                mean, var = gp.normalizer.inverse_mean(mean), gp.normalizer.inverse_variance(var)
        else:
            mean, var = gp.predict(X)
            jac_mean, jac_var = gp.predictive_gradients(X)
        std = np.sqrt(np.maximum(var, _VAR_FLOOR))
        jac_mean = jac_mean[..., 0]
        if gp.normalizer is not None:
            jac_mean = jac_mean * gp.normalizer.std
            jac_var = jac_var * gp.normalizer.std ** 2
        return mean, std, jac_mean, jac_var / (2 * std)

    def copy(self):
        twin = GPModel(kernel=self.model.kern.copy(), noise_var=self.noise_var, exact_feval=self.exact_feval,
                       optimizer=self.optimizer, max_iters=self.max_iters, optimize_restarts=self.optimize_restarts,
                       sparse=self.sparse, num_inducing=self.num_inducing, verbose=self.verbose, ARD=self.ARD, Gower=self.Gower, space=self.space, device=self.device,
                       parallel_restarts=self.parallel_restarts, device_acquisitions=self.device_acquisitions,
                       incremental=self.incremental, lockstep_restarts=self.lockstep_restarts,
                       mean_function=None if self.model.mean_function is None else self.model.mean_function.copy())
        twin._create_model(self.model.X, self.model.Y)
        twin.updateModel(self.model.X, self.model.Y, None, None)
        return twin

    def get_model_parameters(self):
        return np.atleast_2d(self.model[:])

    def get_model_parameters_names(self):
        return self.model.parameter_names_flat().tolist()

    def get_covariance_between_points(self, x1, x2):
        """Posterior covariance between two point sets (gpmodel.py:173-177)."""
        return self.model.posterior_covariance_between_points(x1, x2)


class GPModel_MCMC(BOModel):
    """GP surrogate whose hyper-parameters are integrated out by HMC (GPyOpt/GPyOpt/models/gpmodel.py:180-355): same
    constructor keywords plus ``device``, the same lists of one array per sample from ``predict``, ``predict_withGradients`` and
    ``get_fmin``.  The reference writes every sample into the model and refactorises for each of those calls (:266-272, 285-291,
    307-315); here ``updateModel`` ends with ONE ``gp_ens_fit`` that factors the samples in lockstep and keeps their posteriors
    on the device, and the calls above read that ensemble (``gp_ens_predict_rows``, eight locations per call)."""
    MCMC_sampler = True
    analytical_gradient_prediction = True

    def __init__(self, kernel=None, noise_var=None, exact_feval=False, n_samples=10, n_burnin=100, subsample_interval=10,
                 step_size=1e-1, leapfrog_steps=20, verbose=False, device=0, mean_function=None):
        if mean_function is not None:
            raise NotImplementedError("GPModel_MCMC does not take a mean function (the ensemble entries refuse one)")
        vars(self).update(kernel=kernel, noise_var=noise_var, exact_feval=exact_feval, verbose=verbose, n_samples=n_samples,
                          subsample_interval=subsample_interval, n_burnin=n_burnin, step_size=step_size,
                          leapfrog_steps=leapfrog_steps, device=device, model=None, hmc=None, hmc_samples=None, _fmins=None)

    def _create_model(self, X, Y):
        """Default kernel RBF with variance 1, default noise 1 % of Var(Y); Gamma priors with mean 2 and variance 4 on the
        kernel parameters and on the noise; ``exact_feval`` fixes the noise at 1e-6 (gpmodel.py:213-238)."""
        self.input_dim = X.shape[1]
        chosen, self.kernel = self.kernel, None
        if chosen is None:
            chosen = _kern.RBF(self.input_dim, variance=1.)
        noise = Y.var() * 0.01 if self.noise_var is None else self.noise_var
        gp = GPRegression(X, Y, kernel=chosen, noise_var=noise, device=self.device)
        gp.kern.set_prior(_priors.Gamma.from_EV(2., 4.))
        gp.likelihood.variance.set_prior(_priors.Gamma.from_EV(2., 4.))
        if self.exact_feval:
            gp.Gaussian_noise.constrain_fixed(1e-6, warning=False)
        else:
            gp.Gaussian_noise.constrain_positive(warning=False)
        self.model = gp

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        """gpmodel.py:240-255: the MAP search, a 1 % perturbation of every parameter, the HMC chain, its thinning -- then the
        kept samples are factored once and stay resident."""
        if self.model is None:
            self._create_model(X_all, Y_all)
        else:
            self.model.set_XY(X_all, Y_all)
        gp = self.model
        gp.optimize(max_iters=200)
        gp[:] = gp.param_array * (1. + np.random.randn(gp.param_array.size) * 0.01)
        self.hmc = HMC(gp, stepsize=self.step_size)
        ss = self.hmc.sample(num_samples=self.n_burnin + self.n_samples * self.subsample_interval, hmc_iters=self.leapfrog_steps)
        self.hmc_samples = ss[self.n_burnin::self.subsample_interval]
        self._fit_ensemble()

    def _members(self):
        """(variance [S], lengthscale [S, nls], noise [S]) of the kept samples: a sample holds the unfixed parameters in
        ``param_array`` order -- kernel variance, lengthscale(s), then the noise unless ``exact_feval`` fixed it."""
        gp, ss = self.model, np.atleast_2d(self.hmc_samples)
        nls = gp.kern.lengthscale.size
        noise = ss[:, 1 + nls] if ss.shape[1] > 1 + nls else np.full(ss.shape[0], float(gp.likelihood.variance))
        return ss[:, 0].copy(), ss[:, 1:1 + nls].copy(), np.asarray(noise, dtype=float).copy()

    def _fit_ensemble(self):
        gp = self.model
        gp._push_params()      # kernel family, ARD and lengthscale count of the members come from the handle's parameters
        gp._dirty = True       # (which drops the handle's own fit: the model refits when it is next asked for itself)
        var, ls, noise = self._members()
        _, _, _, self._fmins = gp._h.ens_fit(var, ls, noise, gp.max_jitter_tries)

    def _rows(self, X, grad):
        """The S posteriors at the rows of ``X``, eight locations per device call: (mean, var[, dmdx, dvdx]) as [S, M(, D)]."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        parts = [self.model._h.ens_predict_rows(X[i:i + 8], True, grad=grad) for i in range(0, X.shape[0], 8)]
        return [np.concatenate([p[k] for p in parts], axis=1) for k in range(4 if grad else 2)]

    def predict(self, X):
        """Lists of S means [M, 1] and S standard deviations [M, 1] (gpmodel.py:257-277)."""
        mean, var = self._rows(X, False)
        return [m[:, None] for m in mean], [np.sqrt(np.clip(v, _VAR_FLOOR, np.inf))[:, None] for v in var]

    def get_fmin(self):
        """The S minima of the members' posterior means over the training inputs (gpmodel.py:279-295), kept by the fit."""
        return [float(f) for f in self._fmins]

    def predict_withGradients(self, X):
        """Lists of S means, standard deviations [M, 1] and their x-gradients [M, D] (gpmodel.py:297-324)."""
        mean, var, dm, dv = self._rows(X, True)
        stds = [np.sqrt(np.clip(v, _VAR_FLOOR, np.inf))[:, None] for v in var]
        return [m[:, None] for m in mean], stds, [d for d in dm], [d / (2 * s) for d, s in zip(dv, stds)]

    def copy(self):
        """A working twin (the reference's ``copy`` builds the wrong class, gpmodel.py:331)."""
        twin = GPModel_MCMC(kernel=self.model.kern.copy(), noise_var=self.noise_var, exact_feval=self.exact_feval,
                            n_samples=self.n_samples, n_burnin=self.n_burnin, subsample_interval=self.subsample_interval,
                            step_size=self.step_size, leapfrog_steps=self.leapfrog_steps, verbose=self.verbose, device=self.device)
        twin.updateModel(self.model.X, self.model.Y, None, None)
        return twin

    def get_model_parameters(self):
        return np.atleast_2d(self.model[:])

    def get_model_parameters_names(self):
        return self.model.parameter_names_flat().tolist()


class GPClassModel(BOModel):
    """A GP classifier as a BO surrogate (``GPClassification``: Bernoulli likelihood, probit link, Laplace fit on the device), in
    the shape ``FeasibilityModel`` takes a constraint model in.  ``updateModel(X, Y, ...)`` takes labels in {0, 1};
    ``predict`` / ``predict_withGradients`` return the LATENT mean and sqrt(s^2 + 1) (``with_noise=False``: sqrt(s^2)), so that
    Phi((0 - mean) / std) is the probability of label 0 -- the term the constraint fold evaluates.  While the labels hold one
    class only the model is fitted at its current hyper-parameters without a search."""
    analytical_gradient_prediction = True
    sparse = False

    def __init__(self, kernel=None, optimizer='bfgs', max_iters=1000, optimize_restarts=5, verbose=True, ARD=False, device=0):
        vars(self).update(kernel=kernel, optimizer=optimizer, max_iters=max_iters, optimize_restarts=optimize_restarts,
                          verbose=verbose, ARD=ARD, device=device, model=None)

    def _create_model(self, X, Y):
        from .gp_classification import GPClassification
        self.input_dim = X.shape[1]
        chosen, self.kernel = self.kernel, None
        if chosen is None:
            chosen = _kern.Matern52(self.input_dim, variance=1., ARD=self.ARD)
        self.model = GPClassification(X, Y, kernel=chosen, device=self.device)

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        if self.model is not None:
            self.model.set_XY(X_all, Y_all)
        else:
            self._create_model(np.asarray(X_all, dtype=float), Y_all)
        labels = np.ravel(self.model.Y)
        if self.max_iters <= 0 or labels.min() == labels.max():
            return
        search = dict(optimizer=self.optimizer, max_iters=self.max_iters)
        if self.optimize_restarts == 1:
            self.model.optimize(messages=False, ipython_notebook=False, **search)
        else:
            self.model.optimize_restarts(num_restarts=self.optimize_restarts, verbose=self.verbose, **search)

    def predict(self, X, with_noise=True):
        mean, var = GPRegression.predict(self.model, np.atleast_2d(X), include_likelihood=with_noise)
        return mean, np.sqrt(np.maximum(var, _VAR_FLOOR))

    def predict_proba(self, X):
        """p(label = 1 | x) [M, 1]."""
        return self.model.predict(np.atleast_2d(X))[0]

    def predict_withGradients(self, X):
        X = np.atleast_2d(X)
        gp = self.model
        few = gp._few_rows(X)
        if few is not None:
            mean, var, jac_mean, jac_var = gp._h.predict_rows(few, include_noise=True, grad=True)
        else:
            mean, var = GPRegression.predict(gp, X, include_likelihood=True)
            jac_mean, jac_var = gp.predictive_gradients(X)
        std = np.sqrt(np.maximum(var, _VAR_FLOOR))
        return mean, std, jac_mean[..., 0], jac_var / (2 * std)

    def get_fmin(self):
        raise NotImplementedError("a classifier has no observed minimum")

    def get_model_parameters(self):
        return np.atleast_2d(self.model[:])

    def get_model_parameters_names(self):
        return self.model.parameter_names_flat().tolist()
