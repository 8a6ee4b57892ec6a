"""``WarpedGP`` and ``WarpedGPModel`` -- the exact GP behind a learned monotone warp of its outputs.

Reference: GPy/GPy/models/warped_gp.py:13-160 (the model), GPy/GPy/util/warping_functions.py:10-169 (the warp),
GPyOpt/GPyOpt/models/warpedgpmodel.py:15-68 (the BO surrogate).

The GP itself is ``GPRegression`` on f(Y): fit, hyper-gradients, posterior and the few-row path are unchanged.  What the warp
adds on the device (include/gphip.h, "output-warped GP"): the warp of the resident targets with its log-Jacobian and the warp's
own gradients -- with the fit, ONE call per L-BFGS evaluation, ``gp_fit_grad_warp`` -- and every prediction pushed back through
the inverse warp at the Gauss-Hermite nodes, ``gp_predict_warped`` over a resident table, ``gp_warp_moments`` after the few-row
predict.
"""
import numpy as np

from . import kern as _kern
from .gp_regression import GPRegression
from .gpmodel import BOModel, _VAR_FLOOR
from .warping_functions import IdentityFunction, TanhFunction


class WarpedGP(GPRegression):
    """GP regression on f(Y), f a warping function with parameters of its own (default ``TanhFunction(warping_terms)``), learned
    with the kernel's by maximising LML + sum log f'(y).  Constructor keywords are the reference's (warped_gp.py:18) plus
    ``device``; the default kernel is ``RBF``.

    * ``Y_untransformed`` holds the (normalised) targets as given -- what the device keeps as its raw targets; ``Y_normalized``
      holds f of them once a fit has been made, as in the reference.
    * ``log_likelihood`` is the GP's LML plus the log-Jacobian (warped_gp.py:51-57).
    * ``predict`` returns mean (or, with ``median``, the median) and variance in the space of the observations while
      ``predict_in_warped_space`` is True, by Gauss-Hermite quadrature of ``deg_gauss_hermite`` nodes; the normaliser's affine
      map is applied to the latent posterior BEFORE the warp is inverted, as the reference does (warped_gp.py:101).
    * Deviations: the inverse warp is the device's bracketed Newton iteration, not the reference's damped sweeps; a negative
      latent variance gives sigma = 0 instead of NaN; the initial warp parameters are all ones (the reference draws
      ``warping_params`` at random and never uses them).
    * ``optimize_restarts(parallel=True)`` advances the restarts in lockstep, one ``gp_fit_grad_warp_batch`` per round: every
      member warps the device's raw targets with warp parameters of its own (``_batch_objective``).  Tanh warps only, up to
      64 restarts and 2048 padded rows; the serial loop otherwise.
    * Replica groups are refused."""

    _appendable = False    # append_XY refits: the fit of this model is more than the exact GP's factor of (X, Y)
    _takes_mean_function = False   # the device refuses a mean function beside an output warp

    def __init__(self, X, Y, kernel=None, warping_function=None, warping_terms=3, normalizer=False, device=0, mean_function=None):
        X = np.asarray(X, dtype=float)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if kernel is None:
            kernel = _kern.RBF(X.shape[1])
        self.warping_function = TanhFunction(warping_terms) if warping_function is None else warping_function
        if not isinstance(self.warping_function, (TanhFunction, IdentityFunction)):
            raise NotImplementedError("the accelerated path takes TanhFunction or IdentityFunction")
        self.predict_in_warped_space = True
        self._logjac = 0.0
        self._fit_count = 0
        super(WarpedGP, self).__init__(X, Y, kernel=kernel, normalizer=normalizer, mean_function=mean_function, device=device,
                                       name="warped gp")
        if self.output_dim != 1:
            raise ValueError("WarpedGP takes one output column, Y has %d" % self.output_dim)
        self.link_parameter(self.warping_function)

    # -- data -------------------------------------------------------------------------
    def set_XY(self, X=None, Y=None):
        """New data (warped_gp.py:33-36); an active warp is re-applied to the new targets on the device."""
        if Y is None and hasattr(self, "Y_untransformed"):
            self.Y_normalized = self.Y_untransformed      # (the base class uploads Y_normalized: the raw targets, not f of them)
        super(WarpedGP, self).set_XY(X, Y)
        self.Y_untransformed = self.Y_normalized.copy()

    def transform_data(self):
        """f(Y_untransformed) on the host (warped_gp.py:47-49)."""
        return self.warping_function.f(self.Y_untransformed.copy()).copy()

    # -- (re)fit ----------------------------------------------------------------------
    def _tanh(self):
        return isinstance(self.warping_function, TanhFunction)

    def _push_params(self):
        """Hyper-parameters, then the warp of the resident targets with the current warp parameters."""
        super(WarpedGP, self)._push_params()
        wf = self.warping_function
        self._logjac = self._h.set_output_warp(wf.psi, float(wf.d)) if self._tanh() else self._h.set_output_warp(None)
        self.Y_normalized = self.transform_data()

    def _ensure_fit(self):
        if self._dirty:
            self._fit_count += 1
        super(WarpedGP, self)._ensure_fit()

    def _predict_resident(self, include_noise):
        self._ensure_fit()
        return self._h.predict(include_noise=include_noise)

    def log_likelihood(self):
        """LML of the GP on f(Y) plus sum log f'(y) (warped_gp.py:51-57)."""
        self._ensure_fit()
        return self._lml + self._logjac

    def _log_likelihood_gradients_natural(self):
        nls = self.kern.lengthscale.size
        wf = self.warping_function
        if not self._tanh():
            return super(WarpedGP, self)._log_likelihood_gradients_natural()
        if self._dirty:
            # objective and gradients of a new parameter vector: warp of the targets, fit, hyper-gradients and the warp's own
            # gradients go down as ONE call
            GPRegression._push_params(self)
            (self._lml, self._logdet, self._jitter), (dv, dl, dn), self._logjac, (dpsi, dd) = self._h.fit_grad_warp(
                wf.psi, float(wf.d), nls, self.max_jitter_tries)
            self.Y_normalized = self.transform_data()
            self._dirty = False
            self._fit_count += 1
        else:
            dv, dl, dn = self._h.lml_grad(nls)
            dpsi, dd = self._h.warp_grad(wf.n_terms)
        self.kern.variance.gradient = np.atleast_1d(dv)
        self.kern.lengthscale.gradient = dl
        self.likelihood.variance.gradient = np.atleast_1d(dn)
        wf.a.gradient[:], wf.b.gradient[:], wf.c.gradient[:], wf.d.gradient[:] = dpsi[:, 0], dpsi[:, 1], dpsi[:, 2], dd
        return [(self.kern.variance, dv), (self.kern.lengthscale, dl), (self.likelihood.variance, dn),
                (wf.a, dpsi[:, 0].copy()), (wf.b, dpsi[:, 1].copy()), (wf.c, dpsi[:, 2].copy()), (wf.d, np.atleast_1d(dd))]

    def _batch_objective(self, xs):
        """``_obj_grad`` for every row of ``xs`` from ONE gp_fit_grad_warp_batch: each member warps the device's raw targets
        with warp parameters of its own and fits them with its kernel parameters.  The objective is -(LML + log-Jacobian) (and
        the priors'), its gradient the natural gradients -- the warp's ``dpsi`` into a / b / c, ``dd`` into d -- through the
        transforms' chain rule; a member that is not positive definite even with jitter is a wall (1e10, zero gradient).  The
        resident targets, warp and fit are left alone."""
        wf = self.warping_function
        k, nls = xs.shape[0], self.kern.lengthscale.size
        var, ls, noise = np.empty(k), np.empty((k, nls)), np.empty(k)
        psi, d = np.empty((k, wf.n_terms, 3)), np.empty(k)
        for j in range(k):
            self.optimizer_array = xs[j]
            var[j], ls[j], noise[j] = float(self.kern.variance), self.kern.lengthscale.values, float(self.likelihood.variance)
            psi[j], d[j] = wf.psi, float(wf.d)
        (lml, _, _), (dv, dl, dn), logjac, (dpsi, dd), status = self._h.fit_grad_warp_batch(psi, d, var, ls, noise,
                                                                                          self.max_jitter_tries)
        f, g = np.empty(k), np.zeros_like(xs)
        for j in range(k):
            if status[j] != 0:
                f[j] = 1e10
                continue
            self.optimizer_array = xs[j]     # (the priors and the chain-rule factors are taken at this member's parameters)
            natural = [(self.kern.variance, dv[j]), (self.kern.lengthscale, dl[j]), (self.likelihood.variance, dn[j]),
                       (wf.a, dpsi[j][:, 0].copy()), (wf.b, dpsi[j][:, 1].copy()), (wf.c, dpsi[j][:, 2].copy()),
                       (wf.d, np.atleast_1d(dd[j]))]
            f[j] = self._objective_value(lml[j] + logjac[j])
            g[j] = -self._transform_gradients(self._natural_with_priors(natural))
        return f, g

    def _lockstep_applies(self, num_restarts):
        """Whether the PLAIN batched entry applies (gp_fit_grad_batch, whose members share the resident targets): never for this
        model -- the library refuses it while an output warp is on.  The restarts of this model ride the warp batch, by
        ``_warp_lockstep_applies``."""
        return False

    def _warp_lockstep_applies(self, num_restarts):
        """The plain model's size rule, for the tanh warp (an ``IdentityFunction`` model keeps the serial loop)."""
        return self._tanh() and GPRegression._lockstep_applies(self, num_restarts)

    def optimize_restarts(self, num_restarts=10, robust=False, verbose=True, parallel=False, num_processes=None, **kwargs):
        """``GPRegression.optimize_restarts``; ``parallel=True`` takes the lockstep route over gp_fit_grad_warp_batch where
        ``_warp_lockstep_applies``, the serial loop otherwise."""
        if parallel and self._warp_lockstep_applies(num_restarts):
            return self._optimize_restarts_lockstep(num_restarts, robust, verbose, **kwargs)
        return super(WarpedGP, self).optimize_restarts(num_restarts, robust=robust, verbose=verbose, parallel=parallel,
                                                       num_processes=num_processes, **kwargs)

    def _device_group(self, devices):
        raise NotImplementedError("replica groups score in latent space: outside the output-warped path")

    # -- prediction ---------------------------------------------------------------------
    def _affine(self):
        """(y_mean, y_std) of the normaliser, (0, 1) without one."""
        if self.normalizer is None:
            return 0.0, 1.0
        return float(np.ravel(self.normalizer.mean)[0]), float(np.ravel(self.normalizer.std)[0])

    def _warped_moments(self, Xnew, deg, median=False, partials=False):
        """Warped (mean, var, median, partials) at ``Xnew`` with the likelihood's noise: a handful of locations through the
        few-row predict and ``gp_warp_moments``, a table through ``gp_predict_warped``."""
        y_mean, y_std = self._affine()
        few = self._few_rows(Xnew)
        if few is not None:
            m, v = self._h.predict_rows(few, include_noise=True)
            return self._h.warp_moments(m, v, y_mean, y_std, deg, median, partials)
        self._stage(Xnew)
        return self._h.predict_warped(True, y_mean, y_std, deg, median, partials)

    def predict(self, Xnew, kern=None, pred_init=None, Y_metadata=None, median=False, deg_gauss_hermite=20, likelihood=None,
                **kwargs):
        """warped_gp.py:89-116.  ``pred_init`` is accepted and ignored (the bracketed inverse needs no starting point).
        ``full_cov`` / ``include_likelihood`` are taken only with ``predict_in_warped_space`` off (the plain GP's predict)."""
        if not self.predict_in_warped_space:
            return super(WarpedGP, self).predict(Xnew, kern=kern, likelihood=likelihood, **kwargs)
        if kwargs.get("full_cov") or not kwargs.get("include_likelihood", True):
            raise NotImplementedError("predictions in the space of the observations are marginal and include the likelihood")
        if kern is not None and kern is not self.kern:
            raise NotImplementedError("prediction with a foreign kernel is outside the accelerated path")
        e = self._empty(Xnew, False)
        if e is not None:
            return e
        wmean, wvar, wmed, _ = self._warped_moments(Xnew, deg_gauss_hermite, median=median)
        return (wmed if median else wmean), wvar

    def predict_quantiles(self, X, quantiles=(2.5, 97.5), Y_metadata=None, likelihood=None, kern=None):
        """warped_gp.py:118-132: the latent quantiles through f^-1 (on the device)."""
        qs = super(WarpedGP, self).predict_quantiles(X, quantiles, Y_metadata=Y_metadata, likelihood=likelihood, kern=kern)
        if not self.predict_in_warped_space:
            return qs
        return [self._h.warp_inverse(q) for q in qs]

    def log_predictive_density(self, x_test, y_test, Y_metadata=None):
        """warped_gp.py:143-160: the Gaussian density of f(y_test) under the latent posterior plus log f'(y_test)."""
        mu, var = self._raw_predict(x_test)
        y_test = np.asarray(y_test, dtype=float)
        fy = self.warping_function.f(y_test)
        v = var + float(self.likelihood.variance)
        lpd = -0.5 * np.log(2 * np.pi) - 0.5 * np.log(v) - 0.5 * np.square(fy - mu) / v      # gaussian.py, log_predictive_density
        return lpd + np.log(self.warping_function.fgrad_y(y_test))


class WarpedGPModel(BOModel):
    """Bayesian optimisation surrogate over ``WarpedGP`` (warpedgpmodel.py:15-68).  Constructor keywords are the reference's
    plus ``device`` and ``parallel_restarts``; default kernel Matern-3/2; one ``optimize`` per update (``optimize_restarts``
    is kept and unused, as in the reference) unless ``parallel_restarts=True`` (an addition, default False): then
    ``optimize_restarts`` restarts run in lockstep, ``optimize_restarts(parallel=True)``, as ``GPModel`` does; ``predict`` returns (mean, std) in the space of the observations with the variance floored at 1e-10;
    ``get_fmin`` is ``predict(X)[0].min()`` as the reference computes it, cached per fit.

    Not a ``GPModel``: the device acquisition entries score the latent GP, so the acquisitions take their host adapter over
    ``predict`` / ``predict_withGradients``.  Pass an instance as ``BayesianOptimization(..., model=WarpedGPModel(...))``;
    ``model_type='warpedGP'`` is NOT enabled.

    Deviation from the reference: ``predict_withGradients`` is available (``analytical_gradient_prediction = True``; the
    reference sets it False and optimises the acquisition without gradients)."""
    analytical_gradient_prediction = True

    def __init__(self, kernel=None, noise_var=None, exact_feval=False, optimizer='bfgs', max_iters=1000, optimize_restarts=5,
                 warping_function=None, warping_terms=3, verbose=False, device=0, parallel_restarts=False):
        vars(self).update(parallel_restarts=bool(parallel_restarts), kernel=kernel, noise_var=noise_var, exact_feval=exact_feval, optimizer=optimizer, max_iters=max_iters,
                          optimize_restarts=optimize_restarts, warping_function=warping_function, warping_terms=warping_terms,
                          verbose=verbose, device=device, model=None)
        self._fmin_cache = None

    def _create_model(self, X, Y):
        self.input_dim = X.shape[1]
        if self.kernel is None:
            self.kernel = _kern.Matern32(self.input_dim, variance=1.)
        gp = WarpedGP(X, Y, kernel=self.kernel, warping_function=self.warping_function, warping_terms=self.warping_terms,
                      device=self.device)
        if self.noise_var is not None:
            gp.Gaussian_noise.variance.set(self.noise_var)
        if self.exact_feval:
            gp.Gaussian_noise.constrain_fixed(1e-6, warning=False)
        else:
            gp.Gaussian_noise.constrain_positive(warning=False)
        self.model = gp

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        if self.model is None:
            self._create_model(X_all, Y_all)
        else:
            self.model.set_XY(X_all, Y_all)
        if self.max_iters <= 0:
            return
        if self.parallel_restarts:   # the restarts in lockstep, one gp_fit_grad_warp_batch per round (WarpedGP._batch_objective)
            self.model.optimize_restarts(num_restarts=self.optimize_restarts, verbose=self.verbose, parallel=True,
                                         optimizer=self.optimizer, max_iters=self.max_iters)
        else:
            self.model.optimize(optimizer=self.optimizer, messages=self.verbose, max_iters=self.max_iters)

    def predict(self, X, with_noise=True):
        mean, var = self.model.predict(np.atleast_2d(X))
        return mean, np.sqrt(np.maximum(var, _VAR_FLOOR))

    def get_fmin(self):
        """``self.model.predict(self.model.X)[0].min()`` (warpedgpmodel.py:67-68): the training inputs staged as the candidate
        table, once per fit."""
        gp = self.model
        gp._ensure_fit()
        key = (gp._fit_count, gp._data_epoch)
        if self._fmin_cache is None or self._fmin_cache[0] != key:
            gp._stage(gp.X)
            y_mean, y_std = gp._affine()
            self._fmin_cache = (key, float(gp._h.predict_warped(True, y_mean, y_std, 20)[0].min()))
        return self._fmin_cache[1]

    def predict_withGradients(self, X):
        """(mean, std, d mean / dx, d std / dx) in the space of the observations: the moments kernel's partials with respect to
        the latent mean and deviation, chained with the latent posterior's input gradients."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        gp = self.model
        y_mean, y_std = gp._affine()
        few = gp._few_rows(X)
        if few is not None:     # latent posterior and gradients of a handful of locations in ONE device call, then the moments
            m, v, jac_m, jac_v = gp._h.predict_rows(few, include_noise=True, grad=True)
            wmean, wvar, _, part = gp._h.warp_moments(m, v, y_mean, y_std, 20, False, True)
        else:
            gp._stage(X)
            m, v = gp._h.predict(include_noise=True)
            wmean, wvar, _, part = gp._h.predict_warped(True, y_mean, y_std, 20, False, True)
            jac_m, jac_v = GPRegression.predictive_gradients(gp, X)
        sigma = np.sqrt(np.maximum(v, 0.0))
        dm_dx = jac_m[..., 0] * y_std                                                     # d (m y_std + y_mean) / dx
        ds_dx = np.where(sigma > 0, jac_v / (2.0 * np.where(sigma > 0, sigma, 1.0)), 0.0) * y_std   # d (sigma y_std) / dx
        dmean = part[:, 0:1] * dm_dx + part[:, 1:2] * ds_dx
        dvar = part[:, 2:3] * dm_dx + part[:, 3:4] * ds_dx
        std = np.sqrt(np.maximum(wvar, _VAR_FLOOR))
        return wmean, std, dmean, dvar / (2 * std)

    def get_model_parameters(self):
        return np.atleast_2d(self.model[:])

    def get_model_parameters_names(self):
        return self.model.parameter_names_flat().tolist()
