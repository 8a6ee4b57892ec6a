"""``InputWarpedGP`` and ``InputWarpedGPModel`` -- the exact GP behind a learned Kumaraswamy warping of its inputs.

Reference: GPy/GPy/models/input_warped_gp.py:12-144 (the model), GPyOpt/GPyOpt/models/input_warped_gpmodel.py:9-88 (the BO
surrogate), GPyOpt/GPyOpt/util/arguments_manager.py:137-147 (``model_type='input_warped_GP'``).

The GP itself is ``GPRegression`` on the warped inputs: fit, posterior and acquisition kernels are unchanged.  What the
warping adds on the device is the LML's gradient with respect to the (warped) training inputs -- ``gp_fit_grad_x``, one call
per L-BFGS evaluation -- and the warp of a candidate table, ``gp_set_candidates_kumar``.
"""
import numpy as np

from . import kern as _kern
from .gp_regression import GPRegression
from .gpmodel import BOModel, _VAR_FLOOR
from .input_warping import KumarWarping

_FEW = 8     # up to this many prediction locations are warped on the host and go down by value (gp_predict_rows)


class InputWarpedGP(GPRegression):
    """GP regression on w(X), w a warping function with parameters of its own (default ``KumarWarping``), learned with the
    kernel's by maximising LML + log prior.  Constructor keywords are the reference's (input_warped_gp.py:73) plus ``device``;
    the default kernel is ``Matern32``.

    * ``X_untransformed`` keeps the inputs as given; ``X`` holds the warped inputs the device sees.
    * ``set_XY`` takes UN-WARPED inputs: they are re-normalised with the ``Xmin`` / ``Xmax`` fixed at construction, warped and
      pushed.  (The reference inherits ``GP.set_XY``, which would store un-warped inputs in the warped slot; that is not
      reproduced.)
    * A change of a warping parameter marks the data stale: the next evaluation re-warps the training inputs, calls
      ``gp_set_data`` and then ``gp_fit_grad_x``.
    * The objective is -(LML + sum of the parameters' log priors) in natural space, its gradient the natural gradients plus
      the priors' through the transforms' chain rule, as for the other parameters.  NO Jacobian term of the transforms is
      added to the prior (paramz is not part of the reference tree, so whether it adds one cannot be pinned).
    * ``predict``, ``predict_noiseless``, ``predict_quantiles``, ``posterior_samples_f`` and
      ``posterior_covariance_between_points`` warp their locations first: tables above eight rows on the device
      (``gp_set_candidates_kumar``), fewer on the host.  ``predictive_gradients`` and ``mean_gradients`` return gradients with
      respect to the UN-WARPED inputs.
    * A Gower kernel raises ``NotImplementedError``.
    * ``optimize_restarts(parallel=True)`` advances the restarts in lockstep, one ``gp_fit_grad_x_batch`` per round: every
      member travels with training inputs of its own, warped on the host by its warping parameters (``_batch_objective``).
      The size rule is the plain model's: up to 64 restarts and 2048 padded rows, the serial loop beyond."""

    _appendable = False    # append_XY refits: the fit of this model is more than the exact GP's factor of (X, Y)
    _takes_mean_function = False   # the input-gradient entries do not carry a mean function

    def __init__(self, X, Y, kernel=None, normalizer=False, warping_function=None, warping_indices=None, Xmin=None, Xmax=None,
                 epsilon=None, device=0, mean_function=None):
        X = np.asarray(X, dtype=float)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if kernel is None:
            kernel = _kern.Matern32(X.shape[1], variance=1.)
        if getattr(kernel, "Gower", False) and getattr(kernel, "space", None) is not None:
            raise NotImplementedError("input warping under the Gower kernel is out of scope")
        self.X_untransformed = X.copy()
        self.warping_function = (KumarWarping(self.X_untransformed, warping_indices, epsilon, Xmin, Xmax)
                                 if warping_function is None else warping_function)
        self._warp_signature = None
        super(InputWarpedGP, self).__init__(X, Y, kernel=kernel, normalizer=normalizer, mean_function=mean_function, device=device,
                                            name="input warped gp")
        self.kernel = self.kern
        self.link_parameter(self.warping_function)

    # -- data -------------------------------------------------------------------------
    def _signature(self):
        return tuple(float(p) for p in self.warping_function.flattened_parameters())

    def transform_data(self, X, test_data=False, device=False):
        """w(X) (input_warped_gp.py:107-117).  ``device=True`` (with ``test_data``) warps the table on the device, where it
        also becomes the resident candidate block."""
        if device and test_data and isinstance(self.warping_function, KumarWarping):
            X = np.atleast_2d(np.asarray(X, dtype=float))
            return self._h.set_candidates_kumar(X, *self.warping_function.device_arguments(self.input_dim), want_warped=True)
        return self.warping_function.f(np.asarray(X, dtype=float), test_data)

    def set_XY(self, X=None, Y=None):
        """New data, X UN-WARPED (see the class docstring)."""
        if X is not None:
            X = np.asarray(X, dtype=float)
            if X.ndim == 1:
                X = X.reshape(-1, 1)
            self.X_untransformed = X.copy()
            if hasattr(self.warping_function, "set_X"):
                self.warping_function.set_X(self.X_untransformed)
        Xw = self.transform_data(self.X_untransformed) if (X is not None or self._warp_signature != self._signature()) else None
        super(InputWarpedGP, self).set_XY(Xw, Y)
        self.X_warped = self.X
        self._warp_signature = self._signature()

    def _push_params(self):
        """Hyper-parameters to the device and, when a warping parameter moved since the inputs were last pushed, the
        re-warped training inputs before them."""
        if self._warp_signature != self._signature():
            self.X = self.X_warped = self.transform_data(self.X_untransformed)
            self._h.set_data(self.X, self.Y_normalized)
            self._data_epoch += 1
            self._warp_signature = self._signature()
        super(InputWarpedGP, self)._push_params()

    # -- objective ----------------------------------------------------------------------
    def _prior_parameters(self):
        return [p for p in self.flattened_parameters() if getattr(p, "prior", None) is not None]

    def log_prior(self):
        return float(sum(np.sum(p.prior.lnpdf(p.values)) for p in self._prior_parameters()))

    def objective_function(self):
        """-(LML + log prior) (Model.objective_function, core/model.py:96-110)."""
        return self._objective_value(self.log_likelihood())

    def _objective_value(self, log_likelihood):
        return -float(log_likelihood) - self.log_prior()

    def _log_likelihood_gradients_natural(self):
        nls = self.kern.lengthscale.size
        if self._dirty:
            # objective and gradients of a new parameter vector: fit, hyper-gradients and dL/dX go down as ONE call
            self._push_params()
            (self._lml, self._logdet, self._jitter), (dv, dl, dn), dL_dX = self._h.fit_grad_x(nls, self.max_jitter_tries)
            self._dirty = False
        else:
            dv, dl, dn = self._h.lml_grad(nls)
            dL_dX = self._h.lml_grad_x()
        self.kern.variance.gradient = np.atleast_1d(dv)
        self.kern.lengthscale.gradient = dl
        self.likelihood.variance.gradient = np.atleast_1d(dn)
        # input_warped_gp.py:103-105: dL/dX of the warped inputs into the warping parameters' gradients
        self.warping_function.update_grads(self.X_untransformed, dL_dX)
        out = [(self.kern.variance, dv), (self.kern.lengthscale, dl), (self.likelihood.variance, dn)]
        out.extend((p, p.gradient.copy()) for p in self.warping_function.flattened_parameters())
        return out

    def _natural_with_priors(self, natural):
        """d(LML + log prior) in natural space (``objective_function_gradients`` chains it through the transforms)."""
        return [(p, np.asarray(g, dtype=float).reshape(-1) + (p.prior.lnpdf_grad(p.values) if getattr(p, "prior", None)
                                                              is not None else 0.0)) for p, g in natural]

    def _batch_objective(self, xs):
        """``_obj_grad`` for every row of ``xs`` from ONE gp_fit_grad_x_batch.  Each member's training inputs are warped here, on
        the host, with the ``transform_data`` the serial loop uses -- the member's inputs are the serial loop's bits -- and
        travel with the call; the resident data and ``_warp_signature`` are left alone, so the ``_ensure_fit`` that closes the
        search re-warps as it does after the serial loop.  A member that is not positive definite even with jitter is a wall
        (1e10, zero gradient)."""
        k, nls = xs.shape[0], self.kern.lengthscale.size
        var, ls, noise = np.empty(k), np.empty((k, nls)), np.empty(k)
        Xw = np.empty((k,) + self.X_untransformed.shape)
        for j in range(k):
            self.optimizer_array = xs[j]
            var[j], ls[j], noise[j] = float(self.kern.variance), self.kern.lengthscale.values, float(self.likelihood.variance)
            Xw[j] = self.transform_data(self.X_untransformed)
        (lml, _, _), (dv, dl, dn), dL_dX, status = self._h.fit_grad_x_batch(Xw, var, ls, noise, self.max_jitter_tries)
        f, g = np.empty(k), np.zeros_like(xs)
        for j in range(k):
            if status[j] != 0:
                f[j] = 1e10
                continue
            self.optimizer_array = xs[j]     # (update_grads, the priors and the chain-rule factors are taken at this member's parameters)
            self.warping_function.update_grads(self.X_untransformed, dL_dX[j])
            natural = [(self.kern.variance, dv[j]), (self.kern.lengthscale, dl[j]), (self.likelihood.variance, dn[j])]
            natural.extend((p, p.gradient.copy()) for p in self.warping_function.flattened_parameters())
            f[j] = self._objective_value(lml[j])
            g[j] = -self._transform_gradients(self._natural_with_priors(natural))
        return f, g

    # -- prediction ---------------------------------------------------------------------
    def _stage(self, Xnew, fit=True):
        Xnew = np.asarray(Xnew, dtype=float)
        if Xnew.ndim == 1:
            Xnew = Xnew[None, :]
        if fit:
            self._ensure_fit()
        elif self._dirty:
            self._push_params()      # (a pending re-warp of the training inputs precedes the fused fit + predict)
        if Xnew.shape[0] > _FEW and isinstance(self.warping_function, KumarWarping):
            self._h.set_candidates_kumar(Xnew, *self.warping_function.device_arguments(self.input_dim))
        else:
            self._h.set_candidates(self.transform_data(Xnew, test_data=True))
        return Xnew

    def _few_rows(self, Xnew, limit=_FEW):
        few = super(InputWarpedGP, self)._few_rows(Xnew, limit)
        return None if few is None else self.transform_data(few, test_data=True)

    def warp_jacobian(self, Xnew):
        """d w(x) / dx at the rows of ``Xnew`` [M, D]: ``fgrad_X(Xnew, test_data=True)`` on the warped columns, 1 on the
        columns that pass through."""
        Xnew = np.atleast_2d(np.asarray(Xnew, dtype=float))
        J = np.ones(Xnew.shape)
        idx = list(getattr(self.warping_function, "warping_indices", range(Xnew.shape[1])))
        J[:, idx] = self.warping_function.fgrad_X(Xnew, test_data=True)[:, idx]
        return J

    def predictive_gradients(self, Xnew, kern=None):
        """(dmu_dX [M, D, P], dv_dX [M, D]) with respect to the un-warped ``Xnew``."""
        dm, dv = super(InputWarpedGP, self).predictive_gradients(Xnew, kern)
        if dm.shape[0] == 0:
            return dm, dv
        J = self.warp_jacobian(Xnew)
        return dm * J[:, :, None], dv * J

    def mean_gradients(self, Xnew):
        dm = super(InputWarpedGP, self).mean_gradients(Xnew)
        return dm if dm.shape[0] == 0 else dm * self.warp_jacobian(Xnew)[:, :, None]

    def _device_group(self, devices):
        raise NotImplementedError("replica groups score un-warped candidate tables: outside the input-warped path")


class InputWarpedGPModel(BOModel):
    """Bayesian optimisation surrogate: ``InputWarpedGP`` with Kumaraswamy warping of every continuous and discrete variable
    of ``space``, in order (input_warped_gpmodel.py:9-88).  Constructor keywords are the reference's plus ``device``; default
    kernel Matern-5/2; noise as ``GPModel`` sets it up.  ``predict`` returns (mean, std) with the variance floored at 1e-10.
    ``parallel_restarts=True`` (an addition, default False) runs the hyper-parameter restarts of ``updateModel`` in lockstep
    (``optimize_restarts(parallel=True)``), as ``GPModel`` does.

    Not a ``GPModel``: the device acquisition entries would score un-warped locations, so the acquisitions take their host
    adapter over ``predict`` / ``predict_withGradients``.

    Two deviations from the reference.  ``predict_withGradients`` is available (``analytical_gradient_prediction = True``;
    the reference sets it False and optimises the acquisition without gradients).  ``Xmin`` / ``Xmax`` are the design space's
    bounds, not the training set's extremes (input_warped_gpmodel.py:82): with the reference's choice every candidate outside
    the training hull warps to NaN."""
    analytical_gradient_prediction = True

    def __init__(self, space, warping_function=None, kernel=None, noise_var=None, exact_feval=False, optimizer='bfgs',
                 max_iters=1000, optimize_restarts=5, verbose=False, ARD=False, device=0, parallel_restarts=False):
        self.space = space
        self.warping_indices = warping_indices_of(space)
        vars(self).update(warping_function=warping_function, kernel=kernel, noise_var=noise_var, exact_feval=exact_feval,
                          optimizer=optimizer, max_iters=max_iters, optimize_restarts=optimize_restarts, verbose=verbose,
                          ARD=ARD, device=device, model=None, parallel_restarts=bool(parallel_restarts))

    def _create_model(self, X, Y):
        self.input_dim = X.shape[1]
        if self.kernel is None:
            self.kernel = _kern.Matern52(self.input_dim, variance=1., ARD=self.ARD)
        noise = 0.01 * Y.var() if self.noise_var is None else self.noise_var
        bounds = np.asarray(self.space.get_bounds(), dtype=float)
        gp = InputWarpedGP(X, Y, kernel=self.kernel, warping_function=self.warping_function,
                           warping_indices=self.warping_indices, Xmin=bounds[:, 0], Xmax=bounds[:, 1], device=self.device)
        gp.Gaussian_noise.variance.set(noise)
        if self.exact_feval:
            gp.Gaussian_noise.constrain_fixed(1e-6, warning=False)
        else:
            gp.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
        self.model = gp

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        if self.model is None:
            self._create_model(X_all, Y_all)
        else:
            self.model.set_XY(X_all, Y_all)
        if self.max_iters <= 0:
            return
        search = dict(optimizer=self.optimizer, max_iters=self.max_iters)
        if self.optimize_restarts == 1:
            self.model.optimize(messages=False, ipython_notebook=False, **search)
        else:
            if self.parallel_restarts:   # the restarts in lockstep, one gp_fit_grad_x_batch per round (InputWarpedGP._batch_objective)
                search["parallel"] = True
            self.model.optimize_restarts(num_restarts=self.optimize_restarts, verbose=self.verbose, **search)

    def predict(self, X, with_noise=True):
        mean, var = self.model.predict(np.atleast_2d(X), include_likelihood=with_noise)
        return mean, np.sqrt(np.maximum(var, _VAR_FLOOR))

    def get_fmin(self):
        """Smallest posterior mean over the training inputs, evaluated on the device and cached per fit."""
        gp = self.model
        gp._ensure_fit()
        lowest = gp._h.fmin()
        if gp.normalizer is not None:
            lowest = float(gp.normalizer.inverse_mean(np.array([[lowest]]))[0, 0])
        return lowest

    def predict_withGradients(self, X):
        """(mean, std, d mean / dx, d std / dx), the gradients with respect to the un-warped ``X``."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        gp = self.model
        few = gp._few_rows(X)
        if few is not None:     # posterior and gradients of a handful of (host-warped) locations in ONE device call
            mean, var, jac_mean, jac_var = gp._h.predict_rows(few, include_noise=True, grad=True)
            J = gp.warp_jacobian(X)
            jac_mean, jac_var = jac_mean * J[:, :, None], jac_var * J
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

    def get_model_parameters(self):
        return np.atleast_2d(self.model[:])

    def get_model_parameters_names(self):
        return self.model.parameter_names_flat().tolist()


def warping_indices_of(space):
    """The input columns of every continuous and discrete variable of ``space``, in order (input_warped_gpmodel.py:50-57)."""
    types = getattr(space, "types", None)
    if types is not None:
        return [i for i, t in enumerate(types) if t in ('continuous', 'discrete')]
    out, i = [], 0
    for var in space.space:
        for _ in range(var.dimensionality):
            if var.type in ('continuous', 'discrete'):
                out.append(i)
            i += 1
    return out
