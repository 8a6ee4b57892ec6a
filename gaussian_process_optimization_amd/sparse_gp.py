"""``SparseGPRegression`` -- host mirror of ``GPy.models.SparseGPRegression`` backed by libgphip's sparse entry points.

Reference: GPy/GPy/models/sparse_gp_regression.py:33-66 (constructor: default kernel RBF, default Z a random subset of X,
Gaussian likelihood of variance 1), GPy/GPy/core/sparse_gp.py:41-119 (Z as the parameter linked at index 0, ``set_Z``,
``parameters_changed`` / ``_update_gradients``), GPy/GPy/inference/latent_function_inference/var_dtc.py:66-277 (the inference),
posterior.py:225-248 (prediction through ``woodbury_inv``), GPy/GPy/core/gp.py:407-454 (``predictive_gradients`` over
``_predictive_variable = Z``).

All numerics run on the device (include/gphip.h, "sparse GP"): ``gp_sparse_fit_grad`` once per objective evaluation -- or one
``gp_sparse_fit_grad_batch`` per round of evaluations of all restarts, ``optimize_restarts(parallel=True)`` --,
``gp_sparse_predict`` per prediction.  This module is bookkeeping: the flat parameter vector [Z row-major, kern.variance,
kern.lengthscale, Gaussian_noise.variance] with Z unconstrained, the Y normaliser, lazy refits.  Homoscedastic noise, certain
inputs, no mean function.  The joint posterior -- ``full_cov``, ``posterior_samples_f``, ``posterior_covariance_between_points`` --
comes from ``gp_sparse_predict_full_cov``, ``gp_sparse_posterior_samples`` and ``gp_sparse_cov_between``.
"""
import numpy as np

from . import kern as _kern
from .gp_regression import GPRegression
from .parameterization import Param

MAX_INDUCING = 2048     # GP_SPARSE_MAX_INDUCING (include/gphip.h)
BATCH_MAX_R = 64                # gp_sparse_fit_grad_batch's limit on the members
BATCH_MAX_BYTES = 16 << 30      # GP_SPARSE_BATCH_MAX_BYTES
LOCKSTEP_MAX_INDUCING = MAX_INDUCING   # profiles/sparse_restarts_timing.txt excludes nothing (see _lockstep_applies)


class Identity(object):
    """The transform of an unconstrained parameter."""

    def f(self, x):
        return np.asarray(x, dtype=float)

    def finv(self, f):
        return np.asarray(f, dtype=float)

    def gradfactor(self, f, df):
        return df


class _SparsePosteriorView(object):
    """The fields of GPy's Posterior a sparse model serves (posterior.py:9-270): woodbury_vector [Mz, P], woodbury_inv [Mz, Mz]."""

    def __init__(self, model):
        self._m = model

    @property
    def woodbury_vector(self):
        self._m._ensure_fit()
        return self._m._h.sparse_posterior()[0]

    @property
    def woodbury_inv(self):
        self._m._ensure_fit()
        return self._m._h.sparse_posterior()[1]


class SparseGPRegression(GPRegression):
    """Sparse GP regression by variational DTC over ``num_inducing`` inducing inputs, on one MI355X.

    :param X: input observations [N, D]
    :param Y: observed values [N, P]
    :param kernel: one of the ``kern.Stationary`` classes (defaults to RBF, sparse_gp_regression.py:37-38)
    :param Z: inducing inputs [Mz, D]; default ``X[np.random.permutation(N)[:min(num_inducing, N)]]`` (the global NumPy
              generator, as the reference, :41-43)
    :param normalizer: ``True`` standardises Y
    :param device: HIP device ordinal

    The Gaussian noise starts at 1.  ``Z`` is the parameter ``inducing_inputs``, first in the flat vector and unconstrained.

    ``device_rows`` (attribute, default False; ``GPModel(sparse=True, device_acquisitions=True)`` sets it): predictions and
    predictive gradients of up to eight locations of a single-output model go down as ONE ``gp_sparse_predict_rows`` call, locations
    by value, instead of ``gp_sparse_predict``.  Same results to rounding, not bitwise."""
    device_rows = False

    _appendable = False    # append_XY refits: the fit of this model is more than the exact GP's factor of (X, Y)
    _takes_mean_function = False   # the sparse entries do not carry a mean function

    def __init__(self, X, Y, kernel=None, Z=None, num_inducing=10, normalizer=None, device=0, name="sparse_gp", mean_function=None):
        X = np.asarray(X, dtype=float)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if kernel is None:
            kernel = _kern.RBF(X.shape[1])
        if Z is None:
            i = np.random.permutation(X.shape[0])[:min(num_inducing, X.shape[0])]
            Z = X.view(np.ndarray)[i].copy()
        else:
            Z = np.array(Z, dtype=float)
            assert Z.ndim == 2 and Z.shape[1] == X.shape[1]
        if getattr(kernel, "Gower", False) and getattr(kernel, "space", None) is not None:
            raise NotImplementedError("the sparse GP does not take the Gower kernel")
        self.Z = None
        self._table = None          # the candidate table resident in the sparse model's own block (_stage_table)
        self._points = None         # the second point set resident for posterior_covariance_between_points (_stage_points)
        super(SparseGPRegression, self).__init__(X, Y, kernel=kernel, normalizer=normalizer, noise_var=1., mean_function=mean_function,
                                                 device=device, name=name)
        self.posterior = _SparsePosteriorView(self)
        self._link_Z(Z)

    # -- the inducing inputs ------------------------------------------------------------
    def _link_Z(self, Z):
        Z = np.asarray(Z, dtype=float)
        if Z.ndim != 2 or Z.shape[1] != self.input_dim:
            raise ValueError("Z needs %d columns, got shape %s" % (self.input_dim, Z.shape))
        if not (1 <= Z.shape[0] <= MAX_INDUCING):
            raise ValueError("the number of inducing inputs must lie in 1..%d, got %d" % (MAX_INDUCING, Z.shape[0]))
        self.Z = Param("inducing_inputs", Z, Identity())
        self.Z._parent = self
        self.num_inducing = Z.shape[0]
        self._dirty = True

    def set_Z(self, Z, trigger_update=True):
        """sparse_gp.py:69-74: a new set of inducing inputs (their number may change)."""
        self._link_Z(Z)

    @property
    def Z_values(self):
        """The inducing inputs as an [Mz, D] array."""
        return self.Z.values.reshape(self.num_inducing, self.input_dim)

    @property
    def _predictive_variable(self):
        return self.Z_values

    def flattened_parameters(self):
        """Z is linked at index 0 (sparse_gp.py:59): [Z, kern.variance, kern.lengthscale, Gaussian_noise.variance]."""
        rest = super(SparseGPRegression, self).flattened_parameters()
        return rest if self.Z is None else [self.Z] + rest

    def parameter_names_flat(self):
        names = super(SparseGPRegression, self).parameter_names_flat()
        if self.Z is None:
            return names
        own = ["%s.%s[[%d]]" % (self.name, self.Z.name, i) for i in range(self.Z.size)]
        return np.array(own + list(names))

    # -- (re)fit ------------------------------------------------------------------------
    def _push_params(self):
        k = self.kern
        if k.Gower and k.space is not None:
            raise NotImplementedError("the sparse GP does not take the Gower kernel")
        self._h.set_gower()
        self._h.set_params(k._kernel_id, k.ARD, float(k.variance), k.lengthscale.values, float(self.likelihood.variance))
        self._h.sparse_set_inducing(self.Z_values)

    def _ensure_fit(self):
        """SparseGP.parameters_changed (sparse_gp.py:76-81): inference on the device when anything changed."""
        if not self._dirty:
            return
        self._push_params()
        self._lml, self._jitter, self._jitter_b = self._h.sparse_fit(self.max_jitter_tries)
        self._logdet = None
        self._dirty = False

    def _log_likelihood_gradients_natural(self):
        """One gp_sparse_fit_grad per evaluation: the LML of this parameter vector is left behind for ``objective_function``."""
        nls = self.kern.lengthscale.size
        self._push_params()
        self._lml, (dv, dl, dn, dZ) = self._h.sparse_fit_grad(nls, self.max_jitter_tries)
        self._dirty = False
        self.Z.gradient = dZ.reshape(-1)
        self.kern.variance.gradient = np.atleast_1d(dv)
        self.kern.lengthscale.gradient = dl
        self.likelihood.variance.gradient = np.atleast_1d(dn)
        return [(self.Z, dZ.reshape(-1)), (self.kern.variance, dv), (self.kern.lengthscale, dl), (self.likelihood.variance, dn)]

    def _uses_gower(self):
        return False

    def _batch_objective(self, xs):
        """``_obj_grad`` for every row of ``xs`` from ONE gp_sparse_fit_grad_batch: each member's Z, variance, lengthscale(s) and
        noise through the transforms (fixed / bounded noise included), the natural gradients back through the chain rule in the
        order of ``flattened_parameters()`` (Z first).  A member whose ladders end without a factor is a wall (1e10, zero
        gradient), as in ``_obj_grad``.  The resident inducing inputs and sparse fit are left alone."""
        k, nls = xs.shape[0], self.kern.lengthscale.size
        Z = np.empty((k, self.num_inducing, self.input_dim))
        var, ls, noise = np.empty(k), np.empty((k, nls)), np.empty(k)
        for j in range(k):
            self.optimizer_array = xs[j]
            Z[j] = self.Z_values
            var[j], ls[j], noise[j] = float(self.kern.variance), self.kern.lengthscale.values, float(self.likelihood.variance)
        (lml, _, _), (dv, dl, dn, dZ), status = self._h.sparse_fit_grad_batch(Z, var, ls, noise, self.max_jitter_tries)
        f, g = np.empty(k), np.zeros_like(xs)
        for j in range(k):
            if status[j] != 0:
                f[j] = 1e10
                continue
            self.optimizer_array = xs[j]     # (the priors and the chain-rule factors are taken at this member's parameters)
            natural = [(self.Z, dZ[j].reshape(-1)), (self.kern.variance, dv[j]), (self.kern.lengthscale, dl[j]),
                       (self.likelihood.variance, dn[j])]
            f[j] = self._objective_value(lml[j])
            g[j] = -self._transform_gradients(self._natural_with_priors(natural))
        return f, g

    def _lockstep_applies(self, num_restarts):
        """``optimize_restarts(parallel=True)`` runs the restarts in lockstep, one gp_sparse_fit_grad_batch per round of L-BFGS
        steps, for 1..64 restarts of a non-empty optimiser vector whose batch buffers (``gp_sparse_batch_bytes``) stay within
        GP_SPARSE_BATCH_MAX_BYTES; otherwise the serial loop runs.  LOCKSTEP_MAX_INDUCING would narrow it to the numbers of
        inducing inputs at which profiles/sparse_restarts_timing.txt shows the R = 5 batch call faster than five single calls:
        the record's rows "Mz 10 / 128 / 512 / 1024 / 2048, R 5" read 4.88x / 4.79x / 2.78x / 1.80x / 1.52x (N = 16384, D = 8), so
        nothing up to the cap on Mz is excluded."""
        if not (1 <= num_restarts <= BATCH_MAX_R and self.optimizer_array.size > 0):
            return False
        if self.num_inducing > LOCKSTEP_MAX_INDUCING:
            return False
        self._push_params()      # (the byte count is taken over the data and parameters the context holds)
        self._dirty = True
        return self._h.sparse_batch_bytes(num_restarts, self.num_inducing) <= BATCH_MAX_BYTES

    def _device_group(self, devices):
        raise NotImplementedError("replica groups score the exact GP: outside the sparse path")

    # -- prediction ---------------------------------------------------------------------
    def _rows_route(self, Xnew, limit=8):
        """True when ``Xnew`` [M, D] is a handful of locations that ``device_rows`` sends down by value."""
        return bool(self.device_rows) and self.output_dim == 1 and 1 <= Xnew.shape[0] <= limit

    def _sparse_predict(self, Xnew, include_noise, grad=False):
        Xnew = np.asarray(Xnew, dtype=float)
        if Xnew.ndim == 1:
            Xnew = Xnew[None, :]
        if Xnew.shape[1] != self.input_dim:
            raise ValueError("candidates have %d columns, model has %d" % (Xnew.shape[1], self.input_dim))
        self._ensure_fit()
        if self._rows_route(Xnew):
            return self._h.sparse_predict_rows(Xnew, include_noise=include_noise, grad=grad)
        return self._h.sparse_predict(Xnew, include_noise=include_noise, grad=grad)

    def _stage_table(self, Xnew):
        """Make ``Xnew`` the sparse model's resident candidate table (gp_sparse_set_candidates), refitting first if anything
        changed.  The same table staged again -- every round of the local-penalisation loop -- is not uploaded again: the device
        keeps it, and its cached posterior, across refits, predictions and rows calls."""
        Xnew = np.asarray(Xnew, dtype=float)
        if Xnew.ndim == 1:
            Xnew = Xnew[None, :]
        self._ensure_fit()
        held = self._table
        if held is None or held[0] is not self._h or held[1].shape != Xnew.shape or not np.array_equal(held[1], Xnew):
            self._h.sparse_set_candidates(Xnew)
            self._table = (self._h, np.array(Xnew, copy=True))
        return Xnew

    def _stage_points(self, X1):
        """Make ``X1`` the resident second point set (gp_sparse_cov_set_points), refitting first if anything changed.  The same
        points staged again -- entropy search's representers, once per candidate block -- are not uploaded again: the device keeps
        them across refits and rebuilds what it derives from them."""
        self._ensure_fit()
        held = self._points
        if held is None or held[0] is not self._h or held[1].shape != X1.shape or not np.array_equal(held[1], X1):
            self._joint_entry("sparse_cov_set_points")(X1)
            self._points = (self._h, np.array(X1, copy=True))

    def _joint_entry(self, name):
        """The handle's method ``name`` of the joint posterior; a handle that does not offer it cannot serve the call."""
        entry = getattr(self._h, name, None)
        if entry is None:
            raise NotImplementedError("this handle does not serve the sparse joint posterior (%s)" % name)
        return entry

    def _joint_rows(self, Xnew):
        Xnew = np.asarray(Xnew, dtype=float)
        if Xnew.ndim == 1:
            Xnew = Xnew[None, :]
        if Xnew.shape[1] != self.input_dim:
            raise ValueError("candidates have %d columns, model has %d" % (Xnew.shape[1], self.input_dim))
        self._ensure_fit()
        return Xnew

    def _raw_predict(self, Xnew, full_cov=False, kern=None):
        """posterior.py:225-248 over the inducing inputs."""
        if kern is not None and kern is not self.kern:
            raise NotImplementedError("prediction with a foreign kernel is outside the accelerated path")
        e = self._empty(Xnew, full_cov)
        if e is not None:
            return e
        if full_cov:
            return self._joint_entry("sparse_predict_full_cov")(self._joint_rows(Xnew), include_noise=False)
        return self._sparse_predict(Xnew, False)

    def predict(self, Xnew, full_cov=False, Y_metadata=None, kern=None, likelihood=None, include_likelihood=True):
        """gp.py:297-354 on the sparse posterior."""
        if kern is not None and kern is not self.kern:
            raise NotImplementedError("prediction with a foreign kernel is outside the accelerated path")
        e = self._empty(Xnew, full_cov)
        if e is not None:
            return e
        if full_cov:
            mean, var = self._joint_entry("sparse_predict_full_cov")(self._joint_rows(Xnew), include_noise=include_likelihood)
        else:
            mean, var = self._sparse_predict(Xnew, include_likelihood)
        if self.normalizer is not None:
            mean = self.normalizer.inverse_mean(mean)
            if full_cov and mean.shape[1] > 1:
                var = self.normalizer.inverse_covariance(var)
            else:
                var = self.normalizer.inverse_variance(var)
        return mean, var

    def predictive_gradients(self, Xnew, kern=None):
        """gp.py:407-454 over ``_predictive_variable = Z``: (dmu_dX [M, D, P], dv_dX [M, D])."""
        Xn = np.asarray(Xnew, dtype=float)
        if Xn.ndim == 2 and Xn.shape[0] == 0:
            return np.empty((0, self.input_dim, self.output_dim)), np.empty((0, self.input_dim))
        return self._sparse_predict(Xnew, False, grad=True)[2:]

    def mean_gradients(self, Xnew):
        Xn = np.asarray(Xnew, dtype=float)
        if Xn.ndim == 1:
            Xn = Xn[None, :]
        if Xn.ndim == 2 and Xn.shape[0] >= 1 and Xn.shape[1] == self.input_dim and self._rows_route(Xn):
            self._ensure_fit()      # d mean / dx alone: the woodbury vector only, no pass over woodbury_inv (estimate_L's inner call)
            return self._h.sparse_mean_grad_rows(Xn)
        return self.predictive_gradients(Xnew)[0]

    def get_fmin(self):
        """min over the training inputs of the posterior mean, first output (gp_sparse_fmin), in the normalised space."""
        self._ensure_fit()
        return self._h.sparse_fmin()

    def posterior_covariance_between_points(self, X1, X2):
        """The off-diagonal block of the full posterior covariance (posterior.py:229-232 over ``_predictive_variable = Z``) of the
        stacked points, K(X1, X2) - K(X1, Z) woodbury_inv K(Z, X2), in the model's (normalised) output space: what
        ``GPRegression.posterior_covariance_between_points`` defines.  (The reference's own method, gp.py:714-721, hands the
        training inputs to a factor that is Mz x Mz: a shape error unless N = Mz.)  ``X1`` is made resident and kept while it
        stays the same, bit for bit; ``X2`` travels: one ``gp_sparse_cov_between`` per call."""
        X1 = self._joint_rows(np.atleast_2d(np.asarray(X1, dtype=float)))
        X2 = self._joint_rows(np.atleast_2d(np.asarray(X2, dtype=float)))
        if X1.shape[0] == 0 or X2.shape[0] == 0:
            return np.empty((X1.shape[0], X2.shape[0]))
        self._stage_points(X1)
        return np.ascontiguousarray(self._joint_entry("sparse_cov_between")(X2).T)

    def posterior_samples_f(self, X, size=10, normals=None, **kw):
        """gp.py:581-609 on the sparse posterior: draws of the latent function at X, [Nnew, output_dim, size], with the semantics of
        ``GPRegression.posterior_samples_f`` -- ``normals`` [output_dim, size, Nnew] for reproducible draws,
        ``posterior_samples_jitter_``, LinAlgError on an exhausted ladder, the normaliser's std on the deviations."""
        X = self._joint_rows(np.atleast_2d(np.asarray(X, dtype=float)))
        M, P = X.shape[0], self.output_dim
        if normals is None:
            normals = np.random.standard_normal((P, size, M))
        normals = np.asarray(normals, dtype=float).reshape(P, size, M)
        m, dev, self.posterior_samples_jitter_ = self._joint_entry("sparse_posterior_samples")(
            X, normals.reshape(P * size, M), include_noise=False, maxtries=self.max_jitter_tries)
        dev = dev.reshape(P, size, M)
        if self.normalizer is not None:
            m = self.normalizer.inverse_mean(m)
            dev = dev * np.asarray(self.normalizer.std, dtype=float).reshape(-1, 1, 1)
        fsim = np.empty((M, P, size))
        for d in range(P):
            fsim[:, d, :] = m[:, d:d + 1] + dev[d].T
        return fsim
