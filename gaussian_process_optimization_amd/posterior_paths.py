"""Samples of the posterior FUNCTION by pathwise conditioning (Wilson et al., "Efficiently sampling functions from Gaussian
process posteriors", ICML 2020) -- an addition with no counterpart in the reference, whose ``posterior_samples_f`` factors the
M x M covariance of a table and whose Thompson batch draws independent marginals.  A path

    f_s(x) = a sum_j w_js cos(omega_j^T x + b_j)  +  sum_n k(x, X_n) V_ns,        a = sqrt(2 variance / F)
    V_s = (K + d I)^-1 (y - Phi(X) w_s - eps_s),   eps_s = sqrt(d) z_s,   d = noise + 1e-8 + jitter of the fit

can be evaluated anywhere, differentiated and minimised.  The first term is a random-Fourier-feature draw from the prior, the
second an exact update through the factor the fit left on the device: only the prior is approximate, the data are interpolated
whatever F is.  All arithmetic runs on the device (include/gphip.h, gp_paths_*); this module draws the hyper-parameter-free
random numbers and keeps the book on which fit the resident paths belong to.
"""
import numpy as np

from . import _lib

# the covariance families by the library's ids: nu of the Matern family (None: the squared exponential, nu -> infinity)
_NU = {_lib.GP_KERNEL_RBF: None, _lib.GP_KERNEL_MATERN52: 2.5, _lib.GP_KERNEL_MATERN32: 1.5, _lib.GP_KERNEL_EXPONENTIAL: 0.5}
_NAMES = {"rbf": _lib.GP_KERNEL_RBF, "expquad": _lib.GP_KERNEL_RBF, "mat52": _lib.GP_KERNEL_MATERN52,
          "matern52": _lib.GP_KERNEL_MATERN52, "mat32": _lib.GP_KERNEL_MATERN32, "matern32": _lib.GP_KERNEL_MATERN32,
          "exponential": _lib.GP_KERNEL_EXPONENTIAL, "ou": _lib.GP_KERNEL_EXPONENTIAL}


def kernel_id(kernel):
    """The library's id of ``kernel``: a ``kern`` object, one of the ids, or a family name."""
    if hasattr(kernel, "_kernel_id"):
        return int(kernel._kernel_id)
    if isinstance(kernel, str):
        if kernel.lower() not in _NAMES:
            raise ValueError("unknown covariance family %r" % kernel)
        return _NAMES[kernel.lower()]
    if int(kernel) not in _NU:
        raise ValueError("unknown kernel id %r" % (kernel,))
    return int(kernel)


def unit_frequencies(kernel, D, F, rng):
    """F frequencies [F, D] from the spectral density of the unit-lengthscale, unit-variance kernel: z ~ N(0, I) for the squared
    exponential; for Matern-nu (5/2, 3/2, and 1/2 = Exponential / OU) the multivariate t with 2 nu degrees of freedom,
    z sqrt(2 nu / g) with g ~ chi^2(2 nu).  E cos(omega^T delta) = k(delta) / variance.  An ARD model divides column d by its
    lengthscale afterwards (the device does, from the resident parameters)."""
    nu = _NU[kernel_id(kernel)]
    z = rng.standard_normal((int(F), int(D)))
    if nu is None:
        return z
    g = rng.chisquare(2.0 * nu, size=int(F))
    return z * np.sqrt(2.0 * nu / g)[:, None]


def draw(kernel, N, D, S, F, seed=None):
    """The four arrays of ``Handle.paths_set`` for S paths of F features over N observations in D dimensions, none of which
    depends on a hyper-parameter: (omega_unit [F, D], phase [F] in [0, 2 pi), w [S, F], z_eps [S, N])."""
    rng = np.random.default_rng(seed)
    omega = unit_frequencies(kernel, D, F, rng)
    phase = rng.uniform(0.0, 2.0 * np.pi, int(F))
    w = rng.standard_normal((int(S), int(F)))
    z = rng.standard_normal((int(S), int(N)))
    return omega, phase, w, z


def check_model(model):
    """What the paths need of a ``GPRegression``: the exact single-output model with a Euclidean covariance and no mean function.
    Everything else is refused before anything reaches the device."""
    if not getattr(type(model), "_appendable", False):
        raise NotImplementedError("posterior paths are defined for the exact GPRegression, not for %s" % type(model).__name__)
    if model.output_dim != 1:
        raise NotImplementedError("posterior paths need a single-output model (got %d outputs)" % model.output_dim)
    if model._uses_gower():
        raise NotImplementedError("posterior paths: a Gower kernel has no spectral density to draw frequencies from")
    if model.mean_function is not None:
        raise NotImplementedError("posterior paths do not take a mean function")


def fit_signature(model):
    """What a fit of ``model`` is a function of: the paths of one signature are not the paths of another."""
    k = model.kern
    return (model._data_epoch, int(k._kernel_id), bool(k.ARD), float(k.variance), tuple(np.ravel(k.lengthscale.values).tolist()),
            float(model.likelihood.variance))


class PosteriorPaths(object):
    """``size`` posterior function samples of ``model``, resident on its device.  Valid for the fit they were drawn for: after new
    hyper-parameters, new data or an append every method raises ``RuntimeError`` -- draw new ones (``model.posterior_paths``).

    :param draws: the four arrays of :func:`draw` (reproducible paths; ``size`` and ``num_features`` are then theirs)
    """

    def __init__(self, model, size=10, num_features=1024, seed=None, draws=None):
        check_model(model)
        model._ensure_fit()
        if draws is None:
            if not 1 <= int(size) <= _lib.GP_PATHS_MAX_S:
                raise ValueError("between 1 and %d paths, got %r" % (_lib.GP_PATHS_MAX_S, size))
            if not 1 <= int(num_features) <= _lib.GP_PATHS_MAX_F:
                raise ValueError("between 1 and %d features, got %r" % (_lib.GP_PATHS_MAX_F, num_features))
            draws = draw(model.kern, model.num_data, model.input_dim, size, num_features, seed)
        self.draws = tuple(np.asarray(a, dtype=float) for a in draws)
        self.size, self.num_features = self.draws[2].shape
        self.model = model
        self.signature = fit_signature(model)
        self._key = (id(self), self.signature)
        model._h.paths_set(*self.draws, key=self._key)

    def _normaliser(self):
        n = self.model.normalizer
        if n is None:
            return 0.0, 1.0
        return float(np.ravel(n.mean)[0]), float(np.ravel(n.std)[0])

    def _check(self):
        m = self.model
        if m._dirty or fit_signature(m) != self.signature or m._h.paths_key != self._key:
            raise RuntimeError("these posterior paths were drawn for another fit of the model (its hyper-parameters or data "
                               "changed, or other paths replaced them): call posterior_paths() again")

    def _locations(self, X):
        X = np.atleast_2d(np.asarray(X, dtype=float))
        if X.shape[1] != self.model.input_dim:
            raise ValueError("locations have %d columns, the model has %d" % (X.shape[1], self.model.input_dim))
        return X

    def __call__(self, X):
        """Every path at the rows of ``X``: [M, size], in the units of Y (the normaliser undone, as ``posterior_samples_f``
        undoes it).  Up to 8 rows go by value, more through a table."""
        self._check()
        X = self._locations(X)
        y_mean, y_std = self._normaliser()
        h = self.model._h
        M = X.shape[0]
        if M == 0:
            return np.empty((0, self.size))
        if M <= _lib.GP_PATHS_MAX_ROWS:
            out = np.empty((M, self.size))
            per = max(1, _lib.GP_PATHS_MAX_ROWS // M)      # whole copies of X per call, each on a path of its own
            for s0 in range(0, self.size, per):
                ss = np.arange(s0, min(s0 + per, self.size))
                v = h.paths_rows(np.tile(X, (ss.size, 1)), np.repeat(ss, M), y_mean, y_std)
                out[:, ss] = v.reshape(ss.size, M).T
            return out
        h.set_candidates(X)
        return np.ascontiguousarray(h.paths_table(y_mean, y_std).T)

    def value_and_gradient(self, X, path=0):
        """(f [M], df/dx [M, D]) of up to 8 locations; ``path`` one index for all rows or one per row."""
        self._check()
        X = self._locations(X)
        y_mean, y_std = self._normaliser()
        return self.model._h.paths_rows(X, path, y_mean, y_std, grad=True)

    def argmin(self, X):
        """Per path the row of ``X`` with the smallest value, reduced on the device: (idx [size], val [size])."""
        self._check()
        X = self._locations(X)
        y_mean, y_std = self._normaliser()
        self.model._h.set_candidates(X)
        return self.model._h.paths_argbest(-1, y_mean, y_std)
