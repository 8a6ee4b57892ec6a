"""Host-side kernel descriptors mirroring ``GPy.kern.RBF`` (alias ``ExpQuad``), ``Matern52``, ``Matern32``
and ``Exponential`` (twin ``OU``).

Reference: GPy/GPy/kern/src/stationary.py:23-82 (Stationary.__init__: variance,
lengthscale, ARD), rbf.py:12-57 (RBF), stationary.py:546-579 (Matern52), :447-482
(Matern32), :384-392 (Exponential), :427-444 (OU).  The fork's ``Gower=`` / ``space=``
arguments exist on RBF and Matern52 only, as in the reference tree.  These
objects only *hold* hyper-parameters; every covariance evaluation happens on
the GPU inside libgphip (kbuild.hip).  ``K``/``Kdiag`` are provided for API
parity and run through the device as well.
"""
import numpy as np

from . import _lib
from .parameterization import Param, Parameterized


class Stationary(Parameterized):
    _kernel_id = None
    _takes_gower = True      # the constructor has the fork's Gower= / space= arguments (RBF, Matern52)

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="stationary",
                 Gower=False, space=None):
        super(Stationary, self).__init__(name)
        # the fork's mixed-variable option (stationary.py:61-65): product of 1-D kernels over the variables of `space`
        self.Gower = bool(Gower)
        self.space = space
        self.input_dim = int(input_dim)
        if active_dims is not None and list(active_dims) != list(range(self.input_dim)):
            raise NotImplementedError("active_dims slicing is outside the accelerated path")
        self.ARD = bool(ARD)
        # stationary.py:66-79
        if not ARD:
            if lengthscale is None:
                lengthscale = np.ones(1)
            else:
                lengthscale = np.asarray(lengthscale, dtype=float).reshape(-1)
                assert lengthscale.size == 1, "Only 1 lengthscale needed for non-ARD kernel"
        else:
            if lengthscale is not None:
                lengthscale = np.asarray(lengthscale, dtype=float).reshape(-1)
                assert lengthscale.size in [1, input_dim], "Bad number of lengthscales"
                if lengthscale.size != input_dim:
                    lengthscale = np.ones(input_dim) * lengthscale
            else:
                lengthscale = np.ones(self.input_dim)
        self.variance = Param("variance", np.atleast_1d(float(variance)))
        self.lengthscale = Param("lengthscale", lengthscale)
        assert self.variance.size == 1
        self.link_parameters(self.variance, self.lengthscale)

    # -- device-backed evaluations (API parity; not used by the fit/predict path) ------
    def K(self, X, X2=None):
        """kern.K(X[, X2]) -- stationary.py:107-140, evaluated by the K-build kernels (kern.py:119 is the contract:
        X2 None -> K(X, X) with the diagonal forced to the variance, X2 given -> the [N, M2] cross covariance)."""
        # one scratch context per DEVICE for the whole process (not per kernel object: a kernel holds hyper-parameters only,
        # so it deep-copies and pickles like the reference's; a loop over kern.K still pays no context creation per call)
        h = _scratch_handle(int(getattr(self, "_device", 0)))
        X = _lib.as_f64(X, 2)
        h.set_data(X, np.zeros((X.shape[0], 1)))
        # the scratch context is shared: a Gower set-up left by another kernel goes off BEFORE the parameters go in (the device
        # refuses Matern32 / Exponential while it is on), a new one goes on AFTER them
        gower = self.Gower and self.space is not None
        if not gower:
            h.set_gower()
        h.set_params(self._kernel_id, self.ARD, float(self.variance), self.lengthscale.values, 0.0)
        if gower:
            h.set_gower(*gower_config(self.space, self.input_dim))
        out = h.kernel_matrix() if X2 is None else h.cross_kernel_matrix(X2)
        if X.shape[0] > _SCRATCH_KEEP_N:      # an N x N device buffer of gigabytes is not kept alive behind the caller's back
            release_scratch(int(getattr(self, "_device", 0)))
        return out

    def Kdiag(self, X):
        ret = np.empty(X.shape[0])  # stationary.py:195-198
        ret[:] = float(self.variance)
        return ret

    def copy(self):
        extra = dict(Gower=self.Gower, space=self.space) if self._takes_gower else {}
        return self.__class__(self.input_dim, float(self.variance), self.lengthscale.values.copy(), self.ARD, name=self.name,
                              **extra)


_SCRATCH = {}
_SCRATCH_KEEP_N = 4096        # scratch contexts that served more rows than this are closed right after the call (128 MB at 4096)


def _scratch_handle(device=0):
    h = _SCRATCH.get(device)
    if h is None or h.h is None:
        h = _SCRATCH[device] = _lib.Handle(device)
    return h


def release_scratch(device=None):
    """Close the scratch context(s) ``kern.K`` evaluates on (all devices, or one)."""
    for d in ([device] if device is not None else list(_SCRATCH)):
        h = _SCRATCH.pop(d, None)
        if h is not None:
            h.close()


def gower_config(space, input_dim):
    """(is_discrete[D], range[D]) from a design space, as the fork's Stationary.K reads it
    (stationary.py:117-119: space.get_continuous_dims / get_discrete_dims / lengthscales)."""
    cont = list(space.get_continuous_dims())
    disc = list(space.get_discrete_dims())
    ranges = list(space.lengthscales())
    is_disc = np.zeros(input_dim, dtype=np.int32)
    rng = np.ones(input_dim)
    for idx, d in enumerate(cont):
        rng[d] = ranges[idx]
    for d in disc:
        is_disc[d] = 1
    if sorted(cont + disc) != list(range(input_dim)):
        raise ValueError("the Gower kernel needs every input dimension to be continuous or discrete in `space`")
    return is_disc, rng


class RBF(Stationary):
    """GPy.kern.RBF -- k(r) = variance * exp(-r^2 / 2)  (rbf.py:50-51)."""
    _kernel_id = _lib.GP_KERNEL_RBF

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="rbf",
                 Gower=False, space=None):
        super(RBF, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, Gower, space)


class Matern52(Stationary):
    """GPy.kern.Matern52 -- k(r) = variance (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)  (stationary.py:575-576)."""
    _kernel_id = _lib.GP_KERNEL_MATERN52

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="Mat52",
                 Gower=False, space=None):
        super(Matern52, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, Gower, space)


class ExpQuad(RBF):
    """GPy.kern.ExpQuad -- the RBF covariance under its other name (the same device kernel)."""
    _takes_gower = False

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="ExpQuad"):
        super(ExpQuad, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name)


class Matern32(Stationary):
    """GPy.kern.Matern32 -- k(r) = variance (1 + sqrt3 r) exp(-sqrt3 r)  (stationary.py:478-479)."""
    _kernel_id = _lib.GP_KERNEL_MATERN32
    _takes_gower = False

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="Mat32"):
        super(Matern32, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name)


class Exponential(Stationary):
    """GPy.kern.Exponential -- k(r) = variance exp(-r)  (stationary.py:388-389).  dK_dr / r is singular at r = 0; the device
    follows the reference's _inv_dist (stationary.py:251-258): a coincident pair adds 0 to every gradient."""
    _kernel_id = _lib.GP_KERNEL_EXPONENTIAL
    _takes_gower = False

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="Exponential"):
        super(Exponential, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name)


class OU(Exponential):
    """GPy.kern.OU -- the Ornstein-Uhlenbeck covariance, k(r) = variance exp(-r)  (stationary.py:427-444): Exponential's twin."""

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="OU"):
        super(OU, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name)
