"""Oracle kernels for the Matern-3/2 and Exponential families, as subclasses of the oracle's ``Stationary`` (oracle/cpu_ref.py),
and direct-distance variants of all four families (``make(name, ...)`` takes "rbf" and "Mat52" as well: the oracle's own classes).

Each family states only ``K_of_r`` and ``dK_dr`` (GPy/GPy/kern/src/stationary.py:478-482 for Matern32, :388-392 for
Exponential); distances, ``K``, ``_inv_dist``, ``update_gradients_full`` and ``gradients_X`` are the oracle's, so ``OracleGP``,
``OracleGPModel``, the acquisition functions and ``OracleLP`` work on them unchanged.

The ``*Direct`` variants replace the Gram trick of ``_unscaled_dist`` (stationary.py:155-173) by direct differences summed in
``np.longdouble``.  The Gram trick carries ~1e-8 of absolute noise in r next to a coincident pair, and the Exponential
covariance is not differentiable at r = 0: that noise is the oracle's error, not the device's.  They serve the K comparison at
1e-13 (with ``extended=True`` the distance stays in long double, so K_of_r is evaluated there too), the duplicated-rows case, and
inputs far from the origin, where the Gram trick cancels |x / l|^2 ~ 1e6 against r^2 ~ 1 (tests/test_family_shapes_host.py).
"""
import numpy as np

from oracle import cpu_ref as O

SQRT3 = np.sqrt(3.0)


class Matern32(O.Stationary):
    """k(r) = variance (1 + sqrt3 r) exp(-sqrt3 r); dk/dr = -3 variance r exp(-sqrt3 r)  (stationary.py:478-482)."""
    name = "Mat32"

    def K_of_r(self, r):
        s3 = np.sqrt(r.dtype.type(3.0)) if hasattr(r, "dtype") else SQRT3
        return self.variance * (1.0 + s3 * r) * np.exp(-s3 * r)

    def dK_dr(self, r):
        s3 = np.sqrt(r.dtype.type(3.0)) if hasattr(r, "dtype") else SQRT3
        return -3.0 * self.variance * r * np.exp(-s3 * r)


class Exponential(O.Stationary):
    """k(r) = variance exp(-r); dk/dr = -k(r)  (stationary.py:388-392)."""
    name = "Exponential"

    def K_of_r(self, r):
        return self.variance * np.exp(-r)

    def dK_dr(self, r):
        return -self.K_of_r(r)


class _DirectDistance(object):
    """Mixin: r from direct differences in long double (no Gram-trick cancellation); rounded to float64 unless ``extended``."""
    extended = False

    def _unscaled_dist(self, X, X2=None):
        A = np.asarray(X, dtype=np.longdouble)
        B = A if X2 is None else np.asarray(X2, dtype=np.longdouble)
        r2 = np.zeros((A.shape[0], B.shape[0]), dtype=np.longdouble)
        for q in range(A.shape[1]):
            d = A[:, q][:, None] - B[:, q][None, :]
            r2 += d * d
        r = np.sqrt(r2)
        return r if self.extended else r.astype(np.float64)

    def _scaled_dist(self, X, X2=None):
        ls = np.asarray(self.lengthscale, dtype=np.longdouble)
        X = np.asarray(X, dtype=np.longdouble)
        X2 = None if X2 is None else np.asarray(X2, dtype=np.longdouble)
        if self.ARD:
            return self._unscaled_dist(X / ls, None if X2 is None else X2 / ls)
        # (the device divides every coordinate by the lengthscale as well; in long double the two orders agree to 1e-19)
        return self._unscaled_dist(X / ls[0], None if X2 is None else X2 / ls[0])


class Matern32Direct(_DirectDistance, Matern32):
    pass


class ExponentialDirect(_DirectDistance, Exponential):
    pass


class RBFDirect(_DirectDistance, O.RBF):
    pass


class Matern52Direct(_DirectDistance, O.Matern52):
    pass


FAMILIES = {"Mat32": (Matern32, Matern32Direct), "Exponential": (Exponential, ExponentialDirect),
            "rbf": (O.RBF, RBFDirect), "Mat52": (O.Matern52, Matern52Direct)}


def make(name, input_dim, variance, lengthscale, ARD, direct=False, extended=False):
    """The oracle kernel of a family; ``direct`` takes direct-difference distances, ``extended`` keeps them in long double."""
    k = FAMILIES[name][1 if direct else 0](input_dim, variance=variance, lengthscale=lengthscale, ARD=ARD)
    if extended:
        assert direct
        k.extended = True
    return k
