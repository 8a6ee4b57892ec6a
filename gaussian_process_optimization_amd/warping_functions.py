"""Output warping functions of the warped GP -- host mirror of ``GPy.util.warping_functions``.

Reference: GPy/GPy/util/warping_functions.py:10-169 (``WarpingFunction``, ``TanhFunction``), :172-231 (``LogFunction``,
``IdentityFunction``).

The model evaluates the warp on the device (include/gphip.h, "output-warped GP"); the NumPy methods here exist for API parity
and for checking: ``f``, ``fgrad_y``, ``fgrad_y_psi``, ``update_grads`` follow the reference's formulas, ``f_inv`` does NOT
follow its 250 damped Newton sweeps (warping_functions.py:34-57, still far from the root for steep warps) but solves each
element inside the bracket the device uses.

Parameters: ``a``, ``b`` (positive, Logexp), ``c`` (free) of ``n_terms`` entries each and ``d`` (positive, Logexp), all starting
at one; ``psi`` is the [n_terms, 3] view (a, b, c) of the first three.  (The reference holds one ``psi`` matrix with a sliced
positivity constraint on its first two columns; the separate parameters say the same.)
"""
import numpy as np

from .parameterization import Logexp, Param, Parameterized

MAX_TERMS = 8      # GP_WARP_MAX_TERMS of the device


class _Free(object):
    """No constraint: the optimiser sees the value itself."""

    def f(self, x):
        return np.asarray(x, dtype=float)

    def finv(self, f):
        return np.asarray(f, dtype=float)

    def gradfactor(self, f, df):
        return df


class WarpingFunction(Parameterized):
    """z = f(y) (warping_functions.py:10-68)."""

    def __init__(self, name):
        super(WarpingFunction, self).__init__(name=name)
        self.rate = 0.1      # the reference's damping, kept as an attribute; ``f_inv`` here does not use it

    def f(self, y):
        raise NotImplementedError

    def fgrad_y(self, y):
        raise NotImplementedError

    def fgrad_y_psi(self, y):
        raise NotImplementedError

    def update_grads(self, Y_untransformed, Kiy):
        pass

    def f_inv(self, z, max_iterations=250, y=None):
        raise NotImplementedError


class TanhFunction(WarpingFunction):
    """f(y) = d y + sum_i a_i tanh(b_i (y + c_i)) (Snelson et al.; warping_functions.py:71-169)."""

    def __init__(self, n_terms=3, initial_y=None):
        n_terms = int(n_terms)
        if not 1 <= n_terms <= MAX_TERMS:
            raise ValueError("n_terms must lie in 1..%d, got %d" % (MAX_TERMS, n_terms))
        super(TanhFunction, self).__init__(name='warp_tanh')
        self.n_terms = n_terms
        self.num_parameters = 3 * n_terms + 1
        self.a = Param('a', np.ones(n_terms), Logexp())
        self.b = Param('b', np.ones(n_terms), Logexp())
        self.c = Param('c', np.ones(n_terms), _Free())
        self.d = Param('d', 1.0, Logexp())
        self.link_parameters(self.a, self.b, self.c, self.d)
        self.initial_y = initial_y

    @property
    def psi(self):
        """[n_terms, 3]: the rows (a_i, b_i, c_i)."""
        return np.c_[self.a.values, self.b.values, self.c.values]

    def set_psi(self, psi, d=None):
        psi = np.asarray(psi, dtype=float).reshape(self.n_terms, 3)
        self.a.set(psi[:, 0])
        self.b.set(psi[:, 1])
        self.c.set(psi[:, 2])
        if d is not None:
            self.d.set(d)

    def f(self, y):
        """warping_functions.py:93-106."""
        y = np.asarray(y, dtype=float)
        z = float(self.d) * y.copy()
        for a, b, c in self.psi:
            z += a * np.tanh(b * (y + c))
        return z

    def fgrad_y(self, y, return_precalc=False):
        """df/dy in the shape of ``y``; with ``return_precalc`` also S, R, D [n_terms, ...] (warping_functions.py:108-128)."""
        y = np.asarray(y, dtype=float)
        psi = self.psi
        shape = (-1,) + (1,) * y.ndim
        S = psi[:, 1].reshape(shape) * (y[None] + psi[:, 2].reshape(shape))
        R = np.tanh(S)
        D = 1 - R ** 2
        grad = float(self.d) + (psi[:, 0].reshape(shape) * psi[:, 1].reshape(shape) * D).sum(axis=0)
        if return_precalc:
            return grad, S, R, D
        return grad

    def fgrad_y_psi(self, y, return_covar_chain=False):
        """d(df/dy)/dpsi, [N, P, n_terms, 4] (columns a, b, c, and d in row 0); with ``return_covar_chain`` also df/dpsi in the
        same layout (warping_functions.py:130-157)."""
        y = np.asarray(y, dtype=float)
        if y.ndim == 1:
            y = y[:, None]
        psi = self.psi
        _, s, r, d = self.fgrad_y(y, return_precalc=True)
        gradients = np.zeros(y.shape + (len(psi), 4))
        for i, (a, b, c) in enumerate(psi):
            gradients[:, :, i, 0] = b * d[i]
            gradients[:, :, i, 1] = a * (d[i] - 2.0 * s[i] * r[i] * d[i])
            gradients[:, :, i, 2] = -2.0 * a * b ** 2 * r[i] * d[i]
        gradients[:, :, 0, 3] = 1.0
        if not return_covar_chain:
            return gradients
        chain = np.zeros(y.shape + (len(psi), 4))
        for i, (a, b, c) in enumerate(psi):
            chain[:, :, i, 0] = r[i]
            chain[:, :, i, 1] = a * (y + c) * d[i]
            chain[:, :, i, 2] = a * b * d[i]
        chain[:, :, 0, 3] = y
        return gradients, chain

    def update_grads(self, Y_untransformed, Kiy):
        """Gradients of LML + log-Jacobian into ``a``, ``b``, ``c``, ``d`` (warping_functions.py:159-169)."""
        Y = np.asarray(Y_untransformed, dtype=float)
        if Y.ndim == 1:
            Y = Y[:, None]
        Kiy = np.asarray(Kiy, dtype=float).reshape(-1)
        grad_y = self.fgrad_y(Y)
        grad_y_psi, grad_psi = self.fgrad_y_psi(Y, return_covar_chain=True)
        djac_dpsi = ((1.0 / grad_y[:, :, None, None]) * grad_y_psi).sum(axis=0).sum(axis=0)
        dquad_dpsi = (Kiy[:, None, None, None] * grad_psi).sum(axis=0).sum(axis=0)
        g = -dquad_dpsi + djac_dpsi
        self.a.gradient[:] = g[:, 0]
        self.b.gradient[:] = g[:, 1]
        self.c.gradient[:] = g[:, 2]
        self.d.gradient[:] = g[0, 3]

    def f_inv(self, z, max_iterations=250, y=None):
        """f^-1 elementwise: Newton's iteration kept inside [(z - sum a) / d, (z + sum a) / d], a step that leaves the bracket
        or fails to halve the previous one replaced by the midpoint, to a step below 2^-52 max(1, |y|) -- the device's
        algorithm (csrc/warp_math.h), not the reference's damped sweeps; ``y`` (a starting point) is accepted and ignored."""
        z = np.asarray(z, dtype=float)
        zf = z.reshape(-1)
        d, sa = float(self.d), float(np.sum(self.a.values))
        lo, hi = (zf - sa) / d, (zf + sa) / d
        out = zf / d
        dxold = hi - lo
        active = np.isfinite(zf)
        for _ in range(128):
            if not active.any():
                break
            f = self.f(out) - zf
            df = self.fgrad_y(out)
            active &= f != 0.0
            pos = f > 0
            hi = np.where(active & pos, out, hi)
            lo = np.where(active & ~pos, out, lo)
            with np.errstate(invalid="ignore", over="ignore"):
                dx = f / df
                yn = out - dx
                bis = ~((yn > lo) & (yn < hi)) | (np.abs(2.0 * f) > np.abs(dxold * df))
            mid = 0.5 * (lo + hi)
            yn = np.where(bis, mid, yn)
            dx = np.where(bis, out - mid, dx)
            dxold = np.where(active, dx, dxold)
            out = np.where(active, yn, out)
            active &= np.abs(dx) > 2.0 ** -52 * np.maximum(1.0, np.abs(out))
        out = np.where(np.isfinite(zf), out, zf)
        return out.reshape(z.shape)


class IdentityFunction(WarpingFunction):
    """f(y) = y, no parameters (warping_functions.py:203-231): the warped model is then the plain GP."""

    def __init__(self, closed_inverse=True):
        super(IdentityFunction, self).__init__(name='identity')
        self.num_parameters = 0

    def f(self, y):
        return np.asarray(y, dtype=float)

    def fgrad_y(self, y):
        return np.ones(np.shape(y))

    def fgrad_y_psi(self, y, return_covar_chain=False):
        return (0, 0) if return_covar_chain else 0

    def f_inv(self, z, max_iterations=250, y=None):
        return np.asarray(z, dtype=float)


class LogFunction(WarpingFunction):
    """The fixed log warp (warping_functions.py:172-200) is not part of the accelerated path."""

    def __init__(self, closed_inverse=True):
        raise NotImplementedError("LogFunction is outside the accelerated path: take the logarithm of Y and fit a GPRegression")
