"""NumPy restatements for the output-warped GP (GPy cannot be imported here: paramz is absent).

* the tanh warp f(y) = d y + sum_i a_i tanh(b_i (y + c_i)), f', the parameter partials and ``update_grads``
  (GPy/GPy/util/warping_functions.py:93-169), in any NumPy float type;
* ``f_inv_damped``: the reference's inverse as written at warping_functions.py:34-57 -- 250 Newton sweeps damped by 0.1 over the
  whole array from y = 1, stopped when the summed update falls below 1e-10;
* ``f_inv_exact``: the root by bisection in ``np.longdouble`` (f is strictly increasing);
* ``moments``: the Gauss-Hermite mean and variance of warped_gp.py:62-87 for either inverse;
* ``WarpedOracle``: the model composed from ``oracle.cpu_ref`` -- the oracle's GP on f(Y) plus the log-Jacobian
  (warped_gp.py:38-57), its natural gradients, and predictions in the space of the observations (warped_gp.py:89-132).

The parameter sets A, B, C and S (steep) are the ones the tests run on.
"""
import numpy as np

from oracle import cpu_ref as O

# (psi rows (a_i, b_i, c_i), d)
PARAMS = {
    "A": (np.ones((3, 3)), 1.0),
    "B": (np.array([[0.7, 1.9, -0.4], [1.6, 0.5, 1.2], [0.3, 4.0, 0.1]]), 0.6),
    "C": (np.array([[1.2, 0.8, 0.3], [0.4, 2.5, -1.0]]), 1.5),
    "S": (np.array([[2.5, 6.0, 0.0]]), 0.05),
}
LD = np.longdouble


def f(y, psi, d, dtype=np.float64):
    y = np.asarray(y, dtype=dtype)
    z = dtype(d) * y
    for a, b, c in np.asarray(psi, dtype=dtype):
        z = z + a * np.tanh(b * (y + c))
    return z


def fgrad_y(y, psi, d, dtype=np.float64):
    y = np.asarray(y, dtype=dtype)
    g = dtype(d) + np.zeros_like(y)
    for a, b, c in np.asarray(psi, dtype=dtype):
        g = g + a * b * (1 - np.tanh(b * (y + c)) ** 2)
    return g


def partials(y, psi, d):
    """(df/dpsi, df'/dpsi), each [len(y), n_terms, 4]: columns a, b, c, and d in row 0 (warping_functions.py:130-157)."""
    y = np.asarray(y, dtype=float).reshape(-1)
    df = np.zeros((y.size, len(psi), 4))
    dfp = np.zeros((y.size, len(psi), 4))
    for i, (a, b, c) in enumerate(psi):
        s = b * (y + c)
        r = np.tanh(s)
        q = 1.0 / np.cosh(s) ** 2
        df[:, i, 0], df[:, i, 1], df[:, i, 2] = r, a * (y + c) * q, a * b * q
        dfp[:, i, 0], dfp[:, i, 1], dfp[:, i, 2] = b * q, a * (q - 2.0 * s * r * q), -2.0 * a * b ** 2 * r * q
    df[:, 0, 3], dfp[:, 0, 3] = y, 1.0
    return df, dfp


def update_grads(Y, Kiy, psi, d):
    """(dpsi [n_terms, 3], dd) of warping_functions.py:159-169."""
    Y, Kiy = np.asarray(Y, dtype=float).reshape(-1), np.asarray(Kiy, dtype=float).reshape(-1)
    df, dfp = partials(Y, psi, d)
    g = -(Kiy[:, None, None] * df).sum(0) + (dfp / fgrad_y(Y, psi, d)[:, None, None]).sum(0)
    return g[:, :3], float(g[0, 3])


def f_inv_damped(z, psi, d, max_iterations=250, rate=0.1):
    """warping_functions.py:34-57, with its whole-array stopping rule."""
    z = np.array(z, dtype=float)
    y = np.ones_like(z)
    it, update = 0, np.inf
    while np.abs(update).sum() > 1e-10 and it < max_iterations:
        update = (f(y, psi, d) - z) / fgrad_y(y, psi, d)
        y -= rate * update
        it += 1
    return y


def f_inv_exact(z, psi, d):
    """The root of f(y) = z in long double, by bisection on [(z - sum a) / d - 1, (z + sum a) / d + 1]."""
    z = np.asarray(z, dtype=LD)
    sa = LD(np.sum(np.asarray(psi)[:, 0]))
    lo, hi = (z - sa) / LD(d) - 1, (z + sa) / LD(d) + 1
    for _ in range(160):
        mid = (lo + hi) / 2
        up = f(mid, psi, d, LD) > z
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    return (lo + hi) / 2


def inverse_bound(z, y, psi, d):
    """8 * 2^-52 (|z| + sum a + d |y|): the residual allowed to an inverse, in long double."""
    return 8 * LD(2.0) ** -52 * (np.abs(np.asarray(z, LD)) + LD(np.sum(np.asarray(psi)[:, 0])) + LD(d) * np.abs(np.asarray(y, LD)))


def nodes(mean, std, deg=20):
    """The arguments z[deg, M] of the inverse (warped_gp.py:62-65) and the weights."""
    t, w = np.polynomial.hermite.hermgauss(deg)
    mean, std = np.asarray(mean, dtype=float).reshape(1, -1), np.asarray(std, dtype=float).reshape(1, -1)
    return t[:, None] * std * np.sqrt(2) + mean, w


def moments(mean, std, psi, d, inverse, deg=20):
    """(warped mean [M], warped variance [M]) of warped_gp.py:67-87; ``inverse(z, psi, d)`` -> y, evaluated in its type."""
    z, w = nodes(mean, std, deg)
    y = inverse(z, psi, d)
    w = np.asarray(w, dtype=y.dtype)[:, None]
    wmean = (w * y).sum(0) / np.sqrt(y.dtype.type(np.pi))
    return wmean, (w * y ** 2).sum(0) / np.sqrt(y.dtype.type(np.pi)) - wmean ** 2


class WarpedOracle(object):
    """``WarpedGP`` composed from the oracle: OracleGP on f(normalised Y), LML + log-Jacobian, natural gradients, predictions."""

    def __init__(self, X, Y, kernel, noise_var, psi, d, normalizer=False):
        self.psi, self.d = np.asarray(psi, dtype=float), float(d)
        self.normalizer = None
        Yn = np.asarray(Y, dtype=float)
        if normalizer:
            self.normalizer = O.Standardize()
            self.normalizer.scale_by(Yn)
            Yn = self.normalizer.normalize(Yn)
        self.Y_untransformed = Yn
        self.gp = O.OracleGP(X, f(Yn, self.psi, self.d), kernel, noise_var)

    def log_jacobian(self):
        return float(np.log(fgrad_y(self.Y_untransformed, self.psi, self.d)).sum())

    def log_likelihood(self):
        return self.gp.log_likelihood() + self.log_jacobian()

    def gradients(self):
        """Natural gradients in the model's order: variance, lengthscale, noise, a, b, c, d."""
        dv, dl, dn = self.gp.gradients()
        dpsi, dd = update_grads(self.Y_untransformed, self.gp.posterior["alpha"], self.psi, self.d)
        return np.r_[dv, np.ravel(dl), dn, dpsi[:, 0], dpsi[:, 1], dpsi[:, 2], dd]

    def latent(self, Xs):
        """(mean, std) of the latent posterior with noise, the normaliser's affine map applied (warped_gp.py:101-105)."""
        m, v = self.gp.predict(Xs)
        if self.normalizer is not None:
            m, v = self.normalizer.inverse_mean(m), self.normalizer.inverse_variance(v)
        return m, np.sqrt(v)

    def predict(self, Xs, median=False, deg=20, inverse=f_inv_exact):
        m, s = self.latent(Xs)
        wmean, wvar = moments(m, s, self.psi, self.d, inverse, deg)
        if median:
            wmean = inverse(m.reshape(-1), self.psi, self.d)
        return np.asarray(wmean, dtype=float)[:, None], np.asarray(wvar, dtype=float)[:, None]

    def predict_quantiles(self, Xs, quantiles=(2.5, 97.5)):
        qs = self.gp.predict_quantiles(Xs, quantiles)
        if self.normalizer is not None:
            qs = [self.normalizer.inverse_mean(q) for q in qs]
        return [np.asarray(f_inv_exact(q, self.psi, self.d), dtype=float) for q in qs]
