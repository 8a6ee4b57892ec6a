"""Shared by tests/test_gpu_warped_batch.py and tests/test_warped_batch_host.py: problems, members and references of the two
batched entries of the warped models, ``gp_fit_grad_x_batch`` and ``gp_fit_grad_warp_batch``.

* ``data``: inputs in [0, 1]^D and P target columns, seeded.  Rows 0 and 1 (where there are two) lie within 1e-6 of the upper
  corner: a Kumaraswamy warp with a = b = 3 maps both to exactly (1, ..., 1) -- (1 - u^3)^3 <= 2.7e-17 is below half an ulp of
  1 -- so the member that carries that warp has a coincident pair, which must add exactly 0 to dL/dX (``_inv_dist``).
* ``kumar_members``: member r's inputs, the Kumaraswamy CDF of the base X with exponents spread over 0.3 .. 3 per member and
  dimension; the LAST member (of two or more) is the collapsing one.
* ``tanh_members``: per-member tanh warps (psi [R, T, 3], d [R]) with a in 0.2 .. 2, b in 0.3 .. 3, c in -1 .. 1, d in 0.3 .. 1.5.
* ``kernel_members``: variance, lengthscale(s) and noise spread over decades (the spread of tests/test_gpu_fit_grad_batch.py,
  the noise kept at 1e-4 and above: the collapsing member has a duplicated row).
* ``OracleHandle``: what the two models ask of ``_lib.Handle``, answered by ``oracle.cpu_ref`` (no device), and
  ``BatchOverSingles``: the same with the two batch methods, each a loop over the single-member methods.
* the comparison rules of the GPU tests (``same_bits``, ``close``, ``err``).
"""
import numpy as np

from oracle import cpu_ref as O

import _kernel_families as KF
import _warped_ref as WR

FAMILIES = ["rbf", "Mat52", "Mat32", "Exponential"]     # in the order of the GP_KERNEL_* codes 0 .. 3


def data(N, D, P, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    if N >= 2:
        X[0] = 1.0 - 1e-6 * rng.uniform(0.1, 0.4, D)
        X[1] = 1.0 - 1e-6 * rng.uniform(0.5, 0.9, D)
    Y = np.stack([np.sin(2 * np.pi * (p + 1) * X).sum(1) / np.sqrt(D) + 0.1 * rng.standard_normal(N) for p in range(P)], 1)
    return X, Y


def kumar(X, a, b):
    """1 - (1 - x^a)^b per column (x in [0, 1]): KumarWarping.f with bounds 0 and 1."""
    return 1.0 - np.power(1.0 - np.power(X, a[None, :]), b[None, :])


def kumar_members(X, R, seed):
    """Xw [R, N, D]; with R >= 2 and N >= 2 the last member maps rows 0 and 1 onto the same point."""
    rng = np.random.default_rng(seed)
    D = X.shape[1]
    Xw = np.empty((R,) + X.shape)
    for r in range(R):
        a, b = rng.uniform(0.3, 3.0, D), rng.uniform(0.3, 3.0, D)
        if r == R - 1 and R >= 2:
            a[:], b[:] = 3.0, 3.0
        Xw[r] = kumar(X, a, b)
    if R >= 2 and X.shape[0] >= 2:
        assert np.array_equal(Xw[R - 1][0], Xw[R - 1][1]) and not np.array_equal(X[0], X[1])
    return Xw


def tanh_members(R, T, seed):
    rng = np.random.default_rng(seed)
    psi = np.stack([rng.uniform(0.2, 2.0, (R, T)), rng.uniform(0.3, 3.0, (R, T)), rng.uniform(-1.0, 1.0, (R, T))], axis=2)
    return np.ascontiguousarray(psi), rng.uniform(0.3, 1.5, R)


def kernel_members(R, D, ard, seed):
    rng = np.random.default_rng(seed)
    nls = D if ard else 1
    var = 10.0 ** rng.uniform(-1.5, 1.5, R)
    ls = np.sqrt(D) * 10.0 ** rng.uniform(-1.2, 0.3, (R, nls))
    noise = 10.0 ** rng.uniform(-4.0, -1.0, R)
    return var, ls, noise


# ---- comparison rules ----------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=float), np.ascontiguousarray(b, dtype=float)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def close(head_a, head_b, grad_a, grad_b, rtol=1e-12):
    """``_close`` of tests/test_gpu_fit_grad_batch.py: the head (lml, log det, jitter, ...) within rtol relative, the gradient
    entries within rtol of the member's largest one."""
    head_a, head_b = np.asarray(head_a, dtype=float), np.asarray(head_b, dtype=float)
    grad_a, grad_b = np.asarray(grad_a, dtype=float), np.asarray(grad_b, dtype=float)
    head = np.all(np.abs(head_a - head_b) <= rtol * np.abs(head_b))
    return bool(head and np.max(np.abs(grad_a - grad_b)) <= rtol * np.max(np.abs(grad_b)))


def err(what, got, ref, tol, scale=None):
    """Largest error relative to the largest reference entry, printed before it is asserted."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), what
    s = float(np.max(np.abs(ref))) if scale is None else float(scale)
    e = float(np.max(np.abs(got - ref))) / max(s, 1e-300)
    print("%-52s err %.3e  tol %.1e" % (what, e, tol))
    assert e <= tol, (what, e, tol)


# ---- oracle references -----------------------------------------------------------------------------------------------------------
def oracle_x(fam, ard, X, Y, variance, ls, noise):
    """(lml, (dvariance, dlengthscale, dnoise), dL_dX) of one member from the direct-distance oracle (tests/test_gpu_lml_grad_x.py)."""
    kern = KF.make(fam, X.shape[1], variance, np.asarray(ls, dtype=float), ard, direct=True)
    p = O.exact_gaussian_inference(kern, X, Y, noise)
    dv, dl = kern.update_gradients_full(p["dL_dK"], X)
    return p["lml"], (dv, dl, p["dL_dthetaL"]), np.asarray(kern.gradients_X(p["dL_dK"], X), dtype=float)


def oracle_warp(fam, ard, X, Yraw, variance, ls, noise, psi, d):
    """The composed oracle of tests/test_gpu_warped_gp.py for one member: (LML + log-Jacobian, natural gradients in the order
    variance, lengthscale, noise, a, b, c, d)."""
    kern = KF.make(fam, X.shape[1], variance, np.asarray(ls, dtype=float), ard, direct=True)
    ora = WR.WarpedOracle(X, Yraw, kern, noise, psi, d)
    return ora.log_likelihood(), ora.gradients()


# ---- a handle without a device -----------------------------------------------------------------------------------------------
class OracleHandle(object):
    """What ``InputWarpedGP`` and ``WarpedGP`` ask of ``_lib.Handle`` during a hyper-parameter search, answered by the oracle."""

    def __init__(self, device=0):
        self.calls = {"fit": 0, "fit_grad_x": 0, "fit_grad_warp": 0, "fit_grad_x_batch": 0, "fit_grad_warp_batch": 0}
        self.batch_sizes = []
        self.warp = None
        self.fail_when = None        # callable(variance, lengthscale, noise) -> True: the member is not positive definite

    def close(self):
        pass

    def set_data(self, X, Y):
        self.X, self.Yraw = np.array(X, dtype=float), np.array(Y, dtype=float)
        self.N, self.D, self.P = self.X.shape[0], self.X.shape[1], self.Yraw.shape[1]

    def set_params(self, kernel, ard, variance, lengthscale, noise):
        self.params = (int(kernel), bool(ard), float(variance), np.array(np.atleast_1d(lengthscale), dtype=float), float(noise))
        self.n_ls = self.params[3].size

    def set_gower(self, *a):
        pass

    def set_output_warp(self, psi=None, d=1.0):
        if psi is None or np.size(psi) == 0:
            self.warp = None
            return 0.0
        self.warp = (np.array(psi, dtype=float), float(d))
        return float(np.log(WR.fgrad_y(self.Yraw, *self.warp)).sum())

    def _targets(self):
        return self.Yraw if self.warp is None else WR.f(self.Yraw, *self.warp)

    def _infer(self, maxtries):
        k, ard, v, ls, n = self.params
        if self.fail_when is not None and self.fail_when(v, ls, n):
            raise np.linalg.LinAlgError("not positive definite, even with jitter.")
        kern = KF.make(FAMILIES[k], self.D, v, ls, ard)
        p = O.exact_gaussian_inference(kern, self.X, self._targets(), n, maxtries=maxtries)
        dv, dl = kern.update_gradients_full(p["dL_dK"], self.X)
        return kern, p, (p["lml"], p["logdet"], p["jitter"]), (dv, dl, p["dL_dthetaL"])

    def fit(self, maxtries=5):
        self.calls["fit"] += 1
        return self._infer(maxtries)[2]

    def lml_grad(self, nls):
        return self._infer(5)[3]

    def lml_grad_x(self):
        kern, p, _, _ = self._infer(5)
        return np.asarray(kern.gradients_X(p["dL_dK"], self.X), dtype=float)

    def fit_grad_x(self, nls, maxtries=5):
        self.calls["fit_grad_x"] += 1
        kern, p, fit, grads = self._infer(maxtries)
        return fit, grads, np.asarray(kern.gradients_X(p["dL_dK"], self.X), dtype=float)

    def warp_grad(self, n_terms):
        _, p, _, _ = self._infer(5)
        return WR.update_grads(self.Yraw, p["alpha"], *self.warp)

    def fit_grad_warp(self, psi, d, nls, maxtries=5):
        self.calls["fit_grad_warp"] += 1
        lj = self.set_output_warp(psi, d)
        _, p, fit, grads = self._infer(maxtries)
        return fit, grads, lj, WR.update_grads(self.Yraw, p["alpha"], *self.warp)


class BatchOverSingles(OracleHandle):
    """``OracleHandle`` with the two batch methods of ``_lib.Handle``, each a loop over the single-member methods on a scratch
    handle: the resident data, parameters and warp of this one are left alone, as the device entries leave them."""

    def _scratch(self):
        s = OracleHandle()
        s.fail_when = self.fail_when
        return s

    def _loop(self, R, nls, one, extras):
        lml, logdet, jit = np.full(R, np.nan), np.full(R, np.nan), np.full(R, np.nan)
        dv, dl, dn = np.full(R, np.nan), np.full((R, nls), np.nan), np.full(R, np.nan)
        status = np.zeros(R, dtype=np.int32)
        for r in range(R):
            try:
                res = one(r)
            except np.linalg.LinAlgError:
                status[r] = 1
                continue
            (lml[r], logdet[r], jit[r]), (dv[r], dl[r], dn[r]) = res[0], res[1]
            extras(r, res[2:])
        return (lml, logdet, jit), (dv, dl, dn), status

    def fit_grad_x_batch(self, Xw, variances, lengthscales, noises, maxtries=5):
        self.calls["fit_grad_x_batch"] += 1
        R = len(variances)
        self.batch_sizes.append(R)
        k, ard = self.params[:2]
        dX = np.full((R, self.N, self.D), np.nan)
        s = self._scratch()

        def one(r):
            s.set_data(Xw[r], self._targets())
            s.set_params(k, ard, variances[r], lengthscales[r], noises[r])
            return s.fit_grad_x(self.n_ls, maxtries)

        def extras(r, rest):
            dX[r] = rest[0]

        fit, grads, status = self._loop(R, self.n_ls, one, extras)
        return fit, grads, dX, status

    def fit_grad_warp_batch(self, psis, ds, variances, lengthscales, noises, maxtries=5):
        self.calls["fit_grad_warp_batch"] += 1
        R = len(variances)
        self.batch_sizes.append(R)
        k, ard = self.params[:2]
        psis = np.asarray(psis, dtype=float)
        lj, dpsi, dd = np.full(R, np.nan), np.full(psis.shape, np.nan), np.full(R, np.nan)
        s = self._scratch()
        s.set_data(self.X, self.Yraw)

        def one(r):
            s.set_params(k, ard, variances[r], lengthscales[r], noises[r])
            return s.fit_grad_warp(psis[r], ds[r], self.n_ls, maxtries)

        def extras(r, rest):
            lj[r], (dpsi[r], dd[r]) = rest[0], rest[1]

        fit, grads, status = self._loop(R, self.n_ls, one, extras)
        return fit, grads, lj, (dpsi, dd), status
