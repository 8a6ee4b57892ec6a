"""Entropy search on the host: what stays in NumPy / LAPACK around the device kernels of csrc/es.hip.

Reference: GPyOpt/GPyOpt/util/epmgp.py (``joint_min``, ``min_faktor``), GPyOpt/GPyOpt/acquisitions/ES.py:124-207,
GPyOpt/GPyOpt/util/mcmc_sampler.py.  The device runs the EP sweeps (``gp_es_pmin``) and scores candidate tables
(``gp_es_acq``); this module holds

* ``ep_sweeps``   -- the same sweeps in NumPy, for the host route (sparse models, cost models, ``device=False``),
* ``ep_closing``  -- the closing algebra of one chain: log Z and its derivatives from the site parameters (R solves of order
                     R - 1 for a belief: milliseconds),
* ``renormalise`` -- ``joint_min``'s normalisation of the R chains into one belief,
* ``quadratic_forms`` -- Q with ``m^T Q_i m`` = ES.py:148-154's deterministic change for the innovation ``m``,
* ``score``       -- ES.py:156-170 for one innovation,
* ``AffineInvariantEnsembleSampler`` -- the Goodman-Weare stretch move (the reference wraps emcee; the draws here are NOT
                     emcee's: another generator, another order of proposals -- the same stationary law).
"""
import numpy as np
from scipy.special import erfc

_ROOT_2 = np.sqrt(2.0)
_LOG_2PI = np.log(2.0) + np.log(np.pi)
_EPS32 = float(np.finfo(np.float32).eps)
_LOGP_FLOOR = -500.0        # what joint_min gives a chain whose log Z is -inf (epmgp.py:92)


def _npmax(a, b):
    """numpy.max of two scalars: a NaN wins."""
    return a + b if (a != a or b != b) else max(a, b)


def ep_sweeps(mu, cov, max_sweeps=50, tol=1e-3):
    """The EP sweeps of the R chains "representer k is the minimum" (epmgp.py:122-153 with lt_factor :211-272): site
    precisions ``P``, precision-means ``MP`` and log scales ``logS`` [R, R - 1], ``status`` [R] (0 converged, 1 sweep limit,
    -1 a factor ended the chain: log Z = -inf; a NaN in the working covariance raises, as the reference does) and ``sweeps``
    [R], the sweeps begun.  Same thresholds as the reference and as the device kernel."""
    mu, cov = np.asarray(mu, dtype=float), np.asarray(cov, dtype=float)
    R = mu.shape[0]
    P, MP, logS = (np.zeros((R, max(R - 1, 0))) for _ in range(3))
    status, sweeps = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    with np.errstate(all='ignore'):
        for k in range(R):
            M, V = mu.copy(), cov.copy()
            state, count = 1, 0
            while count < max_sweeps and state == 1:
                count += 1
                total, ended = 0.0, False
                for i in range(R - 1):
                    l = i if i < k else i + 1
                    p, mp = P[k, i], MP[k, i]
                    cVc = (V[l, l] - 2.0 * V[k, l] + V[k, k]) / 2.0
                    Vc = (V[:, l] - V[:, k]) / _ROOT_2
                    cM = (M[l] - M[k]) / _ROOT_2
                    cav_v = _npmax(cVc / (1.0 - p * cVc), 0.0)
                    cav_m = cM + cav_v * (p * cM - mp)
                    z = cav_m / np.sqrt(cav_v + 1e-25)
                    if z != z:
                        z = -np.inf
                    if z < -6.0:
                        P[k, i], MP[k, i], logS[k, i] = 0.0, 0.0, -np.inf
                        state, ended = -1, True
                        break
                    if z > 6.0:     # the factor holds almost surely: its message is removed
                        dp, dmp = -p, -mp
                        d = dp if dp > dmp else dmp
                        p_new, mp_new, ls = 0.0, 0.0, 0.0
                    else:
                        log_pdf = -0.5 * (z * z + _LOG_2PI)
                        log_cdf = np.log(0.5 * erfc(-z / _ROOT_2))
                        ratio = np.exp(log_pdf - log_cdf)
                        alpha = ratio / np.sqrt(cav_v)
                        beta = alpha * (alpha * cav_v + cav_m)
                        r = beta / (1.0 - beta)
                        dp = _npmax(-p + _EPS32, r / cav_v - p)
                        dmp = _npmax(-mp + _EPS32, r * (alpha + cav_m / cav_v) + alpha - mp)
                        d = _npmax(dmp, dp)
                        p_new, mp_new = p + dp, mp + dmp
                        ls = log_cdf - 0.5 * (np.log(beta) - np.log(p_new) - np.log(cav_v)) + (alpha * alpha) / (2.0 * beta) * cav_v
                    den = 1.0 + dp * cVc
                    V = V - dp / den * np.outer(Vc, Vc)
                    M = M + (dmp - cM * dp) / den * Vc
                    P[k, i], MP[k, i], logS[k, i] = p_new, mp_new, ls
                    if np.any(np.isnan(V)):
                        raise RuntimeError("expectation propagation in entropy search: the working covariance contains NaN")
                    if d != d:
                        state, ended = -1, True
                        break
                    total += abs(d)
                if not ended and abs(total) < tol:
                    state = 0
            status[k], sweeps[k] = state, count
    return P, MP, logS, status, sweeps


def lower_mask(R):
    """The boolean mask of the lower triangle, diagonal included: ``A[lower_mask(R)]`` packs it in row-major order -- the
    packing of ``dlogPdSigma`` (epmgp.py:207) and of ES.py:148."""
    return np.tril(np.ones((R, R), dtype=bool))


def ep_closing(mu, cov, k, P, MP, logS):
    """log Z of chain ``k`` and its derivatives with respect to ``mu`` [R], ``mu mu`` [R, R] and the packed lower triangle of
    ``cov`` [R (R + 1) / 2], from the chain's site parameters (epmgp.py:166-208)."""
    mu, cov = np.asarray(mu, dtype=float), np.asarray(cov, dtype=float)
    R = mu.shape[0]
    others = [l for l in range(R) if l != k]
    C = np.zeros((R, R - 1))        # column i: the direction (e_l - e_k) / sqrt2 of factor i
    C[others, np.arange(R - 1)] = 1.0 / _ROOT_2
    C[k, :] = -1.0 / _ROOT_2
    Rm = C * np.sqrt(P)[None, :]
    r = C @ MP
    nz = MP != 0
    mpm = float(np.sum(MP[nz] * MP[nz] / P[nz]))
    inner = np.eye(R - 1) + Rm.T @ cov @ Rm
    A = Rm @ np.linalg.solve(inner, Rm.T)
    A = 0.5 * (A.T + A)
    b = mu + cov @ r
    Ab = A @ b
    for bump in (0.0, 1e-10, 1e-6):
        try:
            chol = np.linalg.cholesky(inner + bump * np.eye(R - 1) if bump else inner)
            break
        except np.linalg.LinAlgError:
            if bump == 1e-6:
                raise
    logdet = 2.0 * np.sum(np.log(np.diagonal(chol)))
    logZ = 0.5 * (r @ cov @ r - b @ Ab - logdet) + mu @ r + np.sum(logS) - 0.5 * mpm
    Dm = -A - 2.0 * np.outer(r, Ab) + np.outer(r, r) + np.outer(b @ A, Ab)
    Dm = 0.5 * (Dm + Dm.T - np.diag(np.diagonal(Dm)))
    return logZ, r - Ab, -A, Dm[lower_mask(R)]


def renormalise(logZ, dMu, dSigma, dMuMu):
    """The R chains' log Z and derivatives into one belief (epmgp.py:92-119): (logP [R], dlogPdMu [R, R], dlogPdSigma
    [R, R (R + 1) / 2], dlogPdMudMu [R, R, R]).  -inf entries become -500 first.  The last correction adds the SQUARE of the
    mean shift ``Zm[j]^2`` along the second index where the derivation has the outer product ``Zm Zm^T``: the reference's
    arithmetic (its ``Zm.T * Zm`` on a 1-D array), kept so that the belief is the reference's -- dlogPdMudMu is therefore not
    symmetric, which ``quadratic_forms`` takes care of."""
    logZ = np.array(logZ, dtype=float)
    logZ[np.isinf(logZ)] = _LOGP_FLOOR
    w = np.exp(logZ)
    Z = np.sum(w)
    top = np.max(logZ)
    with np.errstate(divide='ignore'):
        s = top + np.log(np.sum(np.exp(logZ - top)))
    s = top if np.isinf(s) else s
    Zm = (w[:, None] * dMu).sum(0) / Z
    Zs = (w[:, None] * dSigma).sum(0) / Z
    second = dMuMu + dMu[:, :, None] * dMu[:, None, :]
    gg = np.einsum('kij,k->ij', second, w) / Z
    return logZ - s, dMu - Zm, dSigma - Zs, dMuMu + (-gg + Zm * Zm)[None, :, :]


def joint_min(mu, cov, sites=None):
    """``epmgp.joint_min(mu, cov, with_derivatives=True)``; ``sites`` = (P, MP, logS, status, ...) of the EP sweeps when the
    device ran them, else they run here."""
    mu, cov = np.asarray(mu, dtype=float), np.asarray(cov, dtype=float)
    R = mu.shape[0]
    if sites is None:
        sites = ep_sweeps(mu, cov)
    P, MP, logS, status = sites[:4]
    if np.any(np.asarray(status) == -2):
        raise RuntimeError("expectation propagation in entropy search: the working covariance contains NaN")
    logZ, dMu = np.full(R, -np.inf), np.zeros((R, R))
    dSigma, dMuMu = np.zeros((R, R * (R + 1) // 2)), np.zeros((R, R, R))
    for k in range(R):
        if status[k] != -1:
            logZ[k], dMu[k], dMuMu[k], dSigma[k] = ep_closing(mu, cov, k, P[k], MP[k], logS[k])
    return renormalise(logZ, dMu, dSigma, dMuMu)


def quadratic_forms(dlogPdSigma, dlogPdMudMu):
    """Q [R, R, R] with ``m^T Q[i] m`` = ``dlogPdSigma[i] . pack(-m m^T) + 0.5 sum_ab dlogPdMudMu[i, a, b] m_a m_b``
    (ES.py:148-154): Q_i = (H_i + H_i^T) / 4 - (T_i + T_i^T) / 2, T_i the packed row unpacked into the lower triangle."""
    H = np.asarray(dlogPdMudMu, dtype=float)
    R = H.shape[0]
    T = np.zeros((R, R, R))
    T[:, lower_mask(R)] = np.asarray(dlogPdSigma, dtype=float)
    return 0.25 * (H + H.transpose(0, 2, 1)) - 0.5 * (T + T.transpose(0, 2, 1))


def score(m, logP, u, G, Q, W):
    """ES._compute_acq's value (ES.py:150-170) for the innovation ``m`` [R] of one candidate: the mean over the quantiles
    ``W`` of sum_i e^l (l + u_i), l the normalised predicted log belief.  (Not negated.)"""
    m = np.ravel(m)
    base = np.ravel(logP) + np.einsum('iab,a,b->i', Q, m, m)
    pred = base[:, None] + (G @ m)[:, None] * np.ravel(W)[None, :]
    top = np.amax(pred, axis=0)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        lse = top + np.log(np.sum(np.exp(pred - top), axis=0))
    pred = pred - (top if np.any(np.isinf(lse)) else lse)
    return float(np.mean(np.sum(np.exp(pred) * (pred + np.ravel(u)[:, None]), axis=0)))


class McmcSampler(object):
    """util/mcmc_sampler.py:5-27: ``get_samples(n_samples, log_p_function, burn_in_steps)`` -> (samples [n, D], log values
    [n, 1])."""

    def __init__(self, space):
        self.space = space

    def get_samples(self, n_samples, log_p_function, burn_in_steps=50):
        raise NotImplementedError


class AffineInvariantEnsembleSampler(McmcSampler):
    """Goodman & Weare's affine-invariant ensemble sampler (2010) with the stretch move, a = 2: ``n_samples`` walkers started
    from ``space.samples_uniform``, two half-ensembles updated in turn, ``burn_in_steps`` sweeps; the walkers' final positions
    are the samples (util/mcmc_sampler.py:29-59 runs emcee the same way).  The draws are not emcee's.  ``log_p_function`` is
    tried on the whole half-ensemble first -- ONE call per half step (the default proposal of AcquisitionEntropySearch takes a
    matrix: one device acquisition call) -- and row by row where it refuses a matrix with ValueError, as the reference's own
    proposal does.  ``seed``: a private generator, reproducible draws; None: NumPy's global one."""

    def __init__(self, space, seed=None):
        super(AffineInvariantEnsembleSampler, self).__init__(space)
        self.seed = seed

    @staticmethod
    def _log_p(log_p_function, X):
        try:
            vals = np.asarray(log_p_function(X), dtype=float).reshape(-1)
            if vals.shape[0] == X.shape[0]:
                return vals
        except ValueError:
            pass
        return np.array([float(np.ravel(log_p_function(x))[0]) for x in X])

    def get_samples(self, n_samples, log_p_function, burn_in_steps=50):
        rng = np.random if self.seed is None else np.random.RandomState(self.seed)
        n = int(n_samples)
        X = np.array(self.space.samples_uniform(n, rng), dtype=float).reshape(n, -1)
        D = X.shape[1]
        logp = self._log_p(log_p_function, X)
        halves = (np.arange(0, n // 2), np.arange(n // 2, n))
        for _ in range(int(burn_in_steps)):
            for mine, other in (halves, halves[::-1]):
                if mine.size == 0 or other.size == 0:
                    continue
                zz = (1.0 + rng.uniform(size=mine.size)) ** 2 / 2.0      # density ~ 1 / sqrt(z) on [1 / a, a], a = 2
                partner = X[other[rng.randint(other.size, size=mine.size)]]
                prop = partner + zz[:, None] * (X[mine] - partner)
                new = self._log_p(log_p_function, prop)
                with np.errstate(invalid='ignore'):
                    accept = np.log(rng.uniform(size=mine.size)) < (D - 1) * np.log(zz) + new - logp[mine]
                accept &= ~np.isnan(new)
                X[mine[accept]] = prop[accept]
                logp[mine[accept]] = new[accept]
        return X, logp.reshape(-1, 1)
