"""Entropy search stated once more, in NumPy long double, independently of the package: the EP sweeps of p_min (with sweep
counts, the last sum |d| of every chain and how close any z came to the +-6 thresholds), the closing algebra of a chain, the
renormalisation into a belief, and the ES score of one innovation.

Formulas: Cunningham, Hennig & Lacoste-Julien, "Gaussian probabilities and expectation propagation" (2011) as GPyOpt's
util/epmgp.py arranges them (min_faktor, lt_factor, log_relative_gauss, joint_min) and Hennig & Schuler (2012) as
acquisitions/ES.py:124-207 evaluates them.  The tests compare the device kernels and the package's host algebra with this file
and with the reference's own recorded outputs (tests/golden/es_epmgp.npz).
"""
import numpy as np
from scipy.special import erfc

LD = np.longdouble
SQ2 = np.sqrt(LD(2))
L2P = np.log(LD(2)) + np.log(LD(np.pi))
EPS32 = LD(np.finfo(np.float32).eps)


def _mx(a, b):
    return a + b if (a != a or b != b) else (a if a > b else b)


def _log_cdf(z):
    # erfc in double (what the reference and the device evaluate); the argument and the logarithm in long double
    return np.log(LD(0.5) * LD(erfc(float(-z / SQ2))))


def sweeps(mu, cov, max_sweeps=50, tol=1e-3):
    """dict(P, MP, logS [R, R - 1] float64, status, sweeps [R], last_diff [R] (sum |d| of the last complete sweep, NaN when a
    chain ended inside a sweep), z_margin: the smallest | |z| - 6 | met)."""
    mu, cov = np.asarray(mu, dtype=LD), np.asarray(cov, dtype=LD)
    R = mu.shape[0]
    P, MP, logS = (np.zeros((R, max(R - 1, 0)), dtype=LD) for _ in range(3))
    status, count = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    last = np.full(R, np.nan)
    margin = np.inf
    with np.errstate(all="ignore"):
        for k in range(R):
            M, V = mu.copy(), cov.copy()
            st, n = 1, 0
            while n < max_sweeps and st == 1:
                n += 1
                tot, ended = LD(0), False
                for i in range(R - 1):
                    l = i if i < k else i + 1
                    p, mp = P[k, i], MP[k, i]
                    cVc = (V[l, l] - 2 * V[k, l] + V[k, k]) / 2
                    Vc = (V[:, l] - V[:, k]) / SQ2
                    cM = (M[l] - M[k]) / SQ2
                    cv = _mx(cVc / (1 - p * cVc), LD(0))
                    cm = cM + cv * (p * cM - mp)
                    z = cm / np.sqrt(cv + LD(1e-25))
                    if z != z:
                        z = -np.inf
                    if np.isfinite(z):
                        margin = min(margin, abs(abs(float(z)) - 6.0))
                    if z < -6:
                        P[k, i], MP[k, i], logS[k, i] = 0, 0, -np.inf
                        st, ended = -1, True
                        break
                    if z > 6:
                        dp, dmp = -p, -mp
                        d = dp if dp > dmp else dmp
                        pn, mpn, ls = LD(0), LD(0), LD(0)
                    else:
                        lphi = -(z * z + L2P) / 2
                        lPhi = _log_cdf(z)
                        e = np.exp(lphi - lPhi)
                        al = e / np.sqrt(cv)
                        be = al * (al * cv + cm)
                        r = be / (1 - be)
                        dp = _mx(-p + EPS32, r / cv - p)
                        dmp = _mx(-mp + EPS32, r * (al + cm / cv) + al - mp)
                        d = _mx(dmp, dp)
                        pn, mpn = p + dp, mp + dmp
                        ls = lPhi - (np.log(be) - np.log(pn) - np.log(cv)) / 2 + (al * al) / (2 * be) * cv
                    den = 1 + dp * cVc
                    V = V - dp / den * np.outer(Vc, Vc)
                    M = M + (dmp - cM * dp) / den * Vc
                    P[k, i], MP[k, i], logS[k, i] = pn, mpn, ls
                    if np.any(np.isnan(V)):
                        st, ended = -2, True
                        break
                    if d != d:
                        st, ended = -1, True
                        break
                    tot += abs(d)
                if not ended:
                    last[k] = float(tot)
                    if abs(tot) < tol:
                        st = 0
            status[k], count[k] = st, n
    return dict(P=P.astype(float), MP=MP.astype(float), logS=logS.astype(float), status=status, sweeps=count, last_diff=last,
                z_margin=margin)


def lower_pack(A):
    R = A.shape[0]
    return np.array([A[a, b] for a in range(R) for b in range(a + 1)])


def closing(mu, cov, k, P, MP, logS):
    """(logZ, dlogZ/dmu [R], d2logZ/dmu dmu [R, R], dlogZ/dSigma packed) of chain k in long double, returned as float64."""
    mu, cov = np.asarray(mu, dtype=LD), np.asarray(cov, dtype=LD)
    P, MP, logS = (np.asarray(a, dtype=LD) for a in (P, MP, logS))
    R = mu.shape[0]
    C = np.zeros((R, R - 1), dtype=LD)
    for i in range(R - 1):
        C[i if i < k else i + 1, i] = 1 / SQ2
    C[k, :] = -1 / SQ2
    Rm = C * np.sqrt(P)[None, :]
    r = C @ MP
    mpm = sum((MP[i] * MP[i] / P[i] for i in range(R - 1) if MP[i] != 0), LD(0))
    inner = np.eye(R - 1, dtype=LD) + Rm.T @ cov @ Rm
    # long-double Cholesky and solves, written out (LAPACK has none)
    n = R - 1
    Lc = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lc[j, j] = np.sqrt(inner[j, j] - Lc[j, :j] @ Lc[j, :j])
        for i in range(j + 1, n):
            Lc[i, j] = (inner[i, j] - Lc[i, :j] @ Lc[j, :j]) / Lc[j, j]
    Y = np.zeros((n, R), dtype=LD)       # Lc Y = Rm^T
    for i in range(n):
        Y[i] = (Rm.T[i] - Lc[i, :i] @ Y[:i]) / Lc[i, i]
    A = Y.T @ Y
    A = (A + A.T) / 2
    b = mu + cov @ r
    Ab = A @ b
    logdet = 2 * np.sum(np.log(np.diagonal(Lc)))
    logZ = (r @ cov @ r - b @ Ab - logdet) / 2 + mu @ r + np.sum(logS) - mpm / 2
    Dm = -A - 2 * np.outer(r, Ab) + np.outer(r, r) + np.outer(b @ A, Ab)
    Dm = (Dm + Dm.T - np.diag(np.diagonal(Dm))) / 2
    return float(logZ), (r - Ab).astype(float), (-A).astype(float), lower_pack(Dm).astype(float)


def belief(mu, cov, sw=None):
    """(logP, dlogPdMu, dlogPdSigma, dlogPdMudMu) as the reference's joint_min(with_derivatives=True) returns them."""
    sw = sweeps(mu, cov) if sw is None else sw
    R = len(mu)
    logZ, dMu = np.full(R, -np.inf), np.zeros((R, R))
    dS, dMM = np.zeros((R, R * (R + 1) // 2)), np.zeros((R, R, R))
    for k in range(R):
        if sw["status"][k] >= 0:
            logZ[k], dMu[k], dMM[k], dS[k] = closing(mu, cov, k, sw["P"][k], sw["MP"][k], sw["logS"][k])
    logZ[np.isinf(logZ)] = -500.0
    w = np.exp(logZ)
    Z = w.sum()
    top = logZ.max()
    with np.errstate(divide="ignore"):
        s = top + np.log(np.sum(np.exp(logZ - top)))
    s = top if np.isinf(s) else s
    Zm = (w[:, None] * dMu).sum(0) / Z
    Zs = (w[:, None] * dS).sum(0) / Z
    gg = np.einsum("kij,k->ij", dMM + np.einsum("ki,kj->kij", dMu, dMu), w) / Z
    adds = -gg + Zm * Zm       # the reference's broadcast of a vector of squares (epmgp.py:116-117), not an outer product
    return logZ - s, dMu - Zm, dS - Zs, dMM + adds[None, :, :]


def det_reference_style(m, dlogPdSigma, dlogPdMudMu):
    """The deterministic change of ES.py:145-154 for the innovation m, term by term as the reference combines them."""
    m = np.asarray(m, dtype=LD).reshape(-1, 1)
    R = m.shape[0]
    dV = -(m @ m.T)
    packed = np.array([dV[a, b] for a in range(R) for b in range(a + 1)], dtype=LD)
    mm = m @ m.T
    trace = np.array([np.sum(np.asarray(dlogPdMudMu[i], dtype=LD) * mm) for i in range(R)], dtype=LD)
    return (np.asarray(dlogPdSigma, dtype=LD) @ packed + trace / 2).astype(float)


def score(m, logP, u, G, det, W):
    """-mean_w sum_i e^l (l + u_i) in long double: ``det`` [R] the deterministic change, G = dlogPdMu, W the quantiles; the
    normaliser falls back to the maximum for every w when any w's log-sum-exp is infinite (ES.py:159-164)."""
    m, logP, u, det, W = (np.asarray(a, dtype=LD).ravel() for a in (m, logP, u, det, W))
    g = np.asarray(G, dtype=LD) @ m
    pred = (logP + det)[:, None] + g[:, None] * W[None, :]
    top = pred.max(axis=0)
    with np.errstate(all="ignore"):
        lse = top + np.log(np.sum(np.exp(pred - top), axis=0))
    pred = pred - (top if np.any(np.isinf(lse)) else lse)
    return -float(np.mean(np.sum(np.exp(pred) * (pred + u[:, None]), axis=0)))
