"""The joint expected improvement qEI and its gradient in ``np.longdouble`` (x87 80-bit, eps 1.1e-19) from the raw data -- a
kernel build, Cholesky and substitutions of its own, no inverse factor -- and the case table of tests/test_gpu_qei.py and
tests/test_qei_truth_host.py.  ``evaluate(dtype=np.float64)`` is the same algorithm in plain float64: the yardstick of the
device's gradient error.  Nothing here imports the library or needs a GPU; everything is computed once per case and read-only.

    k_i = k(X, x_i),  m_i = k_i^T alpha,  v_i = L^-1 k_i,  beta_i = L^-T v_i          (L L^T = K + d I, d = noise + 1e-8 + jitter)
    Sigma_ij = k(x_i, x_j) - v_i . v_j  (+ noise on the diagonal);   m' = y_std m + y_mean,  Sigma' = y_std^2 Sigma
    C = chol(Sigma'),  y_s = m' + C z_s,  I_sj = fmin - par - y_sj,  j*(s) = argmax_j I_sj (lowest j on a tie), active: I_{s j*} > 0
    qEI = (1 / S) sum_active I_{s j*}
    mbar_j = -(1 / S) #{active s: j* = j},  Cbar_jl = -(1 / S) sum_{active s, j* = j} z_sl (l <= j)
    P = tril(C^T Cbar), diagonal halved;  Sigma_bar = sym(C^-T P C^-1);  A = 2 Sigma_bar
    d qEI / d x_i = y_std mbar_i J_i^T alpha + y_std^2 (sum_j A_ij dk(x_i, x_j)/dx_i - J_i^T sum_j A_ij beta_j)
J_i the [N, D] input Jacobian of k(X, x_i); dk/dx_q = dK_dr (x_q - X_nq) / (l_q^2 r), 0 where r = 0 (the _inv_dist convention).

f_min is PASSED IN: each case takes fmin - par as the midpoint between the two middle order statistics, over the samples, of
min_j y_sj -- exactly half the samples are active -- and, for S = 1, the sample's min_j y_sj plus half the posterior standard
deviation of that location.  The selection of j* and of the active set is discontinuous, so every case must keep every sample's
margin (|I_{s j*}|, for active samples also the gap to the runner-up) at least 1000 value allowances wide: ``conditions`` computes
what tests/test_qei_truth_host.py asserts.  The seeds below were chosen on the CPU under these conditions.
"""
import collections
import functools

import numpy as np

T = np.longdouble
FAMILY_ID = {"rbf": 0, "Mat52": 1, "Mat32": 2, "Exponential": 3}      # GP_KERNEL_* of include/gphip.h
VARIANCE = 1.3
Y_MEAN, Y_STD = 0.3, 1.7      # the output normaliser of every evaluation
PAR = 0.01                    # the acquisition's jitter
MARGIN_FACTOR = 1000.0

# N 130 / 300 / 1100: two 128-row blocks, three, two 1024-column chunks; q 1, 2..4 and 5..8: the three pass layouts
Case = collections.namedtuple("Case", "id N D q S fam ard noise qres seed ls_scale")
TABLE = (
    Case("a", 130, 2, 2, 64, "rbf", False, 1e-2, 2, 0, 0.3),            # two row blocks, the narrow pass
    Case("b", 300, 3, 8, 256, "Mat52", True, 1e-2, 8, 0, 0.3),          # the wide pass, full q
    Case("c", 300, 16, 8, 256, "rbf", True, 1e-2, 8, 0, 0.3),           # q D = 128, the limit of ROWS_MAX_XS
    Case("d", 1100, 4, 5, 1000, "Mat32", False, 1e-6, 5, 240, 0.1),       # two column chunks; S no multiple of 64 or 256; exact_feval's noise
    Case("e", 300, 3, 1, 64, "Exponential", False, 1e-2, 1, 0, 0.3),    # q = 1
    Case("f", 300, 3, 4, 1, "rbf", False, 1e-2, 4, 0, 0.3),             # S = 1
    Case("g", 300, 3, 3, 128, "Mat52", False, 1e-2, 8, 0, 0.3),         # a location on a training input; resident q = 8, the call uses 3
)
CASES = {c.id: c for c in TABLE}
Problem = collections.namedtuple("Problem", "case X Y ls ls_arg Xq Z")
Truth = collections.namedtuple("Truth", "mean cov value grad mbar Sbar imp jstar active")


def rel_tol(noise):
    """tests/test_gpu_rows.py: what two float64 routes over the same inverse factor are granted."""
    return 1e-9 if noise >= 1e-4 else 2e-6


def sigma2(noise, jitter=0.0):
    """The diagonal of the factor, as the library forms it in double."""
    return (float(noise) + 1e-8) + float(jitter)


def response(X):
    return np.sin(3.0 * X.sum(1)) + 0.5 * np.cos(5.0 * X[:, 0])


def locations(c, X, seed):
    """The batch and the base samples of a case from ``seed`` (the data do not depend on it)."""
    rng = np.random.default_rng(9100 + 131 * ord(c.id) + seed)
    Xq = rng.uniform(0, 1, (c.q, c.D))
    if c.id == "g":
        Xq[1] = X[17]
    Z = rng.standard_normal((c.S, c.qres))
    return Xq, Z


@functools.lru_cache(maxsize=None)
def problem(cid):
    c = CASES[cid]
    rng = np.random.default_rng(9000 + ord(cid))
    X = rng.uniform(0, 1, (c.N, c.D))
    Y = (response(X) + 0.1 * rng.standard_normal(c.N))[:, None]
    Y = (Y - Y.mean()) / Y.std()
    base = c.ls_scale * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.7, 1.4, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    Xq, Z = locations(c, X, c.seed)
    for a in (X, Y, ls_arg, ls, Xq, Z):
        a.setflags(write=False)
    return Problem(c, X, Y, ls, ls_arg, Xq, Z)


# ---- the arithmetic, in the dtype of its operands ----------------------------------------------------------------------------------
def chol(A):
    """Unblocked left-looking Cholesky; a non-positive pivot is an error of the test's inputs."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def solve(L, B, trans=0):
    """L X = B (trans 0) or L^T X = B (trans 1)."""
    X = np.array(B, dtype=L.dtype, copy=True)
    n = L.shape[0]
    if trans == 0:
        for i in range(n):
            X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def k_of_r(fam, variance, r):
    t = r.dtype.type
    if fam == "rbf":
        return variance * np.exp(-t(0.5) * r * r)
    if fam == "Mat52":
        s5 = np.sqrt(t(5))
        return variance * (1 + s5 * r + t(5) / 3 * r * r) * np.exp(-s5 * r)
    if fam == "Mat32":
        s3 = np.sqrt(t(3))
        return variance * (1 + s3 * r) * np.exp(-s3 * r)
    assert fam == "Exponential"
    return variance * np.exp(-r)


def dk_dr_over_r(fam, variance, r):
    """dK_dr / r, 0 where r = 0."""
    t = r.dtype.type
    if fam == "rbf":
        g = -k_of_r(fam, variance, r)
    elif fam == "Mat52":
        s5 = np.sqrt(t(5))
        g = -(t(5) / 3) * variance * (1 + s5 * r) * np.exp(-s5 * r)
    elif fam == "Mat32":
        g = -3 * variance * np.exp(-np.sqrt(t(3)) * r)
    else:
        g = -k_of_r(fam, variance, r) / np.where(r == 0, t(1), r)
    return np.where(r == 0, t(0), g)


def _scaled_diff(A, B, ls):
    diff = (A[:, None, :] - B[None, :, :]) / ls
    return diff, np.sqrt((diff * diff).sum(-1))


Fit = collections.namedtuple("Fit", "X ls L alpha")


def fit(fam, variance, ls, d, X, y, dtype=T):
    X, ls = np.asarray(X, dtype=dtype), np.asarray(ls, dtype=dtype)
    y = np.asarray(y, dtype=dtype).ravel()
    _, r = _scaled_diff(X, X, ls)
    K = k_of_r(fam, dtype(variance), r) + dtype(d) * np.eye(X.shape[0], dtype=dtype)
    L = chol(K)
    alpha = solve(L, solve(L, y, 0), 1)
    return Fit(X, ls, L, alpha)


def posterior(fam, variance, noise_add, f, Xq, y_mean=Y_MEAN, y_std=Y_STD, parts=False):
    """De-normalised joint mean [q] and covariance [q, q] of the rows of Xq."""
    t = f.X.dtype.type
    Xq = np.asarray(Xq, dtype=t)
    dX, rX = _scaled_diff(Xq, f.X, f.ls)
    k = k_of_r(fam, t(variance), rX)                                    # [q, N]
    v = solve(f.L, k.T, 0)                                              # [N, q]
    dq, rq = _scaled_diff(Xq, Xq, f.ls)
    Sig = k_of_r(fam, t(variance), rq) - v.T @ v + t(noise_add) * np.eye(Xq.shape[0], dtype=t)
    Sig = (Sig + Sig.T) / 2
    m = k @ f.alpha
    mean, cov = t(y_std) * m + t(y_mean), t(y_std) ** 2 * Sig
    return (mean, cov, dX, rX, v, dq, rq) if parts else (mean, cov)


def evaluate(fam, variance, noise_add, f, Xq, Z, t0, y_mean=Y_MEAN, y_std=Y_STD, grad=True, dtype=None):
    """qEI of the batch Xq over the base samples Z (their leading q columns) with t0 = fmin - par, in the arithmetic of the fit
    ``f``: a ``Truth``."""
    t = f.X.dtype.type
    q = np.shape(Xq)[0]
    Z = np.asarray(Z, dtype=t)[:, :q]
    S = Z.shape[0]
    mean, cov, dX, rX, v, dq, rq = posterior(fam, variance, noise_add, f, Xq, y_mean, y_std, parts=True)
    C = chol(cov)
    Ys = mean[None, :] + Z @ C.T
    imp = t(t0) - Ys
    jstar = np.argmax(imp, axis=1)                                      # the first of the maxima: the lowest j on a tie
    best = imp[np.arange(S), jstar]
    active = best > 0
    value = np.where(active, best, t(0)).sum() / S
    if not grad:
        return Truth(mean, cov, value, None, None, None, imp, jstar, active)
    mbar, Cbar = np.zeros(q, dtype=t), np.zeros((q, q), dtype=t)
    for s in np.flatnonzero(active):
        j = jstar[s]
        mbar[j] -= t(1) / S
        Cbar[j, :j + 1] -= Z[s, :j + 1] / S
    P = np.tril(C.T @ Cbar)
    P[np.diag_indices(q)] *= t(0.5)
    Tm = solve(C, solve(C, P, 1).T, 1).T                                # C^-T P C^-1
    Sbar = (Tm + Tm.T) / 2
    A = 2 * Sbar
    beta = solve(f.L, v, 1)                                             # [N, q]
    gX = dk_dr_over_r(fam, t(variance), rX)                             # [q, N]
    gq = dk_dr_over_r(fam, t(variance), rq)                             # [q, q]
    g = np.zeros((q, f.X.shape[1]), dtype=t)
    for i in range(q):
        Ji = gX[i][:, None] * dX[i] / f.ls                              # [N, D]
        Jq = gq[i][:, None] * dq[i] / f.ls                              # [q, D]: dk(x_i, x_j) / dx_i
        g[i] = t(y_std) * mbar[i] * (Ji.T @ f.alpha) + t(y_std) ** 2 * (A[i] @ Jq - Ji.T @ (beta @ A[i]))
    return Truth(mean, cov, value, g, mbar, Sbar, imp, jstar, active)


def threshold(imp0, cov, jstar0):
    """t0 = fmin - par from the improvements at t0 = 0 (imp0 = -y): half the samples active; S = 1: the sample active by half the
    posterior standard deviation of its best location."""
    ymin = (-imp0).min(axis=1)
    S = ymin.size
    if S == 1:
        return float(ymin[0] + np.sqrt(cov[jstar0[0], jstar0[0]]) / 2)
    srt = np.sort(ymin)
    return float((srt[S // 2 - 1] + srt[S // 2]) / 2)


def tolerances(noise, mean_norm_max, variance=VARIANCE, y_std=Y_STD):
    """The absolute tolerances of the de-normalised mean and covariance: tests/test_gpu_rows.py's relative ones on max(1, max |m|)
    and on the prior variance, carried through the normaliser."""
    r = rel_tol(noise)
    return r * max(1.0, mean_norm_max) * y_std, r * variance * y_std ** 2


def value_allowance(noise, tr, t0, variance=VARIANCE, y_mean=Y_MEAN, y_std=Y_STD, par=PAR):
    """First order from the adjoint: sum_j |mbar_j| tol_m + sum_ij |Sigma_bar_ij| tol_Sigma, and a rounding floor of 64 eps
    (|fmin| + max |y|)."""
    m_norm = float(np.max(np.abs((tr.mean - T(y_mean)) / T(y_std))))
    tol_m, tol_S = tolerances(noise, m_norm, variance, y_std)
    ymax = float(np.max(np.abs(T(t0) - tr.imp)))
    return (float(np.abs(tr.mbar).sum()) * tol_m + float(np.abs(tr.Sbar).sum()) * tol_S
            + 64 * np.finfo(np.float64).eps * (abs(t0 + par) + ymax))


def margins(tr):
    """(the smallest |I_{s j*}| over all samples, the smallest gap to the runner-up over the active ones)."""
    S, q = tr.imp.shape
    best = tr.imp[np.arange(S), tr.jstar]
    m0 = float(np.min(np.abs(best)))
    if q == 1 or not tr.active.any():
        return m0, np.inf
    srt = np.sort(tr.imp, axis=1)
    return m0, float(np.min((srt[:, -1] - srt[:, -2])[tr.active]))


Solved = collections.namedtuple("Solved", "p fit t0 fmin truth allowance")


def solve_case(c, p, jitter=0.0, dtype=T, t0=None):
    f = fit(c.fam, VARIANCE, p.ls, sigma2(c.noise, jitter), p.X, p.Y, dtype)
    if t0 is None:
        tr0 = evaluate(c.fam, VARIANCE, c.noise, f, p.Xq, p.Z, 0.0, grad=False)
        t0 = threshold(tr0.imp, tr0.cov, tr0.jstar)
    tr = evaluate(c.fam, VARIANCE, c.noise, f, p.Xq, p.Z, t0)
    return Solved(p, f, t0, t0 + PAR, tr, value_allowance(c.noise, tr, t0))


@functools.lru_cache(maxsize=None)
def truth(cid, jitter=0.0):
    """The long-double truth of a case at the jitter the device's fit ended with (0 for every case here)."""
    return solve_case(CASES[cid], problem(cid), jitter, T)


@functools.lru_cache(maxsize=None)
def float64_restatement(cid, jitter=0.0):
    """The same algorithm in plain float64 at the truth's threshold."""
    return solve_case(CASES[cid], problem(cid), jitter, np.float64, truth(cid, jitter).t0)


def conditions(sv):
    """What a case must satisfy: (active share, smallest margin, the margin it needs)."""
    m0, m1 = margins(sv.truth)
    return float(np.mean(sv.truth.active)), min(m0, m1), MARGIN_FACTOR * sv.allowance


# ---- q = 1 against the closed form ------------------------------------------------------------------------------------------------------
def stratified_normals(S=4096):
    """The normal quantiles at the S stratum midpoints (s + 1/2) / S: a midpoint rule for E[.] under N(0, 1)."""
    from statistics import NormalDist
    nd = NormalDist()
    return np.array([nd.inv_cdf((s + 0.5) / S) for s in range(S)])[:, None]


def closed_form_ei(m, s, t0):
    """EI of acquisitions.get_quantiles: s (u Phi(u) + phi(u)), u = (fmin - par - m) / s, in long double."""
    from math import erfc
    u = (T(t0) - T(m)) / T(s)
    phi = np.exp(-u * u / 2) / np.sqrt(2 * T(np.pi))
    Phi = T(erfc(float(-u / np.sqrt(T(2))))) / 2
    return float(T(s) * (u * Phi + phi))


def quadrature_error(m, s, t0, S=4096):
    """|stratified estimate - closed form| of the one-dimensional EI at (m, s): the midpoint rule's error, computed, not assumed."""
    z = np.asarray(stratified_normals(S)[:, 0], dtype=T)
    est = float(np.maximum(T(t0) - (T(m) + T(s) * z), 0).sum() / S)
    return abs(est - closed_form_ei(m, s, t0))
