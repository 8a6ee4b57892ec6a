"""GP classification by Laplace's method with a probit link in ``np.longdouble`` (x87 80-bit, eps 1.1e-19): the sites, the Newton
iteration run to stationarity, log Z and its gradient, the latent posterior with its x-gradients, p(y = 1 | x), a float64 NumPy
replica of the device's iteration, and the case table of tests/test_gpu_laplace.py and tests/test_laplace_truth_host.py.

Rasmussen & Williams, Gaussian Processes for Machine Learning, Algorithms 3.1 and 5.1.  Labels y in {-1, +1}, K without noise and
without 1e-8, z = y f, n = phi(z) / Phi(z):

    log p = log Phi(z),  g = y n,  W = max(n (n + z), 1e-20),  t = y (n (z^2 - 1) + 3 z n^2 + 2 n^3)
    mode:  a = g(K a);  B = I + W^1/2 K W^1/2 = L L^T;  log Z = -a.f / 2 + sum log p - sum log L_ii
    R = W^1/2 B^-1 W^1/2 = (K + W^-1)^-1,  s2 = diag(K - K R K) t / 2,  u = (I - R K) s2
    d log Z / d theta = sum_ij G_ij dK_ij / d theta,  G = (a a^T - R + u a^T + a u^T) / 2
    latent posterior at x:  m = k*.a,  s^2 = k** - k*.R k*;  p(y = 1 | x) = Phi(m / sqrt(1 + s^2))

The W floor is part of the definition (reached only for y f >~ 9.5).  Nothing here imports the library or the oracle or needs a
GPU; everything is computed once per case (functools.lru_cache) and read-only.  The Cholesky factorisation is written out in long
double, O(N^3) in Python, so no case is larger than N = 300.

log Phi is long double throughout (tests/_feas_truth.py takes erfc from scipy in double, which leaves 1e-16 of relative noise in
phi / Phi -- above the stationarity asked of the mode here): with x = |z| / sqrt 2, erfc(x) for x >= 1 by the continued fraction
e^-x^2 / sqrt pi / (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...)))) evaluated bottom-up over 600 levels (error below e^-60 at x = 1),
for x < 1 as 1 - erf(x) with erf(x) = 2 / sqrt pi e^-x^2 sum_n 2^n x^(2n+1) / (2n+1)!! (positive terms).  log Phi(z) is the
logarithm of that tail for z <= 0 -- formed without the underflow, -x^2 - log(pi) / 2 + log(fraction) -- and log1p of minus it above.
"""
import collections
import functools

import numpy as np

T = np.longdouble
HALF_LOG_2PI = T("0.918938533204672741780329736405617639861")
HALF_LOG_PI = T("0.572364942924700087071713675676529355824")
LOG_2 = T("0.693147180559945309417232121458176568076")


def _log_half_erfc(x):
    """log(erfc(x) / 2) for x >= 0 [array], long double."""
    x = np.asarray(x, dtype=T)
    out = np.empty(x.shape, T)
    big = x >= 1
    xb = x[big]
    if xb.size:
        cf = xb.copy()
        for k in range(600, 0, -1):
            cf = xb + (T(k) / 2) / cf
        out[big] = -xb * xb - HALF_LOG_PI - np.log(cf) - LOG_2
    xs = x[~big]
    if xs.size:
        term = xs.copy()
        tot = xs.copy()
        for n in range(1, 200):
            term = term * 2 * xs * xs / (2 * n + 1)
            tot = tot + term
        erf = 2 * np.exp(-xs * xs - HALF_LOG_PI) * tot
        out[~big] = np.log((1 - erf) / 2)
    return out


def log_ndtr(z):
    """log Phi(z) [shape of z] in long double."""
    z = np.asarray(z, dtype=T)
    q = _log_half_erfc(np.abs(z) / np.sqrt(T(2)))
    return np.where(z <= 0, q, np.log1p(-np.exp(q)))

W_FLOOR = T(1e-20)
CAP = 40

# ---- covariances ------------------------------------------------------------------------------------------------------------------
FAMILIES = ("RBF", "Mat52", "Mat32", "Exponential")


def _k_g(fam, variance, r2):
    """k(r) and g = (dk/dr) / r (0 where r = 0 and the quotient has no limit: the Exponential) at squared scaled distances r2."""
    r2 = np.asarray(r2)
    r = np.sqrt(r2)
    v = r2.dtype.type(variance)
    if fam == "RBF":
        k = v * np.exp(-r2 / 2)
        return k, -k
    if fam == "Mat52":
        s5 = np.sqrt(r2.dtype.type(5))
        e = np.exp(-s5 * r)
        return v * (1 + s5 * r + 5 * r2 / 3) * e, -(v * 5 / 3) * (1 + s5 * r) * e
    if fam == "Mat32":
        s3 = np.sqrt(r2.dtype.type(3))
        e = np.exp(-s3 * r)
        return v * (1 + s3 * r) * e, -3 * v * e
    k = v * np.exp(-r)
    safe = np.where(r2 == 0, 1, r)
    return k, np.where(r2 == 0, 0, -k / safe)


def _diffs(X1, X2, ls):
    """(x1 - x2) / l, [N1, N2, D]."""
    return (X1[:, None, :] - X2[None, :, :]) / ls[None, None, :]


def cov(fam, variance, ls, X1, X2, dtype=T):
    d = _diffs(np.asarray(X1, dtype), np.asarray(X2, dtype), np.asarray(ls, dtype))
    return _k_g(fam, variance, (d * d).sum(2))[0]


# ---- long-double linear algebra ---------------------------------------------------------------------------------------------------
def chol(A):
    """Lower Cholesky factor, row by row in the dtype of A."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("pivot %d" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, Bm):
    """L^-1 Bm (Bm [n] or [n, m])."""
    X = np.array(Bm, dtype=L.dtype)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_upper_t(L, Bm):
    """L^-T Bm."""
    X = np.array(Bm, dtype=L.dtype)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def matvec(K, v):
    """K v with a compensated (Neumaier) sum over the columns: f = K a cancels heavily (sum |K_ij a_j| ~ 10^3 |f_i| at N = 300 under
    a large variance), and a plain long-double sum would leave the mode's residual at 2e-16."""
    s = np.zeros(K.shape[0], K.dtype)
    c = np.zeros(K.shape[0], K.dtype)
    for j in range(K.shape[1]):
        p = K[:, j] * v[j]
        t = s + p
        c = c + np.where(np.abs(s) >= np.abs(p), (s - t) + p, (p - t) + s)
        s = t
    return s + c


# ---- sites ------------------------------------------------------------------------------------------------------------------------
Sites = collections.namedtuple("Sites", "logp g W t n")


def sites(y, f):
    """The probit sites at latent values f under labels y (long double, the W floor applied)."""
    y, f = np.asarray(y, dtype=T), np.asarray(f, dtype=T)
    z = y * f
    lp = log_ndtr(z)
    n = np.exp(-z * z / 2 - HALF_LOG_2PI - lp)
    W = np.maximum(n * (n + z), W_FLOOR)
    t = y * (n * (z * z - 1) + 3 * z * n * n + 2 * n * n * n)
    return Sites(lp, y * n, W, t, n)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# N = 40 the small baseline; 127, 128, 129 around one 128 tile; 300 three tiles with a ragged last one, once more with the look-ahead
# factorisation forced inside the Newton loop (`lookahead`: set_option("lookahead_min_tiles", 0) as tests/test_gpu_lookahead.py; the
# truth is the base case's).  All four families, iso and ARD, variance 1 ... 100.  Edge cases: `sep` strongly separated labels under
# a large variance (W below 1e-10), `rare` a class share below 0.2, `twin` coincident inputs under the Exponential family.
Case = collections.namedtuple("Case", "id fam ard N D variance kind lookahead base")
TABLE = (
    Case("a", "RBF", False, 40, 2, 1.0, "", False, "a"),
    Case("b", "Mat52", True, 127, 3, 4.0, "", False, "b"),
    Case("c", "Mat32", False, 128, 3, 10.0, "", False, "c"),
    Case("d", "Exponential", True, 129, 3, 2.0, "twin", False, "d"),
    Case("e", "Mat52", False, 300, 4, 25.0, "rare", False, "e"),
    Case("f", "RBF", True, 300, 4, 100.0, "sep", False, "f"),
    Case("fl", "RBF", True, 300, 4, 100.0, "sep", True, "f"),
    Case("g", "Mat32", True, 40, 2, 3.0, "", False, "g"),
    Case("h", "Exponential", False, 40, 2, 50.0, "sep", False, "h"),
)
CASES = {c.id: c for c in TABLE}
M_LOC = 9   # test locations: rows calls of 1, 4 (narrow), 8 (wide) and 9 (a second group), the table of all
Problem = collections.namedtuple("Problem", "case X y labels01 ls ls_arg Xs")


@functools.lru_cache(maxsize=None)
def problem(cid):
    c = CASES[CASES[cid].base]
    rng = np.random.default_rng(7100 + sum(ord(ch) for ch in c.id))
    X = rng.uniform(0, 1, (c.N, c.D))
    if c.kind == "twin":
        X[5] = X[3]
        X[77] = X[3]
        X[128] = X[100]
    w = np.cos(0.9 * np.arange(1, c.D + 1))
    if c.kind == "sep":
        lat = 8.0 * (X[:, 0] - 0.5)                       # a clean boundary: every label is the sign, none is flipped
        lat = np.where(np.abs(lat) < 0.4, np.sign(lat + 1e-9) * 0.4, lat)
        y = np.sign(lat)
    else:
        lat = np.sin(3.0 * X @ w / np.sqrt(c.D)) + 0.4 * np.cos(5.0 * X[:, 0])
        if c.kind == "rare":
            lat = lat - np.quantile(lat, 0.86)            # about one label in seven is +1
        y = np.sign(lat + 0.25 * rng.standard_normal(c.N))
    y[y == 0] = 1.0
    if c.kind == "twin":
        y[5], y[77] = y[3], -y[3]                        # coincident inputs: one agrees, one contradicts
    base = 0.35 * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.7, 1.4, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    Xs = rng.uniform(0, 1, (M_LOC, c.D))
    Xs[1] = X[2]                                          # one location on a training point
    labels01 = (y > 0).astype(np.float64)[:, None]
    for a in (X, y, labels01, ls, ls_arg, Xs):
        a.setflags(write=False)
    return Problem(c, X, y, labels01, ls, ls_arg, Xs)


# ---- the mode ---------------------------------------------------------------------------------------------------------------------
Fit = collections.namedtuple("Fit", "a f W t g logZ logdetB iters resid K L")


def _newton(K, y, max_iter=200):
    """Newton's iteration in a to stationarity in long double: |a - g(K a)|_inf below 1e-16 of its scale (returns the residual)."""
    N = K.shape[0]
    a = np.zeros(N, T)
    f = np.zeros(N, T)
    psi_old = N * np.log(T(0.5))
    I = np.eye(N, dtype=T)
    for it in range(1, max_iter + 1):
        s = sites(y, f)
        sw = np.sqrt(s.W)
        L = chol(I + sw[:, None] * K * sw[None, :])
        # the step in correction form, da = (I + W K)^-1 (g - a) = r - W^1/2 B^-1 W^1/2 K r (the same step as b - W^1/2 B^-1 W^1/2 K b
        # minus a, since f = K a): its rounding error is relative to the shrinking da, not to a
        r = s.g - a
        da = r - sw * solve_upper_t(L, solve_lower(L, sw * (K @ r)))
        df = K @ da
        step = T(1)
        while True:
            an, fn = a + step * da, f + step * df
            psi = -(an @ fn) / 2 + sites(y, fn).logp.sum()
            if psi >= psi_old - T(1e-17) * max(T(1), abs(psi_old)) or step < T(1e-9):
                break
            step = step / 2
        a, psi_old = an, psi
        f = matvec(K, a)                            # (afresh: no drift from the accumulated steps)
        resid = np.abs(a - sites(y, f).g).max()
        if resid <= T(1e-16) * max(np.abs(a).max(), T(1e-300)):
            return a, f, it, resid
    raise RuntimeError("the truth's Newton iteration did not reach stationarity")


def fit_k(K, y):
    """The Laplace fit of labels y under the kernel matrix K (long double)."""
    K = np.asarray(K, dtype=T)
    a, f, it, resid = _newton(K, np.asarray(y, dtype=T))
    s = sites(y, f)
    sw = np.sqrt(s.W)
    L = chol(np.eye(K.shape[0], dtype=T) + sw[:, None] * K * sw[None, :])
    ldb = 2 * np.log(np.diag(L)).sum()
    logZ = -(a @ f) / 2 + s.logp.sum() - ldb / 2
    return Fit(a, f, s.W, s.t, s.g, logZ, ldb, it, resid, K, L)


def params_fit(fam, variance, ls, X, y):
    return fit_k(cov(fam, variance, ls, X, X), y)


@functools.lru_cache(maxsize=None)
def fit(cid):
    p = problem(cid)
    return params_fit(p.case.fam, p.case.variance, p.ls, p.X, p.y)


def _R(ft):
    """R = W^1/2 B^-1 W^1/2 = (K + W^-1)^-1."""
    sw = np.sqrt(ft.W)
    C = solve_lower(ft.L, np.diag(sw))          # L^-1 W^1/2
    return C.T @ C


@functools.lru_cache(maxsize=None)
def gradient(cid):
    """d log Z / d (variance, lengthscale(s)) [1 + nls], the implicit part included (long double)."""
    p = problem(cid)
    c = p.case
    ft = fit(cid)
    K = ft.K
    R = _R(ft)
    sw = np.sqrt(ft.W)
    C = solve_lower(ft.L, sw[:, None] * K)      # L^-1 W^1/2 K
    s2 = (np.diag(K) - (C * C).sum(0)) * ft.t / 2
    u = s2 - R @ (K @ s2)
    G = (np.outer(ft.a, ft.a) - R + np.outer(u, ft.a) + np.outer(ft.a, u)) / 2
    d = _diffs(p.X.astype(T), p.X.astype(T), p.ls.astype(T))
    r2 = (d * d).sum(2)
    _, g = _k_g(c.fam, c.variance, r2)
    out = [(G * K).sum() / T(c.variance)]
    if c.ard:
        for q in range(c.D):                    # dK / dl_q = -g d_q^2 / l_q
            out.append(-(G * g * d[:, :, q] ** 2).sum() / T(p.ls[q]))
    else:
        out.append(-(G * g * r2).sum() / T(p.ls[0]))
    return np.array(out, dtype=T)


Posterior = collections.namedtuple("Posterior", "mean var dmdx dvdx p tol_p")


@functools.lru_cache(maxsize=None)
def posterior(cid):
    """The latent posterior at the case's locations: mean, variance (no noise) [M], their x-gradients [M, D], p(y = 1 | x) [M] and
    tol_p [M], what the posterior tolerances of the GPU tests (mean 1e-6 max(1, |m|), sd 1e-6 sd + 1e-12 on sqrt(s^2 + 1))
    propagate to through Phi: |dp| <= phi(z) (dm / sd + |z| dsd / sd), z = m / sd."""
    p = problem(cid)
    c = p.case
    ft = fit(cid)
    Xs, X, ls = p.Xs.astype(T), p.X.astype(T), p.ls.astype(T)
    d = _diffs(Xs, X, ls)
    ks, g = _k_g(c.fam, c.variance, (d * d).sum(2))
    R = _R(ft)
    beta = ks @ R
    mean = ks @ ft.a
    var = T(c.variance) - (beta * ks).sum(1)
    gx = g[:, :, None] * d / ls[None, None, :]      # d k(x, x_n) / dx_q
    dmdx = np.einsum("mnq,n->mq", gx, ft.a)
    dvdx = -2 * np.einsum("mnq,mn->mq", gx, beta)
    sd = np.sqrt(1 + var)
    z = mean / sd
    prob = np.exp(log_ndtr(z))
    phi = np.exp(-z * z / 2 - HALF_LOG_2PI)
    tol_p = phi * (T(1e-6) * np.maximum(1, np.abs(mean)) / sd + np.abs(z) * (T(1e-6) * sd + T(1e-12)) / sd)
    return Posterior(mean, var, dmdx, dvdx, prob, tol_p)


# ---- the device's iteration in float64 NumPy --------------------------------------------------------------------------------------
F64 = collections.namedtuple("F64", "a f logZ logdetB iters halvings converged wmin")


def _sites64(y, f):
    s = sites(y, f)
    return tuple(np.asarray(v, dtype=np.float64) for v in (s.logp, s.g, s.W))


@functools.lru_cache(maxsize=None)
def newton_f64(cid):
    """The iteration as the library runs it -- start, direction, halving, stopping rule -- in float64 NumPy."""
    p = problem(cid)
    c = p.case
    K = cov(c.fam, c.variance, p.ls, p.X, p.X, np.float64)
    y = p.y
    N = c.N
    a, f = np.zeros(N), np.zeros(N)
    psi_old, stalls, halvings = N * np.log(0.5), 0, 0
    for it in range(1, CAP + 1):
        _, g, W = _sites64(y, f)
        sw = np.sqrt(W)
        L = np.linalg.cholesky(np.eye(N) + sw[:, None] * K * sw[None, :])
        b = W * f + g
        sol = np.linalg.solve(L.T, np.linalg.solve(L, sw * (K @ b)))
        da = (b - sw * sol) - a
        df = K @ da
        step, tol = 1.0, 1e-12 * max(1.0, abs(psi_old))
        while True:
            an, fn = a + step * da, f + step * df
            lp = _sites64(y, fn)[0].sum()
            psi = -0.5 * (an @ fn) + lp
            if psi >= psi_old - tol or step < 2.0 ** -30:
                break
            step *= 0.5
            halvings += 1
        small = step * np.abs(da).max() <= 1e-10 * np.abs(an).max()
        stalls = stalls + 1 if abs(psi - psi_old) <= 1e-13 * max(1.0, abs(psi_old)) else 0
        a, f, psi_old = an, fn, psi
        if small or stalls >= 2:
            ldb = 2.0 * np.log(np.diag(L)).sum()
            return F64(a, f, -0.5 * (a @ f) + lp - 0.5 * ldb, ldb, it, halvings, True, W.min())
    return F64(a, f, np.nan, np.nan, CAP, halvings, False, np.nan)
