"""Max-value entropy search (Wang & Jegelka 2017, mirrored for a minimum) in ``np.longdouble`` (x87 80-bit, eps 1.1e-19), the
rounding-error bound of the device's evaluation of it (``mes_terms`` / ``mes_h``, csrc/acq_math.h; the two-level sum of
csrc/mes.hip), the propagation of a posterior tolerance through it, and the case table of tests/test_gpu_mes.py and
tests/test_mes_truth_host.py.

    m = mean y_std + y_mean,  s = sqrt(max(var y_std^2, 1e-10)),  g_k = (m - y*_k) / s
    h(g) = g lambda(g) / 2 - log Phi(g),  lambda = phi / Phi = exp(-g^2 / 2 - log(2 pi) / 2 - log Phi(g))
    alpha = (1 / K) sum_k h(g_k)                       (index order, then the division)
    h'(g) = -(lambda / 2) B(g),  B = 1 + g^2 + g lambda
    c_m = d alpha / dm = ((1 / K) sum_k h'(g_k)) / s,  c_s = d alpha / ds = -((1 / K) sum_k h'(g_k) g_k) / s
    d alpha / dx = c_m y_std dmdx + c_s ds_scale dvdx,  ds_scale = y_std^2 / (2 s)
    log S(y) = sum_i log Phi((m_i - y) / s_i)           (the sampler's survival function over a table)

Nothing here imports the library or needs a GPU; everything is computed once per case and read-only.  log Phi and its evaluation
error ev(g) are tests/_feas_truth.py's (the logarithm in long double, the series below -20), with erfc in long double as well
(erfc_ld: h multiplies an error of log Phi by g^2 / 2, and SciPy's double erfc is not good enough for that).

The truth's B.  1 + g^2 + g lambda cancels for g << 0 (B -> 2 / g^2: about g^4 / 2 ulp lost).  At or below g = -12 the truth
takes it from the asymptotic series  B = (sum_{i>=1} -2 i T_i) / (1 + sum_i T_i),  T_i = (-1)^i (2i-1)!! g^-2i,  summed in long
double up to its smallest term (below e^-70 relative there), and h from the same pieces; above, from the three terms (h and B
lose at most 12^4 / 4 ... 12^4 / 2 long-double ulp there, 1e-15 -- four orders below the device's bound at that point).  The device does the same at -20 (sixteen terms, h and lambda included), the point where gp_log_ndtr switches as well.

The bound follows the device operation by operation, u = 2^-53, library functions as in _feas_truth.py (sqrt correctly rounded,
exp and log within 4 ulp = 8 u, erfc within 16 u); contraction into fma only removes roundings.  |F^(g^) - F(g)| <= |F'| dg
(the argument's own error) + the evaluation error at a fixed argument:

* m, v, s, g as _feas_truth.py has z:  dg <= |dm| / s + 4 u |g|,  |dm| <= u (|mean y_std| + |m|)
* t = log Phi(g): evaluation error ev(g) (three branches, _feas_truth.py)
* g > -20:  lambda = exp(E), E = -g^2/2 - c - t, at a fixed g:  el = ev + u (2 g^2 + 4 + |E|) + 8 u  relative
            h = A - t, A = g lambda / 2:   dh <= |h'| dg + ev + |A| (el + 2 u) + 2 u (|A| + |t|)
            (towards -20, |A| ~ |t| ~ g^2 / 2 while h ~ log|g|: h carries ~ g^2 el there, 1e-11 relative just above -20)
* g <= -20: everything from the series' pieces (mes_h, csrc/acq_math.h), nothing cancels:  lambda = -g / R: el = 8 u;
            h = W / (2 R) + log(-g) + c - log R, W = sum_i T_i g^2 = -1 + 3 t - ...: W is good to 40 u as S is, the quotient to 48 u
            on |W / 2R| <= 1/2, the two logarithms to 8 u each (R itself to 4 u), three additions:
            dh <= |h'| dg + 64 u (1/2 + log|g| + c + 0.01)
* B at a fixed g:   g > -20:  dB <= 4 u (1 + g^2 + |g| lambda) + |g| lambda el      (the cancellation: ~ g^4 / 2 relative at -20)
                    g <= -20: dB <= 64 u B   (t = 1 / g^2: 2 u; term i: 3 i u; the alternating sums are dominated by their first
                    term, sum |2 i T_i| <= 1.02 (2 t), so S is good to 40 u, R to 4 u, the quotient adds u; truncation < 1e-24)
* h' = -(lambda / 2) B:   dh' <= |h''| dg + |h'| (el + 3 u) + (lambda / 2) dB,   h'' = (lambda / 2) ((g + lambda) B - B'),
      B' = 2 g + lambda - g lambda (g + lambda)
* every per-sample bound carries the floor 1e-300: below the normal range (2.2e-308; g ~ 38: phi underflows) a double's error is
  absolute, not relative
* the sums over k in index order: (K - 1) u sum_k |.|; the division by K: u (2 u with the conversion)
      bound(alpha) = (sum_k dh_k + (K - 1) u sum_k |h_k|) / K + 2 u |alpha|
      bound(c_m)   = (sum_k dh'_k + (K - 1) u sum_k |h'_k|) / (K s) + 5 u |c_m|
      q_k = h'_k g_k:  dq_k <= dh'_k |g_k| + |h'_k| dg_k + u |q_k|
      bound(c_s)   = (sum_k dq_k + (K - 1) u sum_k |q_k|) / (K s) + 5 u |c_s|
* dm_d = dmdx y_std: u;  ds_d = dvdx ds_scale: 5 u (ds_scale: 4 u);  out_d = -(c_m dm_d + c_s ds_d):
      bound(d alpha / dx_d) = bound(c_m) |dm_d| + bound(c_s) |ds_d| + 8 u (|c_m dm_d| + |c_s ds_d|)
all times (1 + 1e-3) for the terms of second order.

log S over M rows at one trial value: the rows' t_i carry lambda_i dg_i + ev_i (m and s with every operation rounded on its own:
the same dg), and the two-level sum -- a 64-lane tree (6 levels), 3 adds over the waves, the chunks of 256 rows in order -- adds
(9 + nch - 1) u sum_i |t_i| (every t_i <= 0: no partial sum exceeds the total).
"""
import collections
import functools

import numpy as np

import _feas_truth as FT

T = FT.T
U = FT.U
HALF_LOG_2PI = FT.HALF_LOG_2PI
FLOOR = T(1e-300)    # below the normal range (2.2e-308) a double's error is absolute: every per-sample bound carries this floor
CHUNK = 256          # rows per chunk of the device's two-level sum (MES_CHUNK, csrc/gphip_internal.h)
SERIES_AT = T(-12)   # the truth's B by series at or below this
DEV_SERIES_AT = -20.0


SQRT_PI = np.sqrt(T("3.14159265358979323846264338327950288"))


def erfc_ld(x):
    """erfc(x) for x >= 0 [1-D] in long double: below 1 one minus the Maclaurin series of erf (terms below 1, erfc above 0.15:
    nothing lost), from 1 on the continued fraction  exp(-x^2) / sqrt(pi) / (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...))))
    evaluated backwards over 400 levels (truncation ~ exp(-2 x sqrt(2 N)): below e^-56 at x = 1)."""
    x = np.asarray(x, dtype=T)
    out = np.empty(x.shape, T)
    small = x < 1
    xs = x[small]
    term, acc = xs.copy(), xs.copy()
    for n in range(1, 60):
        term = -term * xs * xs / n
        acc = acc + term / (2 * n + 1)
    out[small] = 1 - 2 / SQRT_PI * acc
    xl = x[~small]
    k = xl.copy()
    for n in range(400, 0, -1):
        k = xl + (T(n) / 2) / k
    with np.errstate(under="ignore"):
        out[~small] = np.exp(-xl * xl) / SQRT_PI / k
    return out


def log_ndtr(z):
    """log Phi(z) [shape of z] in long double, whole arrays at a time (a table of 1000 rows at 64 trial values is one call):
    _feas_truth.log_ndtr's construction -- log(erfc(-z / sqrt 2) / 2), log1p of the upper tail for z > 0, its series at and below
    -20 -- with erfc itself in long double (erfc_ld).  SciPy's double erfc, which _feas_truth.py takes, carries the rounding of
    its argument times z^2: 1.5e-14 at z = -12, which h(g) = g lambda / 2 - log Phi multiplies by g^2 / 2 once more."""
    shape = np.shape(z)
    z = np.atleast_1d(np.asarray(z, dtype=T)).ravel()
    e = erfc_ld(np.abs(z) / np.sqrt(T(2)))
    # z <= 0: Phi = erfc(-z / sqrt 2) / 2;  z > 0: Phi = 1 - erfc(z / sqrt 2) / 2
    with np.errstate(divide="ignore"):      # (erfc underflows far below -20, where the series takes over)
        out = np.where(z > 0, np.log1p(-e / 2), np.log(e / 2))
    for i in np.nonzero(z <= -20)[0]:
        out[i] = FT._series(z[i])
    return out.reshape(shape)


def _bracket_series(g):
    """B(g) = 1 + g^2 + g lambda(g) for g << 0, long double: (sum_i -2 i T_i) / (1 + sum_i T_i) up to the smallest term."""
    g = T(g)
    inv = 1 / (g * g)
    term, R, S, i = T(1), T(1), T(0), 0
    while True:
        i += 1
        nxt = -term * (2 * i - 1) * inv
        if abs(nxt) >= abs(term) or i > 400:
            break
        term = nxt
        R = R + term
        S = S + (-2 * i) * term
        if abs(term) < T(1e-26):
            break
    return S / R


def bracket(g, lam=None):
    """B(g) [shape of g] in long double."""
    g = np.asarray(g, dtype=T)
    lam = mills(g) if lam is None else lam
    out = np.empty(g.shape, T)
    for i, gi in np.ndenumerate(g):
        out[i] = _bracket_series(gi) if gi <= SERIES_AT else 1 + gi * gi + gi * lam[i]
    return out


def _series_R(g):
    """R = 1 + sum_i T_i for g << 0, long double, up to the smallest term (Phi = phi / (-g) R, lambda = -g / R)."""
    g = T(g)
    inv = 1 / (g * g)
    term, R, i = T(1), T(1), 0
    while True:
        i += 1
        nxt = -term * (2 * i - 1) * inv
        if abs(nxt) >= abs(term) or i > 400:
            break
        term = nxt
        R = R + term
        if abs(term) < T(1e-26):
            break
    return R


def mills(g):
    """lambda = phi / Phi [shape of g]: exp(-g^2 / 2 - c - log Phi), whose exponent cancels two terms of size g^2 / 2; at and
    below -12 therefore -g / R from the series."""
    g = np.asarray(g, dtype=T)
    out = np.atleast_1d(np.exp(-g * g / 2 - HALF_LOG_2PI - log_ndtr(g))).copy()
    gf = np.atleast_1d(g)
    for i in zip(*np.nonzero(gf <= SERIES_AT)):
        out[i] = -gf[i] / _series_R(gf[i])
    return out.reshape(np.shape(g))


def h(g):
    """h(g) = g lambda / 2 - log Phi(g).  For g <= -12 from the series' pieces (no cancellation): with R = 1 + sum T_i,
    h = (g^2 / 2) (1 - 1 / R) + log(-g) + log(2 pi) / 2 - log R  and  g^2 (1 - 1/R) = g^2 (R - 1) / R = (sum_i T_i g^2) / R."""
    g = np.asarray(g, dtype=T)
    out = np.empty(g.shape, T)
    lam = mills(g)
    t = log_ndtr(g)
    for i, gi in np.ndenumerate(g):
        if gi <= SERIES_AT:
            inv = 1 / (gi * gi)
            term, R, W, k = T(1), T(1), T(0), 0      # W = sum_i T_i g^2
            while True:
                k += 1
                nxt = -term * (2 * k - 1) * inv
                if abs(nxt) >= abs(term) or k > 400:
                    break
                W = W + nxt * gi * gi
                term = nxt
                R = R + term
                if abs(term) < T(1e-26):
                    break
            out[i] = W / (2 * R) + np.log(-gi) + HALF_LOG_2PI - np.log(R)
        else:
            out[i] = gi * lam[i] / 2 - t[i]
    return out


def hprime(g):
    g = np.asarray(g, dtype=T)
    lam = mills(g)
    return -(lam / 2) * bracket(g, lam)


def hsecond(g):
    """h''(g) (enters the bounds only)."""
    g = np.asarray(g, dtype=T)
    lam = mills(g)
    B = bracket(g, lam)
    Bp = 2 * g + lam - g * lam * (g + lam)
    return (lam / 2) * ((g + lam) * B - Bp)


def _ev(g, t, lam):
    """The evaluation error of the device's log Phi at a fixed argument (_feas_truth.py, three branches)."""
    az, at = np.abs(g), np.abs(t)
    return np.where(g > 6, at * (4 * g * g + 32) * U + t * t,
                    np.where(g > -20, 16 * U + 2 * U * lam * az + 8 * U * at, U * (2 * g * g + 3 * at + 32)))


def _row(mean, var, y_mean, y_std):
    mn, vr = np.asarray(mean, dtype=np.float64).astype(T), np.asarray(var, dtype=np.float64).astype(T)
    ym, ys = T(np.float64(y_mean)), T(np.float64(y_std))
    m = mn * ys + ym
    s = np.sqrt(np.maximum(vr * ys * ys, T(1e-10)))
    d_m = U * (np.abs(mn * ys) + np.abs(m))
    return m, s, d_m, ys


Score = collections.namedtuple("Score", "alpha dalpha bound_alpha bound_dalpha g lam s hp hpp c_m c_s dm ds")


def score(mean, var, dmdx, dvdx, ystar, y_mean, y_std):
    """MES at M locations over the K samples ``ystar``.  mean, var [M]; dmdx, dvdx [M, D] or None.  Returns Score: alpha [M],
    d alpha / dx [M, D] (None without gradients), their rounding-error bounds on the device, and the pieces ([K, M]: g, lambda, h',
    h''; [M]: s, c_m, c_s; [M, D]: dm, ds) the propagation reads.  The entries return -alpha and -d alpha / dx."""
    m, s, d_m, ys = _row(mean, var, y_mean, y_std)
    y = np.asarray(ystar, dtype=np.float64).astype(T).reshape(-1, 1)
    K = y.shape[0]
    g = (m[None, :] - y) / s[None, :]
    t = log_ndtr(g)
    lam = mills(g)
    B = bracket(g, lam)
    hv = h(g)
    hp = -(lam / 2) * B
    Bp = 2 * g + lam - g * lam * (g + lam)
    hpp = (lam / 2) * ((g + lam) * B - Bp)

    def seq(a):
        acc = a[0].copy()
        for k in range(1, K):
            acc = acc + a[k]
        return acc

    alpha = seq(hv) / K
    c_m = (seq(hp) / K) / s
    c_s = -((seq(hp * g) / K) / s)
    # ---- the device's rounding
    dg = d_m[None, :] / s[None, :] + 4 * U * np.abs(g)
    ev = _ev(g, t, lam)
    E = -g * g / 2 - HALF_LOG_2PI - t
    far = g <= DEV_SERIES_AT
    el = np.where(far, 8 * U, ev + U * (2 * g * g + 4 + np.abs(E)) + 8 * U)
    A = g * lam / 2
    with np.errstate(invalid="ignore", divide="ignore"):
        dh_far = np.abs(hp) * dg + 64 * U * (T(0.5) + np.abs(np.log(np.where(far, -g, T(1)))) + HALF_LOG_2PI + T(0.01))
    dh = np.where(far, dh_far, np.abs(hp) * dg + ev + np.abs(A) * (el + 2 * U) + 2 * U * (np.abs(A) + np.abs(t))) + FLOOR
    dB = np.where(~far, 4 * U * (1 + g * g + np.abs(g) * lam) + np.abs(g) * lam * el, 64 * U * np.abs(B))
    dhp = np.abs(hpp) * dg + np.abs(hp) * (el + 3 * U) + (lam / 2) * dB + FLOOR
    q = hp * g
    dq = dhp * np.abs(g) + np.abs(hp) * dg + U * np.abs(q) + FLOOR
    one = 1 + T(1e-3)
    b_alpha = ((dh.sum(0) + (K - 1) * U * np.abs(hv).sum(0)) / K + 2 * U * np.abs(alpha)) * one
    b_cm = (dhp.sum(0) + (K - 1) * U * np.abs(hp).sum(0)) / (K * s) + 5 * U * np.abs(c_m)
    b_cs = (dq.sum(0) + (K - 1) * U * np.abs(q).sum(0)) / (K * s) + 5 * U * np.abs(c_s)
    dalpha = b_d = dm = ds = None
    if dmdx is not None:
        dm = ys * np.asarray(dmdx, dtype=np.float64).astype(T)
        ds = (ys * ys) * np.asarray(dvdx, dtype=np.float64).astype(T) / (2 * s[:, None])
        pm, ps = c_m[:, None] * dm, c_s[:, None] * ds
        dalpha = pm + ps
        b_d = (b_cm[:, None] * np.abs(dm) + b_cs[:, None] * np.abs(ds) + 8 * U * (np.abs(pm) + np.abs(ps))) * one
    return Score(alpha, dalpha, b_alpha, b_d, g, lam, s, hp, hpp, c_m, c_s, dm, ds)


def propagate(f, y_std, d_mean, d_sd, d_dm=None, d_dv=None):
    """What a posterior that is off by d_mean, d_sd [M] (normalised mean and standard deviation) and d_dm, d_dv [M, D] (their
    x-gradients; dv the variance's) moves alpha and its gradient by, to first order, around the Score ``f``:
        dg_k = (|dm| + |g_k| |ds|) / s,   |d alpha| <= (1 / K) sum_k |h'_k| dg_k
        |d c_m| <= (1 / K) sum_k |h''_k| dg_k / s + |c_m| ds / s
        |d c_s| <= (1 / K) sum_k |h''_k g_k + h'_k| dg_k / s + |c_s| ds / s
        |d grad| <= |d c_m| |dm_x| + |c_m| |d dm_x| + |d c_s| |ds_x| + |c_s| |d ds_x|,
    dm_x = y_std dmdx, ds_x = y_std^2 dvdx / (2 s),  |d ds_x| <= y_std^2 |d dvdx| / (2 s) + |ds_x| ds / s."""
    ys = T(np.float64(y_std))
    K = f.g.shape[0]
    dm_, ds_ = ys * np.asarray(d_mean, dtype=T), ys * np.asarray(d_sd, dtype=T)
    dg = (dm_[None, :] + np.abs(f.g) * ds_[None, :]) / f.s[None, :]
    tol_a = (np.abs(f.hp) * dg).sum(0) / K
    tol_d = None
    if d_dm is not None:
        rel = ds_ / f.s
        dcm = (np.abs(f.hpp) * dg).sum(0) / (K * f.s) + np.abs(f.c_m) * rel
        dcs = (np.abs(f.hpp * f.g + f.hp) * dg).sum(0) / (K * f.s) + np.abs(f.c_s) * rel
        e_dm = ys * np.asarray(d_dm, dtype=T)
        e_ds = (ys * ys) * np.asarray(d_dv, dtype=T) / (2 * f.s[:, None]) + np.abs(f.ds) * rel[:, None]
        tol_d = (dcm[:, None] * np.abs(f.dm) + np.abs(f.c_m)[:, None] * e_dm + dcs[:, None] * np.abs(f.ds)
                 + np.abs(f.c_s)[:, None] * e_ds)
    return tol_a, tol_d


# ---- the sampler's sums ------------------------------------------------------------------------------------------------------------
LogS = collections.namedtuple("LogS", "value bound slope")


def logsurv(mean, var, y_mean, y_std, y):
    """log S at the trial values y [G] over the table (mean, var [M]): value [G], the device's rounding-error bound [G], and
    d log S / dy = -sum_i lambda_i / s_i [G]."""
    m, s, d_m, _ = _row(mean, var, y_mean, y_std)
    y = np.asarray(y, dtype=np.float64).astype(T).reshape(-1, 1)
    g = (m[None, :] - y) / s[None, :]
    t = log_ndtr(g)
    lam = mills(g)
    dg = d_m[None, :] / s[None, :] + 4 * U * np.abs(g)
    nch = (m.size + CHUNK - 1) // CHUNK
    bound = ((lam * dg + _ev(g, t, lam)).sum(1) + (9 + nch - 1) * U * np.abs(t).sum(1)) * (1 + T(1e-3))
    return LogS(t.sum(1), bound, -(lam / s[None, :]).sum(1))


def propagate_logsurv(mean, var, y_mean, y_std, y, d_mean, d_sd):
    """First-order move of log S under a posterior off by d_mean, d_sd [M] (normalised): sum_i lambda_i (|dm| + |g_i| |ds|) / s_i."""
    m, s, _, ys = _row(mean, var, y_mean, y_std)
    y = np.asarray(y, dtype=np.float64).astype(T).reshape(-1, 1)
    g = (m[None, :] - y) / s[None, :]
    lam = mills(g)
    return (lam * (ys * np.asarray(d_mean, dtype=T)[None, :] + np.abs(g) * ys * np.asarray(d_sd, dtype=T)[None, :]) / s[None, :]).sum(1)


QUANTILES = (0.25, 0.5, 0.75)
LOGLOG = {0.25: np.log(np.log(4.0 / 3.0)), 0.5: np.log(np.log(2.0)), 0.75: np.log(np.log(4.0))}


def quantile(mean, var, y_mean, y_std, q, nsig=8.0):
    """y with 1 - S(y) = q, by long-double bisection on the truth's log S inside [min(m - nsig s), min(m + nsig s)]."""
    m, s, _, _ = _row(mean, var, y_mean, y_std)
    lo, hi = (m - T(nsig) * s).min(), (m + T(nsig) * s).min()
    target = np.log1p(-T(q))
    for _ in range(70):
        mid = (lo + hi) / 2
        g = (m - mid) / s
        if log_ndtr(g).sum() >= target:      # S still at least 1 - q: the quantile lies above
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def gumbel_fit(y25, y50, y75):
    """(a, b) of the minimum's Gumbel law  Pr[y* <= y] = 1 - exp(-exp((y - a) / b))  through the three quartiles."""
    b = (y75 - y25) / (LOGLOG[0.75] - LOGLOG[0.25])
    return y50 - b * LOGLOG[0.5], b


def gumbel_samples(a, b, K, seed, fmin):
    """K draws a + b log(-log U_k), U from numpy.random.RandomState(seed), clipped at fmin."""
    u = np.random.RandomState(seed).uniform(size=K)
    return np.minimum(a + b * np.log(-np.log(u)), fmin)


# ---- the case table -------------------------------------------------------------------------------------------------------------
# D 2, 3; N 40, 200; Matern-5/2 and Exponential; ARD on and off; K 1, 10, 64.  Rows: nine locations (fused narrow 1, 3, 4, wide 5,
# 8, the fallback 9 are its heads).  Targets: sample k puts g at location k mod 9 on the target -- the series branch (-25), the
# cancelling bracket (-5), 0, 3, 8, and 40 where h underflows towards 0 and must stay finite, with a finite gradient.
Case = collections.namedtuple("Case", "id fam ard D N K")
TABLE = (
    Case("a", "Mat52", True, 2, 40, 1),
    Case("b", "Mat52", False, 3, 200, 10),
    Case("c", "Exponential", True, 3, 40, 64),
    Case("d", "Exponential", False, 2, 200, 10),
    Case("e", "Mat52", True, 3, 200, 64),
    Case("f", "Exponential", True, 2, 40, 1),
)
CASES = {c.id: c for c in TABLE}
G_TARGETS = (-25.0, -5.0, 0.0, 3.0, 8.0, 40.0)
M_ROWS = 9
M_TABLE = 1000
Y_MEAN, Y_STD = 0.3, 1.7      # the output normaliser of every scoring call
NOISE = 1e-2
Problem = collections.namedtuple("Problem", "case X Y variance ls ls_arg Xs Xtab")


def _response(X):
    D = X.shape[1]
    w = np.cos(0.7 * np.arange(1, D + 1))
    return np.sin(3.0 * X @ w / np.sqrt(D)) + ((X - 0.4) ** 2).sum(1) / D


@functools.lru_cache(maxsize=None)
def problem(cid):
    """The data of a case: (X, Y) standardised, kernel parameters, the rows' locations Xs [9, D] and the table Xtab [1000, D]
    (whose head is Xs)."""
    c = CASES[cid]
    rng = np.random.default_rng(3000 + ord(cid))
    X = rng.uniform(0, 1, (c.N, c.D))
    Y = (_response(X) + 0.05 * rng.standard_normal(c.N))[:, None]
    Y = (Y - Y.mean()) / Y.std()
    base = 0.5 * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.7, 1.4, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    Xtab = rng.uniform(0, 1, (M_TABLE, c.D))
    Xs = Xtab[:M_ROWS].copy()
    for a in (X, Y, ls_arg, ls, Xs, Xtab):
        a.setflags(write=False)
    return Problem(c, X, Y, 1.3, ls, ls_arg, Xs, Xtab)


def ystar_for(cid, target, m, sd):
    """K samples that put g of sample k on ``target`` at location k mod M, given the un-normalised posterior mean and standard
    deviation [M] of the locations (placement only)."""
    c = CASES[cid]
    M = m.shape[0]
    idx = np.arange(c.K) % M
    return np.asarray(m, dtype=np.float64)[idx] - target * np.asarray(sd, dtype=np.float64)[idx]
