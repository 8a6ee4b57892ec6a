"""The probability of feasibility of K black-box constraints in ``np.longdouble`` (x87 80-bit, eps 1.1e-19), the rounding-error
bound of the device's evaluation of it (``feas_terms`` / ``feas_grad``, csrc/acq_math.h; the fold of csrc/feas.hip), the
propagation of a posterior tolerance through it, and the case table of tests/test_gpu_feas.py and tests/test_feas_truth_host.py.

    log F(x) = sum_k log Phi(z_k),   z_k = (b_k - m_k) / s_k,   m_k = mean_k c_std_k + c_mean_k,
    s_k = sqrt(max(var_k c_std_k^2, 1e-10)),   d log F / dx = sum_k lambda(z_k) (-dm_k - z_k ds_k) / s_k,
    dm_k = c_std_k dmdx_k,   ds_k = c_std_k^2 dvdx_k / (2 s_k),   lambda = phi / Phi = exp(-z^2 / 2 - log(2 pi) / 2 - log Phi(z))

Nothing here imports the library or needs a GPU; everything is computed once per case and read-only.

The special function: erfc comes from scipy in double (as tests/_es_truth.py takes it) at zd = float(z), the logarithm -- log1p
of the upper tail for z > 0 -- is taken in long double, and the first-order term lambda(zd) (z - zd) carries the value from zd to
z; below z = -20 the asymptotic series  -z^2/2 - log(-z) - log(2 pi)/2 + log sum_i (-1)^i (2i-1)!! z^-2i  runs in long double up
to its smallest term (< e^-200 relative).

The bound follows the device operation by operation, u = 2^-53.  Library functions are taken at: sqrt correctly rounded, exp within
4 ulp = 8 u (DESIGN.md quotes it), log within 4 ulp, erfc within 8 ulp = 16 u (twice the 5 ulp vendors' tables list for it).
Contraction into fma only removes roundings.

* m: |dm| <= u (|mean c_std| + |m|);  v = var (c_std c_std): 2 u relative, s = sqrt(v): 2 u relative (the clip is exact);
  z = (b - m) / s:   dz <= (|dm| + u |b - m|) / s + 3 u |z|  <=  |dm| / s + 4 u |z|
* t = log Phi(z) moves by lambda(z) dz with its argument, and its evaluation adds ev(z):
    z > 6       t = -erfc(z / sqrt 2) / 2:  |t| (4 z^2 + 32) u for erfc and its argument, t^2 for log(1 - p) = -p - p^2/2 - ...
    -20 < z<=6  t = log(erfc(-z / sqrt 2) / 2):  16 u (erfc, and the rounding of Phi itself near 1) + 2 u lambda |z| (the argument's
                two roundings) + 8 u |t| (log)
    z <= -20    the series:  u (2 z^2 + 3 |t| + 32)  (z^2 / 2, the two logarithms, the three subtractions, <= 2 u truncation)
* the sum over k in index order: (K - 1) u sum_k |t_k|
      bound(log F) = sum_k (lambda_k dz_k + ev_k) + (K - 1) u sum_k |t_k|
* lambda = exp(E), E = -z^2/2 - c - t:  d lambda / lambda <= |z + lambda| dz + ev + u (2 z^2 + 4 + |E|) + 8 u
  (d/dz (-z^2/2 - log Phi) = -(z + lambda))
* dm = c_std dmdx: u;  ds = (c_std c_std) dvdx / (2 s): 5 u;  num = -dm - z ds with A = |dm| + |z ds|:
      |d num| <= |ds| dz + 8 u A
* g = lambda num / s:  |dg| <= |g| (d lambda / lambda + 4 u) + lambda / s |d num|;  the sum over k: (K - 1) u sum_k |g_k|
both times (1 + 1e-3) for the terms of second order.
"""
import collections
import functools

import numpy as np
from scipy.special import erfc

T = np.longdouble
U = T(2.0) ** -53
SQ2 = np.sqrt(T(2))
HALF_LOG_2PI = T("0.918938533204672741780329736405617639861")


def _series(z):
    """log Phi(z) for z <= -20, long double: the asymptotic series up to its smallest term."""
    z = T(z)
    rhs, term, i = T(1), T(1), 0
    inv = 1 / (z * z)
    while True:
        i += 1
        nxt = -term * (2 * i - 1) * inv
        if abs(nxt) >= abs(term) or i > 400:
            break
        term = nxt
        rhs = rhs + term
        if abs(term) < T(1e-25):
            break
    return -z * z / 2 - np.log(-z) - HALF_LOG_2PI + np.log(rhs)


def _log_ndtr_at_double(zd):
    """log Phi at a double argument: erfc in double, the logarithm in long double."""
    if zd > 0:
        return np.log1p(-T(0.5) * T(erfc(zd / float(np.sqrt(2.0)))))
    return np.log(T(0.5) * T(erfc(-zd / float(np.sqrt(2.0)))))


def log_ndtr(z):
    """log Phi(z) [shape of z] in long double."""
    z = np.asarray(z, dtype=T)
    out = np.empty(z.shape, T)
    for i, zi in np.ndenumerate(z):
        if zi <= -20:
            out[i] = _series(zi)
        else:
            zd = float(zi)
            t = _log_ndtr_at_double(zd)
            lam = np.exp(-T(zd) * T(zd) / 2 - HALF_LOG_2PI - t)
            out[i] = t + lam * (zi - T(zd))
    return out


def mills(z):
    """lambda(z) = phi(z) / Phi(z) in long double."""
    z = np.asarray(z, dtype=T)
    return np.exp(-z * z / 2 - HALF_LOG_2PI - log_ndtr(z))


Fold = collections.namedtuple("Fold", "logF dlogF bound_logF bound_dlogF z lam s terms")


def fold(mean, var, dmdx, dvdx, c_mean, c_std, bound):
    """The fold over K constraints at M locations.  mean, var [K, M]; dmdx, dvdx [K, M, D] or None; c_mean, c_std, bound [K].
    Returns Fold: logF [M], dlogF [M, D] (None without gradients), their rounding-error bounds on the device, and z, lambda, s,
    log Phi per constraint [K, M]."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    K, M = mean.shape
    cm, cs, b = (np.asarray(a, dtype=np.float64).astype(T).reshape(K, 1) for a in (c_mean, c_std, bound))
    mn, vr = mean.astype(T), var.astype(T)
    m = mn * cs + cm
    v = np.maximum(vr * cs * cs, T(1e-10))
    s = np.sqrt(v)
    z = (b - m) / s
    t = log_ndtr(z)
    lam = np.exp(-z * z / 2 - HALF_LOG_2PI - t)
    logF = t[0].copy()
    for k in range(1, K):
        logF = logF + t[k]
    d_m = U * (np.abs(mn * cs) + np.abs(m))
    dz = d_m / s + 4 * U * np.abs(z)
    az, at = np.abs(z), np.abs(t)
    ev = np.where(z > 6, at * (4 * z * z + 32) * U + t * t,
                  np.where(z > -20, 16 * U + 2 * U * lam * az + 8 * U * at, U * (2 * z * z + 3 * at + 32)))
    b_log = ((lam * dz + ev).sum(0) + (K - 1) * U * at.sum(0)) * (1 + T(1e-3))
    dlogF = b_d = None
    if dmdx is not None:
        dm = cs[:, :, None] * np.asarray(dmdx, dtype=np.float64).astype(T)
        ds = (cs * cs)[:, :, None] * np.asarray(dvdx, dtype=np.float64).astype(T) / (2 * s[:, :, None])
        num = -dm - z[:, :, None] * ds
        g = lam[:, :, None] * num / s[:, :, None]
        dlogF = g[0].copy()
        for k in range(1, K):
            dlogF = dlogF + g[k]
        E = -z * z / 2 - HALF_LOG_2PI - t
        dlam = np.abs(z + lam) * dz + ev + U * (2 * z * z + 4 + np.abs(E)) + 8 * U
        A = np.abs(dm) + np.abs(z[:, :, None] * ds)
        dnum = np.abs(ds) * dz[:, :, None] + 8 * U * A
        dg = np.abs(g) * (dlam + 4 * U)[:, :, None] + (lam / s)[:, :, None] * dnum
        b_d = (dg.sum(0) + (K - 1) * U * np.abs(g).sum(0)) * (1 + T(1e-3))
    return Fold(logF, dlogF, b_log, b_d, z, lam, s, t)


def propagate(f, c_std, d_mean, d_sd, d_dm=None, d_dv=None, dmdx=None, dvdx=None):
    """What a posterior that is off by d_mean, d_sd [K, M] (normalised mean and standard deviation) and d_dm, d_dv [K, M, D]
    (their x-gradients; dv the variance's) moves log F and its gradient by, to first order, around the Fold ``f``:
        |d t_k| <= lambda (|dm| + |z| |ds|) / s                      (the issue's form; dm, ds un-normalised)
        |d g_k| <= (|lambda'| |num| / s + lambda |ds_x| / s) dz + |g| ds / s + lambda / s (|d dm| + |z| |d ds_x|),
    lambda' = -lambda (z + lambda), dz = (|dm| + |z| |ds|) / s, ds_x = c_std^2 dvdx / (2 s)."""
    K = f.z.shape[0]
    cs = np.asarray(c_std, dtype=np.float64).astype(T).reshape(K, 1)
    dm_, ds_ = cs * np.asarray(d_mean, dtype=T), cs * np.asarray(d_sd, dtype=T)
    dz = (dm_ + np.abs(f.z) * ds_) / f.s
    tol_log = (f.lam * dz).sum(0)
    tol_d = None
    if d_dm is not None:
        gm = cs[:, :, None] * np.asarray(dmdx, dtype=np.float64).astype(T)
        gs = (cs * cs)[:, :, None] * np.asarray(dvdx, dtype=np.float64).astype(T) / (2 * f.s[:, :, None])
        num = -gm - f.z[:, :, None] * gs
        g = f.lam[:, :, None] * num / f.s[:, :, None]
        lamp = f.lam * np.abs(f.z + f.lam)
        e_gm = cs[:, :, None] * np.asarray(d_dm, dtype=T)
        e_gs = (cs * cs)[:, :, None] * np.asarray(d_dv, dtype=T) / (2 * f.s[:, :, None]) + np.abs(gs) * (ds_ / f.s)[:, :, None]
        tol_d = ((lamp / f.s)[:, :, None] * np.abs(num) * dz[:, :, None] + (f.lam / f.s)[:, :, None] * np.abs(gs) * dz[:, :, None]
                 + np.abs(g) * (ds_ / f.s)[:, :, None] + (f.lam / f.s)[:, :, None] * (e_gm + np.abs(f.z)[:, :, None] * e_gs)).sum(0)
    return tol_log, tol_d


# ---- the case table -------------------------------------------------------------------------------------------------------------
# Scored model N = 200; constraint handles of Nc in {33, 200, 300} (one tile with a ragged edge, the scored model's size, three
# tiles); D 1, 6, 20 (D = 20: eight locations are 160 > ROWS_MAX_XS = 128 doubles, a group splits into passes of four); K 1, 3, 8;
# rows M 1, 3, 4, 5, 8, 20 (layouts MV = 1 / 4 / 8, a second and a third group); tables M 1, 9, 257 (257 with mc_max = 128: three
# chunks); Matern-5/2 ARD and Exponential.  `clip`: constraint 0 has noise 1e-12 and location 0 sits on one of its training points.
Case = collections.namedtuple("Case", "id fam ard D K Nc M Mtab clip")
NCS = (33, 200, 300)
TABLE = (
    Case("a", "Mat52", True, 1, 1, (200,), 1, 1, False),
    Case("b", "Mat52", True, 6, 3, (33, 200, 300), 5, 9, True),
    Case("c", "Exponential", False, 20, 8, NCS * 2 + (33, 200), 20, 257, False),
    Case("d", "Exponential", False, 6, 1, (300,), 3, 9, False),
    Case("e", "Mat52", True, 6, 3, (300, 33, 200), 4, 257, True),
    Case("f", "Mat52", True, 1, 8, NCS * 2 + (300, 33), 8, 9, False),
)
CASES = {c.id: c for c in TABLE}
Z_TARGETS = (0.0, -10.0, -25.0, -45.0, 8.0)
N_SCORED = 200
Problem = collections.namedtuple("Problem", "case X Y Xc C variance ls ls_arg noise c_mean c_std Xs Xtab")


def _response(X, k):
    """A smooth constraint over the unit box, different for every k."""
    D = X.shape[1]
    w = np.cos(0.7 * (k + 1) * np.arange(1, D + 1))
    return np.sin(2.0 * X @ w / np.sqrt(D) + 0.3 * k) + 0.5 * ((X - 0.5) ** 2).sum(1) / D - 0.2


@functools.lru_cache(maxsize=None)
def problem(cid):
    """The data of a case: the scored model's (X, Y), K constraint data sets (Xc_k, C_k) with their standardisation, kernel
    parameters shared by the handles, the rows' locations Xs and the table Xtab (whose head is Xs)."""
    c = CASES[cid]
    rng = np.random.default_rng(2000 + ord(cid))
    X = rng.uniform(0, 1, (N_SCORED, c.D))
    Y = (_response(X, 11) + 0.05 * rng.standard_normal(N_SCORED))[:, None]
    Y = (Y - Y.mean()) / Y.std()
    Xc, C, cmean, cstd, noise = [], [], [], [], []
    for k in range(c.K):
        xk = rng.uniform(0, 1, (c.Nc[k], c.D))
        # (the clipped constraint is a small one: its variance on a training point, ~1e-8 c_std^2, lies below the clip at 1e-10)
        ck = _response(xk, k) * (0.1 if (c.clip and k == 0) else 1.0 + 0.5 * k) + 0.3 * k
        cmean.append(ck.mean())
        cstd.append(ck.std())
        Xc.append(xk)
        C.append(((ck - ck.mean()) / ck.std())[:, None])
        noise.append(1e-12 if (c.clip and k == 0) else 1e-3 * (1 + k))
    base = 0.5 * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.7, 1.4, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    Xtab = rng.uniform(0, 1, (max(c.Mtab, c.M), c.D))
    if c.clip:
        Xtab[0] = Xc[0][7]
    Xs = Xtab[:c.M].copy()
    Xtab = Xtab[:c.Mtab].copy()
    for a in [X, Y, ls_arg, ls, Xs, Xtab] + Xc + C:
        a.setflags(write=False)
    return Problem(c, X, Y, tuple(Xc), tuple(C), 1.3, ls, ls_arg, tuple(noise), np.array(cmean), np.array(cstd), Xs, Xtab)


def bounds_for(cid, target, mean, sd):
    """Upper bounds b [K] that put z of constraint k near ``target`` at location k mod M, given the constraints' un-normalised
    posterior mean and standard deviation [K, M] (from the CPU oracle: placement only)."""
    c = CASES[cid]
    M = mean.shape[1]
    return np.array([mean[k, k % M] + target * sd[k, k % M] for k in range(c.K)])
