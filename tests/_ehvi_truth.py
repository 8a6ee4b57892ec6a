"""Expected hypervolume improvement of K independent objective GPs in ``np.longdouble`` (x87 80-bit, eps 1.1e-19), the
rounding-error bound of the device's evaluation of it (``ehvi_level``, csrc/acq_math.h; ``ehvi_location``, csrc/ehvi.hip), the
propagation of a posterior tolerance through it, and the case table of tests/test_gpu_ehvi.py and tests/test_ehvi_truth_host.py.

    EHVI = sum_c prod_k D_ck,  D_ck = Psi_k(u_ck) - Psi_k(l_ck),  Psi_k(c) = s_k (z Phi(z) + phi(z)),  z = (c - m_k) / s_k,
    m_k = mean_k y_std_k + y_mean_k,  s_k = sqrt(max(var_k y_std_k^2, 1e-10)),  Psi_k(-inf) = Phi_k(-inf) = phi_k(-inf) = 0,
    G_mk = sum_c (prod_{j != k} D_cj) (Phi_k(l_ck) - Phi_k(u_ck)),  G_sk = sum_c (prod_{j != k} D_cj) (phi_k(u_ck) - phi_k(l_ck)),
    d EHVI / dx_d = sum_k G_mk y_std_k dmdx_k[d] + G_sk y_std_k^2 dvdx_k[d] / (2 s_k)

Nothing here imports the library or needs a GPU; everything is computed once per case and read-only.

The special function: tests/_feas_truth.py takes erfc from scipy in double and carries it to the long-double argument by a
first-order term, which is enough behind a logarithm.  Here Phi enters differences of neighbouring levels directly, so erfc itself
is evaluated in long double (``erfc``): for |x| < 1 as 1 - erf from the all-positive series
erf(x) = 2 / sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (2n+1)!!, from 1 on by the continued fraction
erfc(x) = exp(-x^2) / sqrt(pi) / (x + (1/2) / (x + (2/2) / (x + (3/2) / (x + ...)))) evaluated backwards over 1200 terms; both to a
few long-double eps (checked against 40-digit values when this was written: below 7e-19 relative on [-40, 40]).

The bound follows the device operation by operation, u = 2^-53, with the conventions of tests/_feas_truth.py: sqrt and division
correctly rounded, exp within 4 ulp = 8 u, erfc within 8 ulp = 16 u; no product is contracted into an fma on the device
(``#pragma clang fp contract(off)``), and a contraction would only remove a rounding.

* per objective: |dm| <= u (|mean y_std| + |m|);  v = var (y_std y_std): 2 u relative, s = sqrt(v): 2 u relative (the clip is exact)
* per level:  z = (c - m) / s:  dz <= |dm| / s + 4 u |z|
    phi = exp((-0.5 z) z) / sqrt(2 pi):  d phi <= phi (|z| dz + u z^2 / 2 + 8 u + 2 u)
    Phi = 0.5 erfc(-z / sqrt 2):         d Phi <= phi (dz + 2 u |z|) + 16 u Phi            (d Phi / dz = phi)
    Psi = s (z Phi + phi):  d(z Phi) <= |z| d Phi + Phi dz + u |z Phi|,  d(sum) <= d(z Phi) + d phi + u |z Phi + phi|,
                            d Psi <= s d(sum) + 3 u |Psi|
* per cell:  D_k = Psi(u) - Psi(l):  dD_k = d Psi(u) + d Psi(l) + u |D_k|;  the product of K factors:
    sum_k dD_k prod_{j != k} |D_j| + (K - 1) u |prod|
* the sum over the cells: thread t adds its ceil(C / 256) cells in order, then six levels of the wave's tree and three additions
  over the waves -- every term passes through at most n_t + 9 additions: (n_t + 9) u sum_c |term_c|
* the partials: the same with one factor replaced by Phi(l) - Phi(u) (error d Phi(l) + d Phi(u) + u |.|) or phi(u) - phi(l)
* the gradient:  A = (G_m y_std) dmdx: |y_std dmdx| dG_m + 2 u |A|;  B = ((G_s (y_std y_std)) dvdx) / (2 s):
    |y_std^2 dvdx / (2 s)| dG_s + 6 u |B|;  A + B: u (|A| + |B|);  the sum over k: (K - 1) u sum_k (|A_k| + |B_k|)
* gradual underflow (the truth's long double reaches 1e-4900, the device's double 5e-324): exp and erfc results below the normal
  range are taken as accurate to the smallest normal number TINY = 2^-1022, and every other operation whose result falls there
  carries up to ETA = 2^-1074, the spacing of the subnormals -- TINY enters d phi and d Phi and travels with them, ETA is added
  once per operation of a cell, of the sums and of the gradient's terms.  Far beyond the front, where a factor is e^-1800, this
  is the whole bound.
everything times (1 + 1e-3) for the terms of second order.  The bound is absolute: deep inside the dominated region, where EHVI
underflows against the levels' Psi, it exceeds the value, as EI's bound does there.
"""
import collections
import functools

import numpy as np

T = np.longdouble
U = T(2.0) ** -53
SQ2 = np.sqrt(T(2))
SQPI = np.sqrt(T("3.14159265358979323846264338327950288419716939937510"))
SQ2PI = SQ2 * SQPI
TINY, ETA = T(2.0) ** -1022, T(2.0) ** -1074
THREADS = 256          # EHVI_THREADS of csrc/gphip_internal.h
MAX_LEVELS, MAX_CELLS = 256, 32768


def erfc(x):
    """erfc [shape of x] in long double."""
    x = np.asarray(x, dtype=T)
    a = np.abs(x)
    small = a < 1
    xs = np.where(small, a, T(0))
    term = xs.copy()
    total = xs.copy()
    for n in range(80):
        term = term * (2 * xs * xs) / (2 * n + 3)
        total = total + term
    lo = 1 - 2 / SQPI * np.exp(-xs * xs) * total
    xl = np.where(small, T(1), a)
    f = xl.copy()
    for n in range(1200, 0, -1):
        f = xl + (T(n) / 2) / f
    with np.errstate(under="ignore"):
        hi = np.exp(-xl * xl) / (SQPI * f)
    pos = np.where(small, lo, hi)
    return np.where(x < 0, 2 - pos, pos)


def ndtr(z):
    return erfc(-np.asarray(z, dtype=T) / SQ2) / 2


def npdf(z):
    z = np.asarray(z, dtype=T)
    with np.errstate(under="ignore"):
        return np.exp(-z * z / 2) / SQ2PI


Levels = collections.namedtuple("Levels", "m s z Psi Phi phi dPsi dPhi dphi")
Truth = collections.namedtuple("Truth", "value grad Gm Gs bound_value bound_grad bound_Gm bound_Gs m s lev D")


def level_tables(mean, var, y_mean, y_std, levels, bound=True):
    """Per objective k the tables over its levels [L_k, M] in long double -- z, Psi, Phi, phi with zeros at index 0 (-inf) -- and
    the device's rounding-error bounds of the three; m, s [K, M]."""
    mean, var = np.asarray(mean, dtype=np.float64).astype(T), np.asarray(var, dtype=np.float64).astype(T)
    K, M = mean.shape
    out = []
    for k in range(K):
        ys, ym = T(np.float64(y_std[k])), T(np.float64(y_mean[k]))
        m = mean[k] * ys + ym
        s = np.sqrt(np.maximum(var[k] * ys * ys, T(1e-10)))
        c = np.asarray(levels[k], dtype=np.float64).astype(T)[1:, None]
        z = (c - m[None, :]) / s[None, :]
        phi, Phi = npdf(z), ndtr(z)
        zP = z * Phi
        Psi = s[None, :] * (zP + phi)
        dPsi = dPhi = dphi = None
        if bound:
            d_m = U * (np.abs(mean[k] * ys) + np.abs(m))
            az = np.abs(z)
            dz = d_m[None, :] / s[None, :] + 4 * U * az
            dphi = phi * (az * dz + U * z * z / 2 + 10 * U) + TINY
            dPhi = phi * (dz + 2 * U * az) + 16 * U * Phi + TINY
            dzP = az * dPhi + Phi * dz + U * np.abs(zP) + ETA
            dsum = dzP + dphi + U * np.abs(zP + phi)
            dPsi = s[None, :] * dsum + 3 * U * np.abs(Psi) + ETA
        zero = np.zeros((1, M), T)
        pad = lambda a: None if a is None else np.vstack((zero, a))
        out.append(Levels(m, s, pad(z), pad(Psi), pad(Phi), pad(phi), pad(dPsi), pad(dPhi), pad(dphi)))
    return out


def _prod_others(D, k):
    """(prod_{j != k} D_j, the indices j)."""
    js = [j for j in range(len(D)) if j != k]
    if len(js) == 1:
        return D[js[0]], js
    return D[js[0]] * D[js[1]], js


def ehvi(mean, var, dmdx, dvdx, y_mean, y_std, levels, cell_lo, cell_hi, bound=True):
    """EHVI at M locations: mean, var [K, M] (normalised posterior, noise included); dmdx, dvdx [K, M, D] or None; y_mean, y_std
    [K]; levels a list of K arrays (entry 0 stands for -inf); cell_lo, cell_hi [C, K].  Returns Truth: value [M] (EHVI itself,
    not negated), grad [M, D] (None without gradients), the partials G_m, G_s [K, M], the device's rounding-error bounds of all
    four (None with ``bound=False``), m, s [K, M], the level tables and the cells' factors D [K][C, M]."""
    lev = level_tables(mean, var, y_mean, y_std, levels, bound)
    K, M = len(lev), lev[0].m.size
    lo, hi = np.asarray(cell_lo, dtype=np.int64), np.asarray(cell_hi, dtype=np.int64)
    C = lo.shape[0]
    depth = (C + THREADS - 1) // THREADS + 9
    D = [lev[k].Psi[hi[:, k]] - lev[k].Psi[lo[:, k]] for k in range(K)]
    aD = [np.abs(d) for d in D]
    prod = D[0] * D[1] if K == 2 else D[0] * D[1] * D[2]
    value = prod.sum(0)
    dD = b_val = None
    if bound:
        dD = [lev[k].dPsi[hi[:, k]] + lev[k].dPsi[lo[:, k]] + U * aD[k] for k in range(K)]
        e = (K - 1) * (U * np.abs(prod) + ETA)
        for k in range(K):
            o, js = _prod_others(aD, k)
            e = e + dD[k] * o
        b_val = (e.sum(0) + depth * U * np.abs(prod).sum(0)) * (1 + T(1e-3))
    Gm, Gs = np.empty((K, M), T), np.empty((K, M), T)
    bGm, bGs = (np.empty((K, M), T), np.empty((K, M), T)) if bound else (None, None)
    for k in range(K):
        o, js = _prod_others(D, k)
        a = lev[k].Phi[lo[:, k]] - lev[k].Phi[hi[:, k]]
        b = lev[k].phi[hi[:, k]] - lev[k].phi[lo[:, k]]
        Gm[k], Gs[k] = (o * a).sum(0), (o * b).sum(0)
        if bound:
            if len(js) == 1:
                do = dD[js[0]]
            else:
                do = dD[js[0]] * aD[js[1]] + dD[js[1]] * aD[js[0]] + U * np.abs(o) + ETA
            da = lev[k].dPhi[lo[:, k]] + lev[k].dPhi[hi[:, k]] + U * np.abs(a)
            db = lev[k].dphi[lo[:, k]] + lev[k].dphi[hi[:, k]] + U * np.abs(b)
            ao = np.abs(o)
            bGm[k] = ((do * np.abs(a) + ao * da + U * np.abs(o * a) + ETA).sum(0) + depth * U * np.abs(o * a).sum(0)) * (1 + T(1e-3))
            bGs[k] = ((do * np.abs(b) + ao * db + U * np.abs(o * b) + ETA).sum(0) + depth * U * np.abs(o * b).sum(0)) * (1 + T(1e-3))
    grad = b_grad = None
    if dmdx is not None:
        gm = np.asarray(dmdx, dtype=np.float64).astype(T)
        gv = np.asarray(dvdx, dtype=np.float64).astype(T)
        grad = np.zeros(gm.shape[1:], T)
        b_grad = np.zeros(gm.shape[1:], T) if bound else None
        mag = np.zeros(gm.shape[1:], T)
        for k in range(K):
            ys = T(np.float64(y_std[k]))
            fa = ys * gm[k]
            fb = ys * ys * gv[k] / (2 * lev[k].s[:, None])
            A, B = Gm[k][:, None] * fa, Gs[k][:, None] * fb
            grad = grad + A + B
            if bound:
                mag = mag + np.abs(A) + np.abs(B)
                b_grad = b_grad + np.abs(fa) * bGm[k][:, None] + np.abs(fb) * bGs[k][:, None] + 3 * U * np.abs(A) + 7 * U * np.abs(B)
        if bound:
            b_grad = (b_grad + (K - 1) * U * mag + 6 * K * ETA) * (1 + T(1e-3))
    return Truth(value, grad, Gm, Gs, b_val, b_grad, bGm, bGs, np.stack([l.m for l in lev]), np.stack([l.s for l in lev]), lev, D)


def propagate(t, y_std, cell_lo, cell_hi, d_mean, d_sd, d_dm=None, d_dv=None, dmdx=None, dvdx=None):
    """What a posterior that is off by d_mean, d_sd [K, M] (normalised mean and standard deviation) and d_dm, d_dv [K, M, D] (their
    x-gradients; dv the variance's) moves EHVI and its gradient by, to first order, around the Truth ``t``:
        |d EHVI| <= sum_k |G_mk| dm_k + |G_sk| ds_k                         (dm, ds un-normalised: y_std d_mean, y_std d_sd)
    and for the gradient the same through the second partials of the cells' factors,
        d(Phi(l) - Phi(u)) / dm = (phi_u - phi_l) / s,       d(Phi(l) - Phi(u)) / ds = d(phi_u - phi_l) / dm = (z_u phi_u - z_l phi_l) / s,
        d(phi_u - phi_l) / ds = (z_u^2 phi_u - z_l^2 phi_l) / s,
    plus |G_mk| y_std d_dm + |G_sk| y_std^2 d_dv / (2 s) + |B| ds / s for the factors behind the partials."""
    lev, D = t.lev, t.D
    K, M = t.m.shape
    lo, hi = np.asarray(cell_lo, dtype=np.int64), np.asarray(cell_hi, dtype=np.int64)
    ys = np.asarray(y_std, dtype=np.float64).astype(T).reshape(K, 1)
    dm_, ds_ = ys * np.asarray(d_mean, dtype=T), ys * np.asarray(d_sd, dtype=T)
    tol_v = (np.abs(t.Gm) * dm_ + np.abs(t.Gs) * ds_).sum(0)
    if d_dm is None:
        return tol_v, None
    a, b, am, as_, bs = [], [], [], [], []
    for k in range(K):
        L = lev[k]
        zp, zzp = L.z * L.phi, L.z * L.z * L.phi
        s = L.s[None, :]
        a.append(L.Phi[lo[:, k]] - L.Phi[hi[:, k]])
        b.append(L.phi[hi[:, k]] - L.phi[lo[:, k]])
        am.append((L.phi[hi[:, k]] - L.phi[lo[:, k]]) / s)
        as_.append((zp[hi[:, k]] - zp[lo[:, k]]) / s)
        bs.append((zzp[hi[:, k]] - zzp[lo[:, k]]) / s)
    dGm, dGs = np.zeros((K, M), T), np.zeros((K, M), T)
    for k in range(K):
        o, js = _prod_others(D, k)
        dGm[k] = np.abs((o * am[k]).sum(0)) * dm_[k] + np.abs((o * as_[k]).sum(0)) * ds_[k]
        dGs[k] = np.abs((o * as_[k]).sum(0)) * dm_[k] + np.abs((o * bs[k]).sum(0)) * ds_[k]
        for j in js:
            rest = [i for i in js if i != j]
            r = D[rest[0]] if rest else T(1)
            dGm[k] += np.abs((a[k] * a[j] * r).sum(0)) * dm_[j] + np.abs((a[k] * b[j] * r).sum(0)) * ds_[j]
            dGs[k] += np.abs((b[k] * a[j] * r).sum(0)) * dm_[j] + np.abs((b[k] * b[j] * r).sum(0)) * ds_[j]
    gm = np.asarray(dmdx, dtype=np.float64).astype(T)
    gv = np.asarray(dvdx, dtype=np.float64).astype(T)
    tol_g = np.zeros(gm.shape[1:], T)
    for k in range(K):
        s = lev[k].s[:, None]
        fa, fb = ys[k] * gm[k], ys[k] * ys[k] * gv[k] / (2 * s)
        tol_g = tol_g + np.abs(fa) * dGm[k][:, None] + np.abs(fb) * dGs[k][:, None] \
            + np.abs(t.Gm[k])[:, None] * ys[k] * np.asarray(d_dm[k], dtype=T) \
            + np.abs(t.Gs[k])[:, None] * ys[k] * ys[k] * np.asarray(d_dv[k], dtype=T) / (2 * s) \
            + np.abs(t.Gs[k][:, None] * fb) * (ds_[k] / lev[k].s)[:, None]
    return tol_v, tol_g


# ---- decompositions (independent of the package's: tests/test_multi_objective_host.py holds the two against each other) ---------
def front_of(P):
    """The non-dominated rows of P [n, K], duplicates once, sorted lexicographically."""
    P = np.unique(np.asarray(P, dtype=float).reshape(-1, np.shape(P)[-1]), axis=0)
    keep = [i for i in range(len(P)) if not any(np.all(q <= P[i]) and np.any(q < P[i]) for q in P)]
    return P[keep]


def cells_of(P, ref):
    """(levels, cell_lo, cell_hi) of the region of (-inf, ref] the rows of P [n, K] do not dominate, K = 2 or 3."""
    ref = np.asarray(ref, dtype=float)
    K = ref.size
    P = np.asarray(P, dtype=float).reshape(-1, K)
    F = front_of(P[np.all(P < ref, axis=1)]) if len(P) else P
    levels = [np.concatenate(([-np.inf], np.unique(F[:, k]), [ref[k]])) for k in range(K)]
    idx = lambda k, v: int(np.flatnonzero(levels[k] == v)[0])
    lo, hi = [], []

    def strips(F2, tail_lo, tail_hi):
        F2 = front_of(F2) if len(F2) else F2
        a = [0] + [idx(0, p[0]) for p in F2] + [len(levels[0]) - 1]
        b = [len(levels[1]) - 1] + [idx(1, p[1]) for p in F2]
        for i in range(len(F2) + 1):
            lo.append((a[i], 0) + tail_lo)
            hi.append((a[i + 1], b[i]) + tail_hi)

    if K == 2:
        strips(F, (), ())
    else:
        for j in range(len(levels[2]) - 1):
            strips(F[F[:, 2] <= levels[2][j], :2], (j,), (j + 1,))
    return levels, np.array(lo, dtype=np.intc), np.array(hi, dtype=np.intc)


def synthetic_decomposition(K, L, C, seed=5):
    """A synthetic decomposition of K objectives with L levels each and C cells: random increasing levels over [-2, 2] and random
    index pairs lo < hi -- not a partition of anything, but every index and every cell slot the kernels can be given.
    ``synthetic_decomposition(3, MAX_LEVELS, MAX_CELLS)`` sits AT the caps."""
    rng = np.random.default_rng(seed)
    levels = [np.concatenate(([-np.inf], np.sort(rng.uniform(-2.0, 2.0, L - 1)))) for _ in range(K)]
    lo = rng.integers(0, L - 1, (C, K))
    hi = lo + 1 + (rng.integers(0, 4, (C, K)) * (rng.uniform(size=(C, K)) < 0.3))
    hi = np.minimum(hi, L - 1)
    lo[0], hi[0] = 0, L - 1                    # both ends of every level array are used
    return levels, lo.astype(np.intc), hi.astype(np.intc)


# ---- the case table -------------------------------------------------------------------------------------------------------------
# N = 120 training rows shared by the K objective handles (one tile with a ragged edge); D 2, 9, 17 (D = 17: eight locations are
# 136 > ROWS_MAX_XS = 128 doubles, a group splits into passes of four); K 2, 3; rows M 1, 5, 8, 11 (layouts MV = 1 / 4 / 8 and a
# second group); fronts of 0 .. 12 points; Matern-5/2 and Exponential, ARD and not.  `clip`: objective 0 has noise 1e-12 and a small
# output scale, and location 0 sits on one of its training points -- its variance lies below the clip at 1e-10.
Case = collections.namedtuple("Case", "id fam ard D K M nfront clip")
TABLE = (
    Case("a", "Mat52", True, 2, 2, 1, 5, False),
    Case("b", "Mat52", True, 9, 3, 5, 12, True),
    Case("c", "Exponential", False, 17, 2, 8, 12, False),
    Case("d", "Exponential", False, 9, 3, 11, 7, False),
    Case("e", "Mat52", False, 17, 3, 11, 4, True),
    Case("f", "Exponential", True, 2, 2, 8, 9, True),
)
CASES = {c.id: c for c in TABLE}
N_TRAIN = 120
PLACEMENTS = ("inside", "on_front", "dominated", "beyond")
Problem = collections.namedtuple("Problem", "case X Y variance ls ls_arg noise y_mean y_std Xs Xtab unit_front")


def _response(X, k):
    """A smooth objective over the unit box, different for every k."""
    D = X.shape[1]
    w = np.cos(0.9 * (k + 1) * np.arange(1, D + 1))
    return np.sin(1.7 * X @ w / np.sqrt(D) + 0.4 * k) + 0.6 * ((X - 0.3 - 0.2 * k) ** 2).sum(1) / D


@functools.lru_cache(maxsize=None)
def problem(cid):
    """The data of a case: inputs X shared by the K objectives, their standardised targets Y [N, K] with the standardisation
    (y_mean, y_std), kernel parameters shared by the handles, the rows' locations Xs, a table Xtab of 300 rows whose head is Xs,
    and a front of at most ``nfront`` points in unit coordinates (``placed_front`` maps it around a location's posterior)."""
    c = CASES[cid]
    rng = np.random.default_rng(3000 + ord(cid))
    X = rng.uniform(0, 1, (N_TRAIN, c.D))
    raw = np.stack([_response(X, k) * (0.05 if (c.clip and k == 0) else 1.0 + 0.7 * k) + 0.4 * k for k in range(c.K)], axis=1)
    raw = raw + 0.02 * raw.std(0) * rng.standard_normal(raw.shape) * np.array([0.0 if (c.clip and k == 0) else 1.0 for k in range(c.K)])
    y_mean, y_std = raw.mean(0), raw.std(0)
    Y = (raw - y_mean) / y_std
    noise = tuple(1e-12 if (c.clip and k == 0) else 1e-3 * (1 + k) for k in range(c.K))
    base = 0.5 * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.7, 1.4, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    Xtab = rng.uniform(0, 1, (300, c.D))
    if c.clip:
        Xtab[0] = X[7]
    Xs = Xtab[:c.M].copy()
    # (points of the plane sum_k p_k = 1 do not dominate each other: a front of exactly nfront points)
    front = front_of(rng.dirichlet(np.ones(c.K), c.nfront)) if c.nfront else np.empty((0, c.K))
    for a in (X, Y, ls_arg, ls, Xs, Xtab, front, y_mean, y_std):
        a.setflags(write=False)
    return Problem(c, X, Y, 1.3, ls, ls_arg, noise, y_mean, y_std, Xs, Xtab, front)


def placed_front(cid, placement, m0, s0):
    """A front (raw objective units) and a reference point that put location 0 -- un-normalised posterior mean m0 [K] and standard
    deviation s0 [K], from the CPU oracle: placement only -- where ``placement`` says: inside the non-dominated region, on a front
    point, deep in the dominated region (20 standard deviations behind a front point in every objective), beyond the reference point.  The unit
    front of the case is mapped by  y = m0 + S (p - anchor)  with S a few (inside, on_front) or 40 (dominated, beyond) standard
    deviations per unit."""
    p = problem(cid)
    F = p.unit_front
    ref = np.full(p.case.K, 2.0)
    pivot = F[len(F) // 2] if len(F) else np.full(p.case.K, 0.5)
    if placement == "inside":
        anchor, scale = pivot - 0.05, 4.0
    elif placement == "on_front":
        anchor, scale = pivot.copy(), 4.0
    elif placement == "dominated":
        anchor, scale = pivot + 0.5, 40.0
    elif placement == "beyond":
        anchor, scale = ref + 0.2, 40.0
    else:
        raise ValueError(placement)
    S = scale * np.asarray(s0, dtype=float)
    return np.asarray(m0, dtype=float) + S * (F - anchor), np.asarray(m0, dtype=float) + S * (ref - anchor)
