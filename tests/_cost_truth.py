"""The cost surface of cost-aware EI / MPI in ``np.longdouble`` (x87 80-bit, eps 1.1e-19), the rounding-error bound of the
device's evaluation of it, and the case table of tests/test_gpu_cost.py and tests/test_cost_truth_host.py.

    logc(x)        = shift + scale sum_j alpha_j k(r_j),              r_j = |(x - Xc_j) / l|
    dlogc(x)/dx_d  = scale / l_d sum_j alpha_j g(r_j) (x_d - Xc_jd) / l_d,      g = dK_dr / r   (0 at r = 0 for the Exponential:
                                                                                  _inv_dist, stationary.py:251-258)

with k of the four Euclidean families (rbf.py:50-54, stationary.py:388-392, 478-482, 575-579), written here from the formulas.
Nothing here imports the library or needs a GPU; everything is computed once per case and read-only.

The bound (``surface`` returns it beside the truth) follows csrc/cost.hip operation by operation, u = 2^-53 the unit roundoff:

* a_d = fl(x_d / l_d), b_jd = fl(Xc_jd / l_d) (one rounding each), df_d = fl(a_d - b_jd):
      |delta df_d| <= e_d = u (|a_d| + |b_jd| + |df_d|)
* r2 = sum_d df_d^2 by D fma:  |delta r2| <= sum_d 2 |df_d| e_d + D u r2;  r = sqrt(r2):
      delta r <= |e|_2 + (D / 2 + 1) u r                                         (Cauchy-Schwarz on sum |df_d| e_d / r)
* k = variance * polynomial(r) * exp(arg), arg = -(r2 / 2, sqrt5 r, sqrt3 r, r):  the rounding of arg is |arg| u relative to k,
  exp is within 4 ulp = 8 u (DESIGN.md quotes it), the polynomial has at most 3 roundings over positive terms, the products 2:
      |delta k| <= |k'(r)| delta r + k u (13 + |arg|)
  and in the same way |delta g| <= |g'(r)| delta r + |g| u (14 + |arg|) (one more for the Exponential's division)
* the sum: chunks of COST_CB = 32 terms accumulated by fma in order (<= 32 roundings on a term's path), the nchunk partial sums
  added in order (<= nchunk more): (32 + nchunk) u sum_j |term_j|; the gradient's term alpha g df has two more roundings of its own
* logc = fma(scale, total, shift): u |logc|;  dlogc_d = fl(fl(scale total) / l_d): 2 u |dlogc_d|

      bound(logc)    = |scale| (sum_j |alpha_j| |delta k_j| + (32 + nchunk) u sum_j |alpha_j k_j|) + u |logc|
      bound(dlogc_d) = |scale| / l_d (sum_j |alpha_j| (|delta g_j| |df_jd| + |g_j| e_jd)
                                     + (34 + nchunk) u sum_j |alpha_j g_j df_jd|) + 2 u |dlogc_d|

both times (1 + 1e-3) for the terms of second order.  In the issue's form gamma eps sum_j |alpha_j k_j| |scale|: gamma =
(32 + nchunk + 13 + |arg|) / 2 from the summation, the combining order and the covariance, plus the distance's share
|k'| delta r / (k eps), which is D-proportional where the inputs are well separated and is evaluated term by term instead of
being bounded by a constant.
"""
import collections
import functools

import numpy as np

T = np.longdouble
U = T(2.0) ** -53
COST_CB = 32
KERNEL_IDS = {"rbf": 0, "Mat52": 1, "Mat32": 2, "Exponential": 3}
S5, S3 = np.sqrt(T(5)), np.sqrt(T(3))


# ---- the four families in long double: k, g = k' / r, |k'|, |g'|, |arg| as functions of r ------------------------------------------
def family(name, variance, r):
    v = T(variance)
    with np.errstate(divide="ignore", invalid="ignore"):
        if name == "rbf":
            k = v * np.exp(-r * r / 2)
            return k, -k, r * k, r * k, r * r / 2
        if name == "Mat52":
            e = np.exp(-S5 * r)
            k = v * (1 + S5 * r + T(5) / 3 * r * r) * e
            g = -T(5) / 3 * v * (1 + S5 * r) * e
            return k, g, np.abs(g) * r, T(25) / 3 * v * r * e, S5 * r
        if name == "Mat32":
            e = np.exp(-S3 * r)
            return v * (1 + S3 * r) * e, -3 * v * e, 3 * v * r * e, 3 * S3 * v * e, S3 * r
        if name == "Exponential":
            k = v * np.exp(-r)
            zero = r == 0
            safe = np.where(zero, T(1), r)
            g = np.where(zero, T(0), -k / safe)
            dg = np.where(zero, T(0), k * (1 / safe + 1 / (safe * safe)))
            return k, g, k, dg, r
    raise KeyError(name)


def surface(name, variance, ls, Xc, alpha, shift, scale, Xs, block=64):
    """(logc [M], dlogc [M, D], bound_logc [M], bound_dlogc [M, D], sum_abs [M]) in long double; ``ls`` [D] (isotropic: repeated).
    sum_abs = |scale| sum_j |alpha_j k_j|, the scale of the issue's bound."""
    Xc, Xs = np.asarray(Xc), np.asarray(Xs)                          # (doubles, or long doubles as they are: tests/_domain_cases.py)
    l = np.asarray(ls, dtype=np.float64).astype(T)
    al = np.asarray(alpha, dtype=np.float64).astype(T)
    Nc, D = Xc.shape
    M = Xs.shape[0]
    nchunk = -(-Nc // COST_CB)
    b = Xc.astype(T) / l
    sh, sc = T(shift), T(scale)
    logc, sabs, blog = np.empty(M, T), np.empty(M, T), np.empty(M, T)
    dlogc, bd = np.empty((M, D), T), np.empty((M, D), T)
    for m0 in range(0, M, block):
        a = Xs[m0:m0 + block].astype(T) / l                       # [m, D]
        df = a[:, None, :] - b[None, :, :]                        # [m, Nc, D]
        r = np.sqrt((df * df).sum(-1))                            # [m, Nc]
        k, g, dk, dg, arg = family(name, variance, r)
        e = U * (np.abs(a)[:, None, :] + np.abs(b)[None, :, :] + np.abs(df))
        dr = np.sqrt((e * e).sum(-1)) + (T(D) / 2 + 1) * U * r
        delk = dk * dr + k * U * (13 + arg)
        delg = dg * dr + np.abs(g) * U * (14 + arg)
        tot = (al * k).sum(-1)
        abs_k = (np.abs(al) * k).sum(-1)
        lc = sh + sc * tot
        logc[m0:m0 + block] = lc
        sabs[m0:m0 + block] = np.abs(sc) * abs_k
        blog[m0:m0 + block] = (np.abs(sc) * ((np.abs(al) * delk).sum(-1) + (COST_CB + nchunk) * U * abs_k) + U * np.abs(lc)) * (1 + T(1e-3))
        terms = (al * g)[:, :, None] * df                          # [m, Nc, D]
        gl = sc * terms.sum(1) / l
        dlogc[m0:m0 + block] = gl
        err = (np.abs(al)[None, :, None] * (delg[:, :, None] * np.abs(df) + np.abs(g)[:, :, None] * e)).sum(1)
        err = err + (COST_CB + 2 + nchunk) * U * np.abs(terms).sum(1)
        bd[m0:m0 + block] = (np.abs(sc) / l * err + 2 * U * np.abs(gl)) * (1 + T(1e-3))
    return logc, dlogc, blog, bd, sabs


# ---- the case table -------------------------------------------------------------------------------------------------------------
# Nc 1, 63, 65, 257, 1000 (one term; either side of two chunks; a ragged chunk behind two full LDS tiles; 8 tiles) and 8225 (257
# chunks and one term: a second round of the few-rows kernel's 256 threads); D 1, 3, 8 (registers), 64 = GP_MAX_D (LDS, 8 gradient passes);
# M 1, 5, 8 (few rows), 9, 130, 1025 (tables: one workgroup, three, seventeen with a ragged last one); all four families, ARD and
# not; `same`: table rows equal to a row of the surface (r = 0); one normaliser with shift != 0, scale != 1.
Case = collections.namedtuple("Case", "id fam ard Nc D M shift scale same")
TABLE = (
    Case("a", "rbf", False, 1, 1, 1, 0.0, 1.0, ()),
    Case("b", "Mat52", True, 63, 3, 5, 0.0, 1.0, ()),
    Case("c", "Mat32", False, 65, 8, 8, 0.0, 1.0, ()),
    Case("d", "Exponential", True, 257, 3, 9, 0.0, 1.0, (2, 7)),
    Case("e", "Mat52", False, 1000, 8, 130, -1.3, 0.7, ()),
    Case("f", "rbf", True, 1000, 3, 1025, 0.0, 1.0, ()),
    Case("g", "Mat32", True, 257, 64, 9, 0.0, 1.0, ()),
    Case("h", "Exponential", False, 65, 64, 5, 0.0, 1.0, (1,)),
    Case("i", "rbf", False, 257, 64, 130, 0.4, 1.9, ()),
    Case("j", "Mat52", True, 1000, 1, 1025, 0.0, 1.0, (0, 1024)),
    Case("k", "Exponential", False, 63, 8, 130, 0.0, 1.0, (5, 129)),
    Case("l", "Mat32", False, 1, 3, 9, 0.0, 1.0, ()),
    Case("m", "Mat52", False, 8225, 3, 9, 0.0, 1.0, ()),
)
CASES = {c.id: c for c in TABLE}
Problem = collections.namedtuple("Problem", "case Xc alpha variance ls ls_arg Xs")


@functools.lru_cache(maxsize=None)
def problem(cid):
    """The data of a case: a surface in the unit box, weights of both signs, lengthscales that keep r of order one at every D, and
    locations of which ``same`` coincide with rows of the surface."""
    c = CASES[cid]
    rng = np.random.default_rng(1000 + ord(cid))
    Xc = rng.uniform(0, 1, (c.Nc, c.D))
    alpha = rng.standard_normal(c.Nc) * rng.uniform(0.1, 2.0, c.Nc)
    base = 0.4 * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.6, 1.6, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    Xs = rng.uniform(0, 1, (c.M, c.D))
    for n, row in enumerate(c.same):
        Xs[row] = Xc[(7 * n + 3) % c.Nc]
    for a in (Xc, alpha, ls_arg, ls, Xs):
        a.setflags(write=False)
    return Problem(c, Xc, alpha, 1.0 + 0.1 * (ord(cid) % 5), ls, ls_arg, Xs)


@functools.lru_cache(maxsize=None)
def truth(cid):
    p = problem(cid)
    out = surface(p.case.fam, p.variance, p.ls, p.Xc, p.alpha, p.case.shift, p.case.scale, p.Xs)
    for a in out:
        a.setflags(write=False)
    return out
