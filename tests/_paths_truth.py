"""Posterior paths (pathwise conditioning; Wilson et al., ICML 2020) in ``np.longdouble`` (x87 80-bit, eps 1.1e-19) from explicit
draws, the rounding-error bound of the device's prior term, and the case table of tests/test_gpu_paths.py and
tests/test_paths_truth_host.py.

    omega_jd = omega_unit_jd / l_d,   a = sqrt(2 variance / F),   d = noise + 1e-8 + jitter
    Phi(X)_nj = a cos(omega_j . X_n + b_j),   r_s = y - Phi(X) w_s - sqrt(d) z_s,   V_s = (K + d I)^-1 r_s     (Cholesky, long double)
    prior_s(x)  = a sum_j w_sj cos(omega_j . x + b_j)              d prior_s / dx  = -a sum_j w_sj omega_j sin(omega_j . x + b_j)
    update_s(x) = sum_n k(x, X_n) V_sn                             d update_s / dx = sum_n dk(x, X_n)/dx V_sn
    f_s = prior_s + update_s;   dk/dx_q = dK_dr (x_q - X_nq) / (l_q^2 r), 0 where r = 0 (the _inv_dist convention)

Nothing here imports the library or needs a GPU; everything is computed once per case and read-only.  The four families and the
long-double Cholesky are tests/_sparse_ref.py's.

The update term is the posterior mean of a GP fitted to the targets r_s, so the device's is held to the tolerance
tests/test_gpu_rows.py grants the mean and its gradient (1e-6 of max(1, |m|), 1e-6 of max(max |dm|, 1e-3)), |m| read as
max(1, max_n |r_sn|): ``update_tolerance``.

The prior term's bound follows the device operation by operation, u = 2^-53 (csrc/paths.hip: paths_arg, the cos tiles against
the matrix cores, paths_rows_kernel):

* omega_jd: one division, u relative.  arg = b + sum_d omega_jd x_d as D fused multiply-adds from b on: with the frequencies' own
  rounding  |d arg| <= (D + 2) u A,  A = |b| + sum_d |omega_jd x_d|   -- the argument error grows with |omega . x + b|
* cos / sin of the library: within 2 ulp of a value of magnitude <= 1, and they move by at most |d arg|:  |d c| <= |d arg| + 2 u
* the products w c (values; fused on the matrix cores, rounded in the rows kernel) and w s omega_d (gradients: two roundings) and
  the sum over j: in ANY order a sum of F terms is good to (F - 1) u sum |term|; with the products' roundings (F + 2) u sum |term|
* a: a division, a product and a square root, 2 u relative; the scaling by a one more: 3 u of the result
      bound(prior)     = a sum_j |w_j| (|d arg_j| + 2 u) + ((F + 2) u + 3 u) a sum_j |w_j c_j|
      bound(d prior_q) = a sum_j |w_j omega_jq| (|d arg_j| + 2 u) + ((F + 2) u + 3 u) a sum_j |w_j s_j omega_jq|
all times (1 + 1e-3) for the terms of second order.  ``combine`` adds what the entries do to the two terms: f = a P + U (one
fma), y_std f + y_mean (one fma) -- 2 u (|f| y_std + |y_mean|) -- and for the gradient the division of the update's sum by l_q
and the two products, 4 u |.|.
"""
import collections
import functools

import numpy as np

import _mes_truth as MT
import _sparse_ref as SR

T = np.longdouble
U = T(2.0) ** -53
LD, F64 = SR.LD, SR.F64

FAMILY_ID = {"rbf": 0, "Mat52": 1, "Mat32": 2, "Exponential": 3}      # GP_KERNEL_* of include/gphip.h
NU = {"rbf": None, "Mat52": 2.5, "Mat32": 1.5, "Exponential": 0.5}
NOISE = MT.NOISE
Y_MEAN, Y_STD = 0.3, 1.7      # the output normaliser of every evaluation
VARIANCE = 1.3
M_TABLE = 300                 # crosses a 256-row chunk of the arg-best reduction and four 64-candidate workgroups, ragged
M_ROWS = 8
TOL = 1e-6                    # tests/test_gpu_rows.py: the mean's and its gradient's tolerance against the oracle

# all four families, ARD and not; D 1 and 5 (and one case at D = 20, beyond what one pass of eight locations takes); N 130 and
# 257 (a 128-row tile crossed once and twice, ragged); F 50 and 130 (no multiple of 4 or 16); S 1, 3 and 17 (one tile of 16 paths,
# and two)
Case = collections.namedtuple("Case", "id fam ard D N F S")
TABLE = (
    Case("a", "rbf", True, 5, 130, 50, 1),
    Case("b", "rbf", False, 1, 257, 130, 3),
    Case("c", "Mat52", True, 1, 257, 50, 17),
    Case("d", "Mat52", False, 5, 130, 130, 3),
    Case("e", "Mat32", True, 5, 257, 130, 17),
    Case("f", "Mat32", False, 1, 130, 50, 1),
    Case("g", "Exponential", True, 5, 257, 50, 3),
    Case("h", "Exponential", False, 5, 130, 130, 17),
    Case("i", "Mat52", True, 20, 130, 50, 10),       # D > 16: a rows call of 8 locations no longer fits one pass (M D <= 128)
)
CASES = {c.id: c for c in TABLE}
Problem = collections.namedtuple("Problem", "case X Y ls ls_arg Xs Xtab draws")
Truth = collections.namedtuple("Truth", "prior update dprior dupdate V r bound dbound")


def sigma2(noise, jitter=0.0):
    """The diagonal of the factor, as the library forms it in double."""
    return (float(noise) + 1e-8) + float(jitter)


def unit_frequencies(fam, D, F, rng):
    """The recipe of posterior_paths.unit_frequencies, restated: N(0, I), or the multivariate t with 2 nu degrees of freedom."""
    z = rng.standard_normal((F, D))
    if NU[fam] is None:
        return z
    return z * np.sqrt(2.0 * NU[fam] / rng.chisquare(2.0 * NU[fam], size=F))[:, None]


def draws(fam, N, D, S, F, seed):
    rng = np.random.default_rng(seed)
    return (unit_frequencies(fam, D, F, rng), rng.uniform(0.0, 2.0 * np.pi, F), rng.standard_normal((S, F)),
            rng.standard_normal((S, N)))


@functools.lru_cache(maxsize=None)
def problem(cid):
    """The data of a case: (X, Y) standardised, lengthscales, the draws, the rows' locations Xs [8, D] -- six random ones and two
    training inputs (a coincident point: the Exponential's kink) -- and the table Xtab [300, D] whose head is Xs."""
    c = CASES[cid]
    rng = np.random.default_rng(7000 + ord(cid))
    X = rng.uniform(0, 1, (c.N, c.D))
    Y = (MT._response(X) + 0.05 * rng.standard_normal(c.N))[:, None]
    Y = (Y - Y.mean()) / Y.std()
    base = 0.5 * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.7, 1.4, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    Xtab = rng.uniform(0, 1, (M_TABLE, c.D))
    Xtab[M_ROWS - 2] = X[0]
    Xtab[M_ROWS - 1] = X[c.N - 1]
    Xs = Xtab[:M_ROWS].copy()
    dr = draws(c.fam, c.N, c.D, c.S, c.F, 7100 + ord(cid))
    for a in (X, Y, ls_arg, ls, Xs, Xtab) + dr:
        a.setflags(write=False)
    return Problem(c, X, Y, ls, ls_arg, Xs, Xtab, dr)


def _scaled_diff(A, B, ls):
    """(A_i - B_n) / l [Ma, Nb, D] and r [Ma, Nb]."""
    diff = (A[:, None, :] - B[None, :, :]) / ls
    return diff, np.sqrt((diff * diff).sum(-1))


def evaluate(fam, variance, ls, d, X, y, dr, Xq, lin=LD, grad=True, bounds=True):
    """The paths of the draws ``dr`` at the rows of ``Xq`` in the arithmetic ``lin``: a ``Truth`` of prior / update [S, M], their
    gradients [S, M, D] (``grad``), V [S, N], the targets r [S, N], and the prior term's device bound and its gradient's
    (``bounds``; long double whatever ``lin``)."""
    t = lin.dtype
    X, Xq, ls = np.asarray(X, dtype=t), np.asarray(Xq, dtype=t), np.asarray(ls, dtype=t)
    y = np.asarray(y, dtype=t).ravel()
    omega_unit, phase, w, z = (np.asarray(a, dtype=t) for a in dr)
    S, F = w.shape
    D = X.shape[1]
    variance, d = t(variance), t(d)
    omega = omega_unit / ls
    amp = np.sqrt(2 * variance / F)
    PhiX = amp * np.cos(X @ omega.T + phase)
    r = y[None, :] - w @ PhiX.T - np.sqrt(d) * z
    _, rXX = _scaled_diff(X, X, ls)
    K = SR.k_of_r(fam, variance, rXX) + d * np.eye(X.shape[0], dtype=t)
    L = lin.chol(K)[0].astype(t)
    V = lin.solve(L, lin.solve(L, r.T, 0), 1).astype(t).T
    arg = Xq @ omega.T + phase
    c, s = np.cos(arg), np.sin(arg)
    prior = amp * (w @ c.T)
    diff, rq = _scaled_diff(Xq, X, ls)
    update = V @ SR.k_of_r(fam, variance, rq).T
    dprior = dupdate = None
    if grad:
        dprior = -amp * np.einsum("sj,mj,jq->smq", w, s, omega)
        safe = np.where(rq > 0, rq, t(1))
        G = np.where(rq > 0, SR.dk_dr(fam, variance, rq) / safe, t(0))      # dK_dr / r, 0 on coincident pairs
        dupdate = np.einsum("sn,mn,mnq->smq", V, G, diff) / ls
    bound = dbound = None
    if bounds:
        A = np.abs(phase)[None, :] + np.abs(Xq[:, None, :] * omega[None, :, :]).sum(-1)          # [M, F]
        darg = (D + 2) * U * A + 2 * U
        aw = np.abs(w)
        scale = (1 + T(1e-3)) * amp
        sumu = (F + 5) * U
        bound = scale * (aw @ darg.T + sumu * (aw @ np.abs(c).T))
        if grad:
            ao = np.abs(omega)
            dbound = scale * (np.einsum("sj,mj,jq->smq", aw, darg, ao) + sumu * np.einsum("sj,mj,jq->smq", aw, np.abs(s), ao))
    return Truth(prior, update, dprior, dupdate, V, r, bound, dbound)


@functools.lru_cache(maxsize=None)
def truth(cid, jitter=0.0):
    """The long-double paths of a case over its table (values) -- the head M_ROWS rows carry the gradients as well."""
    p = problem(cid)
    c = p.case
    d = sigma2(NOISE, jitter)
    tab = evaluate(c.fam, VARIANCE, p.ls, d, p.X, p.Y, p.draws, p.Xtab, grad=False)
    rows = evaluate(c.fam, VARIANCE, p.ls, d, p.X, p.Y, p.draws, p.Xs, grad=True)
    for a in tab + rows:
        if a is not None:
            a.setflags(write=False)
    return tab, rows


def update_tolerance(tr):
    """Per path: (value tolerance, gradient tolerance) of the update term, in the model's normalised units."""
    rmax = np.maximum(1.0, np.abs(tr.r).max(axis=1).astype(np.float64))
    vt = TOL * rmax
    gt = None
    if tr.dupdate is not None:
        gt = TOL * np.maximum(np.abs(tr.dupdate).reshape(tr.dupdate.shape[0], -1).max(axis=1).astype(np.float64), 1e-3)
    return vt, gt


def combine(tr, y_mean=Y_MEAN, y_std=Y_STD):
    """What an entry returns and what it may be off by: (value [S, M], its allowance, gradient [S, M, D] or None, its allowance)."""
    vt, gt = update_tolerance(tr)
    f = tr.prior + tr.update
    val = y_std * f + y_mean
    allow = y_std * (tr.bound + vt[:, None]) + 2 * U * (np.abs(f) * y_std + abs(y_mean))
    if tr.dprior is None:
        return val, allow, None, None
    g = y_std * (tr.dprior + tr.dupdate)
    gallow = y_std * (tr.dbound + gt[:, None, None]) + 4 * U * y_std * (np.abs(tr.dprior) + np.abs(tr.dupdate))
    return val, allow, g, gallow
