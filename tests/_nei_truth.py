"""Noisy expected improvement and its gradient in ``np.longdouble`` (x87 80-bit, eps 1.1e-19) from the raw data -- the kernel
build, Cholesky and substitutions of tests/_qei_truth.py, BOTH factors, no inverse factor -- and the case table of
tests/test_gpu_nei.py and tests/test_nei_truth_host.py.  ``float64_restatement`` is the same algorithm in plain float64: the
yardstick of the device's gradient error.  Nothing here imports the library or needs a GPU; everything is computed once per case
and read-only.

    L L^T = Ky = K + d I (the model),  L0 L0^T = K0 = K + d0 I (the twin),  d = noise + 1e-8 + jitter,  d0 = twin_noise + 1e-8 + jitter0
    g_s = L0 z_s,  r_s = y - g_s - sqrt(d - d0) e_s,  V_s = Ky^-1 r_s,  F_s = y - sqrt(d - d0) e_s - (d - d0) V_s
    a_s = K0^-1 F_s,  fstar_s = min_i F_is
    k = k(X, x),  w = L0^-1 k,  v = y_std^2 (kss - |w|^2 + twin_noise) floored at 1e-10,  s = sqrt(v) floored at 1e-10
    mu_s = y_std k . a_s + y_mean,  t_s = y_std fstar_s + y_mean,  u_s = (t_s - par - mu_s) / s
    NEI = (1 / S) sum_s s (u_s Phi(u_s) + phi(u_s))
    dNEI/dx = -y_std J^T (A0 p) + c ds/dx,  p_s = Phi(u_s) / S,  c = (1 / S) sum_s phi(u_s),  ds/dx = -(y_std^2 / s) J^T L0^-T w (0 at the floor)

Phi comes from mpmath at 40 digits.

The cases: N 130 / 300 / 1100 (two 128-row blocks, three, two 1024-column chunks), S 1 / 16 / 17 / 64 (one fantasy, either side of
the padding to 16, the limit), table M 1 / 33 / 300, rows M 1 / 4 / 8 (the three pass layouts), D up to 16 with M D = 128, all four
families, ARD and not, model noise 1e-2 and 1e-1, twin noise 1e-6 and 1e-4, locations ON a training input (d: no floor at
y_std 1.7; e: y_std = 1e-3, where the variance's floor holds).  Every case must have at least half of the table's locations and
at least half of the gradient rows with NEI >= 1000 allowances, and d - d0 >= 100 d0: ``conditions`` computes what
tests/test_nei_truth_host.py asserts.  The seeds and scales below were chosen on the CPU under these conditions (smooth models at
lengthscale 0.3 sqrt(D) give NEI that underflows at most locations).
"""
import collections
import functools

import mpmath
import numpy as np

from _qei_truth import (FAMILY_ID, PAR, T, VARIANCE, Y_MEAN, Y_STD, _scaled_diff, dk_dr_over_r, fit, k_of_r, rel_tol, response,      # noqa: F401
                        sigma2, solve, tolerances)

MARGIN_FACTOR = 1000.0
FLOOR = 1e-10
NOISE_RATIO = 100.0

# Mt: rows of the table; Mr: its leading rows also go through gp_nei_rows with gradients
Case = collections.namedtuple("Case", "id N D S Mt Mr fam ard noise twin_noise seed ls_scale spread y_std par")
TABLE = (
    Case("a", 130, 2, 1, 1, 1, "Mat52", False, 1e-2, 1e-6, 0, 0.03, 0.15, Y_STD, PAR),          # one fantasy, one row, one location
    Case("b", 300, 3, 16, 33, 4, "Exponential", True, 1e-1, 1e-4, 0, 0.1, 0.05, Y_STD, PAR),    # three row blocks, the narrow pass; S a whole tile
    Case("c", 300, 16, 17, 33, 8, "rbf", True, 1e-2, 1e-6, 0, 0.1, 0.05, Y_STD, PAR),           # M D = 128, the limit of the wide pass; S one past the tile
    Case("d", 1100, 4, 64, 300, 8, "Mat32", False, 1e-1, 1e-6, 0, 0.1, 0.05, Y_STD, PAR),       # two column chunks, the limit of S; a location ON a training input
    # a location ON a training input under a small output scale: y_std^2 v ~ 1e-12, the floor of 1e-10 holds there (at y_std = 1.7
    # the variance on a training input, about the twin's noise, stays above the floor: case d has that location)
    # (the acquisition's jitter scales with the outputs: 0.01 would put every improvement at y_std = 1e-3 ten scales out of reach)
    Case("e", 130, 2, 16, 33, 4, "Mat52", False, 1e-2, 1e-6, 0, 0.03, 0.15, 1e-3, 1e-5),
)
CASES = {c.id: c for c in TABLE}
Problem = collections.namedtuple("Problem", "case X Y ls ls_arg Xs Z E")


@functools.lru_cache(maxsize=None)
def problem(cid):
    c = CASES[cid]
    rng = np.random.default_rng(8000 + ord(cid))
    X = rng.uniform(0, 1, (c.N, c.D))
    Y = (response(X) + 0.1 * rng.standard_normal(c.N))[:, None]
    Y = (Y - Y.mean()) / Y.std()
    base = c.ls_scale * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.7, 1.4, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    rng = np.random.default_rng(8100 + 131 * ord(cid) + c.seed)
    # the locations crowd the low region of the data -- the best observations, perturbed -- where an improvement is likely
    low = np.argsort(Y[:, 0], kind="stable")[:16]
    Xs = np.clip(X[low[np.arange(c.Mt) % 16]] + c.spread * rng.standard_normal((c.Mt, c.D)), 0, 1)
    if cid in "de":
        Xs[2] = X[17]                             # on a training input (e: the variance's floor holds)
    # the draws: GP_NEI_MAX_S rows, the case uses the leading S (the device must give the same bits for them)
    Z = rng.standard_normal((64, c.N))
    E = rng.standard_normal((64, c.N))
    for a in (X, Y, ls_arg, ls, Xs, Z, E):
        a.setflags(write=False)
    return Problem(c, X, Y, ls, ls_arg, Xs, Z, E)


# ---- Phi and phi in the operands' dtype ------------------------------------------------------------------------------------------------
def _mp(x):
    x = T(x)
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - T(hi)))


def _back(x, t):
    x = mpmath.mpf(x)
    hi = float(x)
    return t(hi) + t(float(x - mpmath.mpf(hi)))


def normal_cdf(u):
    """Phi of every entry of ``u`` at 40 digits, rounded to u's dtype."""
    t = u.dtype.type
    out = np.empty_like(u)
    with mpmath.workdps(40):
        for i, x in np.ndenumerate(u):
            out[i] = _back(mpmath.ncdf(_mp(x)), t)
    return out


def normal_pdf(u):
    t = u.dtype.type
    return np.exp(-u * u / 2) / np.sqrt(2 * t(np.pi))


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
Fantasies = collections.namedtuple("Fantasies", "fit fit0 F fstar A0 dd")


def fantasies(fam, variance, ls, d, d0, X, y, Z, E, dtype=T):
    """The S fantasies of the noiseless training values from the draws Z, E [S, N]: both factors, F [N, S], fstar [S], A0 [N, S]."""
    t = dtype
    if not d > d0:
        raise ValueError("noisy EI needs d > d0: %r against %r" % (d, d0))
    f = fit(fam, variance, ls, d, X, y, t)
    f0 = fit(fam, variance, ls, d0, X, y, t)
    yv = np.asarray(y, dtype=t).ravel()[:, None]
    dd = t(d) - t(d0)
    G = f0.L @ np.asarray(Z, dtype=t).T                                  # [N, S]
    B = yv - np.sqrt(dd) * np.asarray(E, dtype=t).T
    R = B - G
    V = solve(f.L, solve(f.L, R, 0), 1)
    F = B - dd * V
    A0 = solve(f0.L, solve(f0.L, F, 0), 1)
    return Fantasies(f, f0, F, F.min(0), A0, dd)


Truth = collections.namedtuple("Truth", "F fstar value grad p c s floored m beta1 mean_norm")


def evaluate(fam, variance, twin_noise, fa, Xs, ngrad=0, par=PAR, y_mean=Y_MEAN, y_std=Y_STD):
    """NEI of every row of Xs over the fantasies ``fa``, and the gradient of the leading ``ngrad`` rows, in the arithmetic of the
    fits: a ``Truth`` (per row: value, p [S], c, s, the floor's flag, the normalised means m [S], ||K0^-1 k||_1)."""
    f0 = fa.fit0
    t = f0.X.dtype.type
    Xs = np.asarray(Xs, dtype=t)
    M, D = Xs.shape
    S = fa.F.shape[1]
    ys, ym = t(y_std), t(y_mean)
    dX, rX = _scaled_diff(Xs, f0.X, f0.ls)
    k = k_of_r(fam, t(variance), rX)                                     # [M, N]
    W = solve(f0.L, k.T, 0)                                              # [N, M]
    beta = solve(f0.L, W, 1)                                             # [N, M]: K0^-1 k
    var = (t(variance) - (W * W).sum(0)) + t(twin_noise)
    v = var * (ys * ys)
    floored = v < t(FLOOR)
    s = np.maximum(np.sqrt(np.where(floored, t(FLOOR), v)), t(1e-10))
    m = k @ fa.A0                                                        # [M, S]
    mu = m * ys + ym
    tt = fa.fstar * ys + ym
    u = (tt[None, :] - mu - t(par)) / s[:, None]
    Phi, phi = normal_cdf(u), normal_pdf(u)
    value = (s[:, None] * (u * Phi + phi)).sum(1) / S
    p, c = Phi / S, phi.sum(1) / S
    grad = np.zeros((ngrad, D), dtype=t)
    if ngrad:
        gX = dk_dr_over_r(fam, t(variance), rX[:ngrad])                  # [ngrad, N]
        for i in range(ngrad):
            J = gX[i][:, None] * dX[i] / f0.ls                           # [N, D]: d k(X, x) / dx
            ds = t(0) * J[0] if floored[i] else -(ys * ys / s[i]) * (J.T @ beta[:, i])
            grad[i] = -ys * (J.T @ (fa.A0 @ p[i])) + c[i] * ds
    mean_norm = float(max(1.0, np.max(np.abs(m))))
    return Truth(fa.F.T.copy(), fa.fstar, value, grad, p, c, s, floored, m, np.abs(beta).sum(0), mean_norm)


def tol_F(noise, F):
    """What the fantasies are granted: the project's relative tolerance at the MODEL's noise (they come through its factor) on
    max(1, max |F|)."""
    return rel_tol(noise) * max(1.0, float(np.max(np.abs(F))))


def allowance(c, tr, y_mean=Y_MEAN):
    """Per location, first order from the adjoint: sum_s p_s tol_m + |dNEI/ds| tol_s + sum_s p_s y_std (tol_F + ||beta||_1 tol_F)
    + 64 eps (max |t| + max |mu| + par).  tol_m and the variance's tolerance are _qei_truth.tolerances' at the twin's noise (s moves
    with the variance: tol_s = tol_v / (2 s)); tol_F above."""
    tol_m, tol_v = tolerances(c.twin_noise, tr.mean_norm, VARIANCE, c.y_std)
    s = np.asarray(tr.s, dtype=float)
    tol_s = tol_v / (2.0 * s)
    tf = tol_F(c.noise, tr.F)
    psum = np.asarray(tr.p, dtype=float).sum(1)
    scale = c.y_std * (float(np.max(np.abs(tr.fstar))) + float(np.max(np.abs(tr.m)))) + 2 * abs(y_mean) + c.par
    return (psum * tol_m + np.abs(np.asarray(tr.c, dtype=float)) * tol_s
            + psum * c.y_std * (tf + np.asarray(tr.beta1, dtype=float) * tf) + 64 * np.finfo(np.float64).eps * scale)


Solved = collections.namedtuple("Solved", "p fan truth allowance tol_F d d0")


def solve_case(c, p, jitter=0.0, jitter0=0.0, dtype=T):
    d, d0 = sigma2(c.noise, jitter), sigma2(c.twin_noise, jitter0)
    fa = fantasies(c.fam, VARIANCE, p.ls, d, d0, p.X, p.Y, p.Z[:c.S], p.E[:c.S], dtype)
    tr = evaluate(c.fam, VARIANCE, c.twin_noise, fa, p.Xs, c.Mr, par=c.par, y_std=c.y_std)
    for a in tr:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    allow = allowance(c, tr)
    allow.setflags(write=False)
    return Solved(p, fa, tr, allow, tol_F(c.noise, tr.F), d, d0)


@functools.lru_cache(maxsize=None)
def truth(cid, jitter=0.0, jitter0=0.0):
    """The long-double truth of a case at the jitters the device's two fits ended with (0 for every case here)."""
    return solve_case(CASES[cid], problem(cid), jitter, jitter0, T)


@functools.lru_cache(maxsize=None)
def float64_restatement(cid, jitter=0.0, jitter0=0.0):
    """The same algorithm in plain float64."""
    return solve_case(CASES[cid], problem(cid), jitter, jitter0, np.float64)


def conditions(sv):
    """What a case must satisfy: (the share of the table's locations with NEI >= 1000 allowances, the same share over the gradient
    rows, (d - d0) / d0)."""
    c = sv.p.case
    ok = np.asarray(sv.truth.value, dtype=float) >= MARGIN_FACTOR * sv.allowance
    return float(np.mean(ok)), float(np.mean(ok[:c.Mr])), (sv.d - sv.d0) / sv.d0
