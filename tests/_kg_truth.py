"""The discrete knowledge gradient and its gradient in ``np.longdouble`` (x87 80-bit, eps 1.1e-19) from the raw data -- the
kernel build, Cholesky and substitutions of tests/_qei_truth.py, no inverse factor -- and the case table of tests/test_gpu_kg.py
and tests/test_kg_truth_host.py.  ``evaluate`` over a float64 fit is the same algorithm in plain float64: the yardstick of the
device's gradient error.  Nothing here imports the library or needs a GPU; everything is computed once per case and read-only.

    w = L^-1 k(X, x),  v = kss - |w|^2,  v' = max(y_std^2 v, 1e-10),  sd = sqrt(v' + y_std^2 noise)
    a_i = y_std mu(a_i),  b_i = y_std^2 (k(x, a_i) - V_A[i] . w) / sd   (i < A);     a_A = y_std mu(x),  b_A = v' / sd
    a* = min_i a_i (lowest index on a tie),  a~_i = a_i - a*
    KG(x) = -sum_i (a~_i p_i + b_i q_i),   p_i = Phi(hi_i) - Phi(lo_i),   q_i = phi(lo_i) - phi(hi_i)
    dKG/dx = ([j* = A] - p_A) y_std dmu(x)/dx - sum_i q_i db_i/dx     (include/gphip.h spells out db_i/dx)

The intervals [lo_i, hi_i] come from a SORTED HULL SWEEP (Frazier, Powell & Dayanik 2009, Algorithm 1): the lines in order of
falling slope, equal slopes reduced to the lowest intercept (the lowest index among identical lines), then one pass with a stack.
The device works in interval form (every line against every other line), so the two share nothing but the definition.  Phi
differences are taken with mpmath at 40 digits.

The cases: N 130 / 300 / 1100 (two 128-row blocks, three, two 1024-column chunks), A 1 / 2 / 63 / 65 / 256 (one wave's edge
either side, the limit), table M 1 / 33 / 300, rows M 1 / 4 / 8 (the three pass layouts), all four families, ARD and not, noise
1e-2 and 1e-6.  Every case must have at least half its locations with KG >= 1000 value allowances, and in gradient cases a gap of
1000 allowances between the two lowest intercepts whenever x's own line is one of them (the gradient has a kink there):
``conditions`` computes what tests/test_kg_truth_host.py asserts.  The seeds below were chosen on the CPU under these conditions.
"""
import collections
import functools

import mpmath
import numpy as np

from _qei_truth import (FAMILY_ID, T, VARIANCE, Y_MEAN, Y_STD, _scaled_diff, dk_dr_over_r, fit, k_of_r, rel_tol, response,      # noqa: F401
                        sigma2, solve, tolerances)

MARGIN_FACTOR = 1000.0
FLOOR = 1e-10

# Mt: rows of the table; Mr: its leading rows also go through gp_kg_rows with gradients
Case = collections.namedtuple("Case", "id N D A Mt Mr fam ard noise seed ls_scale spread y_std")
TABLE = (
    Case("a", 130, 2, 1, 1, 1, "rbf", False, 1e-2, 0, 0.06, 0.05, Y_STD),             # A = 1: the two-line closed form; one row, one location
    Case("b", 300, 3, 2, 33, 4, "Mat52", True, 1e-2, 0, 0.3, 0.05, Y_STD),            # three row blocks, the narrow pass
    Case("c", 300, 16, 63, 33, 8, "rbf", True, 1e-2, 0, 0.1, 0.05, Y_STD),            # M D = 128, the limit of the wide pass; one wave less one
    Case("d", 1100, 4, 65, 300, 8, "Mat32", False, 1e-6, 0, 0.1, 0.05, Y_STD),        # two column chunks; a location ON a training input: the floor
    Case("e", 300, 3, 256, 33, 4, "Exponential", False, 1e-2, 0, 0.3, 0.05, Y_STD),   # the limit of A; a point twice in X_A; a location ON a point
    Case("f", 130, 2, 65, 33, 8, "rbf", False, 1e-6, 0, 0.03, 0.15, Y_STD),           # exact_feval's noise on the smallest matrix, the wide pass
    # a location ON a training input at noise 1e-6 under a small output scale: y_std^2 v ~ 1e-12, the floor of 1e-10 holds there
    # (at y_std = 1.7 the latent variance on a training input, about the noise, stays far above the floor: case d has that location).
    # With no variance left every slope is ~ 0: KG and its gradient are 0 there, which the floor's branch must reproduce, not NaN.
    Case("g", 130, 2, 2, 33, 4, "Mat52", False, 1e-6, 0, 0.03, 0.15, 1e-3),
)
CASES = {c.id: c for c in TABLE}
Problem = collections.namedtuple("Problem", "case X Y ls ls_arg Xa Xs")


@functools.lru_cache(maxsize=None)
def problem(cid):
    c = CASES[cid]
    rng = np.random.default_rng(7000 + ord(cid))
    X = rng.uniform(0, 1, (c.N, c.D))
    Y = (response(X) + 0.1 * rng.standard_normal(c.N))[:, None]
    Y = (Y - Y.mean()) / Y.std()
    base = c.ls_scale * np.sqrt(c.D)
    ls_arg = base * rng.uniform(0.7, 1.4, c.D) if c.ard else np.array([base])
    ls = ls_arg if c.ard else np.repeat(ls_arg, c.D)
    rng = np.random.default_rng(7100 + 131 * ord(cid) + c.seed)
    # Points and locations crowd the low region of the data -- the best observations, perturbed -- so that many intercepts lie
    # within a few slopes of the lowest and KG is substantial (uniform draws over a well-observed model give KG ~ 1e-14)
    low = np.argsort(Y[:, 0], kind="stable")[:16]
    Xa = np.clip(X[low[np.arange(c.A) % 16]] + 0.5 * c.spread * rng.standard_normal((c.A, c.D)), 0, 1)
    Xa[0] = X[low[0]]                             # the best observation itself, as AcquisitionKG keeps it in the set
    Xs = np.clip(X[low[np.arange(c.Mt) % 16]] + c.spread * rng.standard_normal((c.Mt, c.D)), 0, 1)
    if cid in "dg":
        Xs[2] = X[17]                             # on a training input at noise 1e-6 (g: the variance's floor holds)
    if cid == "e":
        Xa[200] = Xa[5]                           # the same point twice: the tie rule
        Xs[10] = Xa[9]                            # on a discretisation point: two nearly identical lines (beyond the gradient
                                                  # rows: min over two coincident lines has a kink in x there)
    for a in (X, Y, ls_arg, ls, Xa, Xs):
        a.setflags(write=False)
    return Problem(c, X, Y, ls, ls_arg, Xa, Xs)


# ---- the envelope ------------------------------------------------------------------------------------------------------------------
def hull(a, b):
    """The lower envelope of the lines a_i + b_i z by the sorted sweep: (lo [n], hi [n]) in the lines' dtype, lo = hi = 0 for lines
    that own no interval."""
    n = a.size
    order = sorted(range(n), key=lambda i: (-b[i], a[i], i))      # falling slope; among equal slopes the lowest, then the first
    keep = [order[0]]
    for i in order[1:]:
        if b[i] != b[keep[-1]]:
            keep.append(i)
    t = a.dtype.type
    stack, start = [], []
    for i in keep:
        while stack:
            j = stack[-1]
            z = (a[i] - a[j]) / (b[j] - b[i])      # right of z the flatter line i lies below j
            if z <= start[-1]:
                stack.pop()
                start.pop()
                continue
            break
        if stack:
            start.append(z)
        else:
            start.append(t(-np.inf))
        stack.append(i)
    lo, hi = np.zeros(n, dtype=a.dtype), np.zeros(n, dtype=a.dtype)
    for s, i in enumerate(stack):
        lo[i] = start[s]
        hi[i] = start[s + 1] if s + 1 < len(stack) else t(np.inf)
    return lo, hi


def _mp(x):
    x = T(x)
    if np.isinf(x):
        return mpmath.inf if x > 0 else -mpmath.inf
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - T(hi)))


def _back(x, t):
    x = mpmath.mpf(x)
    hi = float(x)
    return t(hi) + t(float(x - mpmath.mpf(hi)))


def masses(lo, hi):
    """p_i = Phi(hi_i) - Phi(lo_i) and q_i = phi(lo_i) - phi(hi_i), formed at 40 digits and rounded to the intervals' dtype."""
    t = lo.dtype.type
    p, q = np.zeros_like(lo), np.zeros_like(lo)
    with mpmath.workdps(40):
        for i in range(lo.size):
            if not lo[i] < hi[i]:
                continue
            l, h = _mp(lo[i]), _mp(hi[i])
            p[i] = _back(mpmath.ncdf(h) - mpmath.ncdf(l), t)
            q[i] = _back(mpmath.npdf(l) - mpmath.npdf(h), t)
    return p, q


Truth = collections.namedtuple("Truth", "mu value grad atil b p q jstar sd mean_norm floored gap")


def evaluate(fam, variance, noise, f, Xa, Xs, ngrad=0, y_mean=Y_MEAN, y_std=Y_STD):
    """KG of every row of Xs over the points Xa, and the gradient of the leading ``ngrad`` rows, in the arithmetic of the fit
    ``f``: a ``Truth`` (mu: the points' un-normalised means; per row: the value, a~ [A + 1], b, p, q, j*, sd; gap: the difference
    between the two lowest intercepts)."""
    t = f.X.dtype.type
    Xa, Xs = np.asarray(Xa, dtype=t), np.asarray(Xs, dtype=t)
    A, M, D = Xa.shape[0], Xs.shape[0], Xs.shape[1]
    ys, ys2 = t(y_std), t(y_std) ** 2
    _, rA = _scaled_diff(Xa, f.X, f.ls)
    kA = k_of_r(fam, t(variance), rA)                                   # [A, N]
    VA = solve(f.L, kA.T, 0)                                            # [N, A]
    muA = kA @ f.alpha
    dX, rX = _scaled_diff(Xs, f.X, f.ls)
    kX = k_of_r(fam, t(variance), rX)                                   # [M, N]
    W = solve(f.L, kX.T, 0)                                             # [N, M]
    mux = kX @ f.alpha
    dXA, rXA = _scaled_diff(Xs, Xa, f.ls)
    kXA = k_of_r(fam, t(variance), rXA)                                 # [M, A]
    Cov = kXA - W.T @ VA                                                # [M, A]
    v = t(variance) - (W * W).sum(0)
    if ngrad:
        BA = solve(f.L, VA, 1)                                          # [N, A]
        BX = solve(f.L, W[:, :ngrad], 1)                                # [N, ngrad]
        gX = dk_dr_over_r(fam, t(variance), rX[:ngrad])                 # [ngrad, N]
        gXA = dk_dr_over_r(fam, t(variance), rXA[:ngrad])               # [ngrad, A]
    value, grad = np.zeros(M, dtype=t), np.zeros((ngrad, D), dtype=t)
    atil, b = np.zeros((M, A + 1), dtype=t), np.zeros((M, A + 1), dtype=t)
    p, q = np.zeros((M, A + 1), dtype=t), np.zeros((M, A + 1), dtype=t)
    jstar, sds, floored, gap = np.zeros(M, dtype=int), np.zeros(M, dtype=t), np.zeros(M, dtype=bool), np.zeros(M, dtype=t)
    for m in range(M):
        vf = ys2 * v[m]
        floored[m] = not vf > t(FLOOR)
        vf = max(vf, t(FLOOR))
        sd = np.sqrt(vf + ys2 * t(noise))
        a = np.concatenate([ys * muA, [ys * mux[m]]])
        bm = np.concatenate([ys2 * Cov[m] / sd, [vf / sd]])
        js = int(np.argmin(a))                                          # the first of the minima
        at = a - a[js]
        lo, hi = hull(at, bm)
        pm, qm = masses(lo, hi)
        value[m] = -(at @ pm + bm @ qm)
        atil[m], b[m], p[m], q[m], jstar[m], sds[m] = at, bm, pm, qm, js, sd
        srt = np.sort(at)
        gap[m] = srt[1] - srt[0]
        if m < ngrad:
            J = gX[m][:, None] * dX[m] / f.ls                           # [N, D]: d k(X, x) / dx
            JA = gXA[m][:, None] * dXA[m] / f.ls                        # [A, D]: d k(x, a_i) / dx
            dv = t(0) * J[0] if floored[m] else -2 * ys2 * (J.T @ BX[:, m])
            dsd = dv / (2 * sd)
            db = ys2 * (JA - (J.T @ BA).T) / sd - bm[:A, None] * dsd[None, :] / sd          # [A, D]
            dbA = dv / sd - bm[A] * dsd / sd
            grad[m] = ((1.0 if js == A else 0.0) - pm[A]) * ys * (J.T @ f.alpha) - qm[:A] @ db - qm[A] * dbA
    mean_norm = float(max(np.max(np.abs(muA)), np.max(np.abs(mux))))
    return Truth(ys * muA + t(y_mean), value, grad, atil, b, p, q, jstar, sds, mean_norm, floored, gap)


def value_allowance(noise, tr, variance=VARIANCE, y_std=Y_STD):
    """Per location, first order from the truth's adjoint: (1 + |[j* = A] - p_A|) tol_m + sum_i |q_i| tol_b_i + 64 eps (max a~ +
    max |b|).  tol_m and the covariance's tol_S are _qei_truth.tolerances' (tests/test_gpu_rows.py's relative ones carried through
    the normaliser); a slope is a covariance over sd, and sd moves with the variance: tol_b_i = (tol_S / sd) (1 + |b_i| / (2 sd))."""
    tol_m, tol_S = tolerances(noise, tr.mean_norm, variance, y_std)
    A = tr.p.shape[1] - 1
    sd = np.asarray(tr.sd, dtype=float)
    own = np.abs((tr.jstar == A).astype(float) - np.asarray(tr.p[:, A], dtype=float))
    absb = np.abs(np.asarray(tr.b, dtype=float))
    tol_b = (tol_S / sd)[:, None] * (1.0 + absb / (2.0 * sd[:, None]))
    rounding = 64 * np.finfo(np.float64).eps * (np.asarray(tr.atil, dtype=float).max(1) + absb.max(1))
    return (1.0 + own) * tol_m + (np.abs(np.asarray(tr.q, dtype=float)) * tol_b).sum(1) + rounding


Solved = collections.namedtuple("Solved", "p fit truth allowance")


def solve_case(c, p, jitter=0.0, dtype=T):
    f = fit(c.fam, VARIANCE, p.ls, sigma2(c.noise, jitter), p.X, p.Y, dtype)
    tr = evaluate(c.fam, VARIANCE, c.noise, f, p.Xa, p.Xs, c.Mr, y_std=c.y_std)
    for a in tr:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    allow = value_allowance(c.noise, tr, y_std=c.y_std)
    allow.setflags(write=False)
    return Solved(p, f, tr, allow)


@functools.lru_cache(maxsize=None)
def truth(cid, jitter=0.0):
    """The long-double truth of a case at the jitter the device's fit ended with (0 for every case here)."""
    return solve_case(CASES[cid], problem(cid), jitter, T)


@functools.lru_cache(maxsize=None)
def float64_restatement(cid, jitter=0.0):
    """The same algorithm in plain float64."""
    return solve_case(CASES[cid], problem(cid), jitter, np.float64)


def conditions(sv):
    """What a case must satisfy: (the share of locations with KG >= 1000 allowances, the smallest gap / allowance over the gradient
    rows where x's own line is one of the two lowest -- inf where there is none)."""
    tr, c = sv.truth, sv.p.case
    share = float(np.mean(np.asarray(tr.value, dtype=float) >= MARGIN_FACTOR * sv.allowance))
    worst = np.inf
    for m in range(c.Mr):
        order = np.argsort(np.asarray(tr.atil[m], dtype=float), kind="stable")[:2]
        if c.A in order:
            worst = min(worst, float(tr.gap[m]) / sv.allowance[m])
    return share, worst


def two_line_closed_form(atil, b):
    """A = 1: -E[min(a~_0 + b_0 Z, a~_1 + b_1 Z)] = |d| phi(c / |d|) - c Phi(-c / |d|) with c = |a~_0 - a~_1| (one of them is 0)
    and d = b_0 - b_1, in long double through mpmath."""
    c, d = abs(T(atil[0]) - T(atil[1])), abs(T(b[0]) - T(b[1]))
    if d == 0:
        return T(0)
    with mpmath.workdps(40):
        u = _mp(c) / _mp(d)
        return _back(_mp(d) * mpmath.npdf(u) - _mp(c) * mpmath.ncdf(-u), T)
