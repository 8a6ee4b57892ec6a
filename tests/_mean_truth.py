"""The exact GP with an affine mean function m(x) = x^T A + b in ``np.longdouble`` (x87 80-bit, eps 1.1e-19), the float64
references it is held against, and the case table of tests/test_gpu_mean_function.py and tests/test_mean_truth_host.py.

Built on tests/_sparse_ref.py (``LD.chol`` / ``LD.solve``, ``Kern`` over direct-difference distances kept in long double), as
tests/_ens_truth.py is.  For a case (family, ard, variance, lengthscale, noise; A [D, P] and / or b [P]), with R = Y - X A - 1 b^T
(core/gp.py:267, exact_gaussian_inference.py:42-50: YYT_factor = Y - m):

* L = chol(K + (noise + 1e-8) I), alpha = L^-T L^-1 R,  lml = -(N P log 2 pi + P log det + sum alpha o R) / 2;
* dL_dK = (alpha alpha^T - P Ky^-1) / 2 through ``update_gradients_full``; dnoise = trace dL_dK;
* dA = X^T alpha, dB = 1^T alpha (dL_dm = alpha through Linear / Constant.update_gradients, linear.py:35-36);
* at x: mean = k*^T alpha + m(x), var = kss - |L^-1 k*|^2 (+ noise), dmdx = gradients_X(alpha^T) + A, dvdx = gradients_X(-2 beta^T);
* fmin = min_i (K alpha + m(X))_i.

Two float64 references: ``closed64`` is the same formulas in float64 (``_sparse_ref.F64``); ``oracle64`` is the pinned oracle used
as it is -- ``OracleGP`` over direct distances on the targets Y - m(X), plus m(x*) and A on the way out.  The bound of a GPU
comparison is tests/test_gpu_ensemble_sizes.py's: err <= max(MULT x e64, FLOOR_N x scale) with MULT = 64, FLOOR = 1e-13
(``_ens_truth``), e64 the oracle's own error against the truth.  The scores are the oracle's NumPy rules (``acq_EI`` ...) over a
stand-in model that serves a given posterior (``PosteriorModel``).  Cached per case, read-only; nothing here needs a GPU.
"""
import collections
import functools

import numpy as np

from oracle import cpu_ref as O

import _ens_truth as ET
import _family_shapes as FS
import _kernel_families as KF
import _sparse_ref as SR

LD, F64 = SR.LD, SR.F64
T = np.longdouble
CONST_DIAG = 1e-8               # exact_gaussian_inference.py:56
VAR, NOISE = 1.3, 1e-2
MEAN_GRAD_CH = 256              # csrc/gphip_internal.h: rows per first-level partial of gp_mean_grad
MULT, floor_n, e64_of = ET.MULT, ET.floor_n, ET.e64_of

# N 1, 127, 128, 129, 257 (one point; either side of one tile; a third tile) and 255, 256 (with 257: either side of the chunk of
# gp_mean_grad); D 1, 3, 64 = GP_MAX_D (two locations per fused pass); P 1, 3, 16 (D + P <= 79: the gradient pass's LDS, so P = 16
# goes with D = 3); A alone, b alone, both; all four families, ARD and not.
Case = collections.namedtuple("Case", "id N D P fam ard parts")
TABLE = (
    Case("a", 1, 1, 1, "rbf", False, "Ab"),
    Case("b", 127, 3, 1, "Mat52", True, "A"),
    Case("c", 128, 3, 3, "rbf", False, "b"),
    Case("d", 129, 3, 1, "Mat32", False, "Ab"),
    Case("e", 257, 3, 16, "rbf", True, "Ab"),
    Case("f", 256, 1, 1, "Exponential", False, "Ab"),
    Case("g", 255, 64, 1, "rbf", True, "Ab"),
    Case("h", 257, 64, 3, "Mat52", False, "A"),
)
CASES = {c.id: c for c in TABLE}
SINGLE = tuple(c.id for c in TABLE if c.P == 1)       # the cases the rows and acquisition entries take
TABLE_MS = (9, 130, 300)

Problem = collections.namedtuple("Problem", "case X Y ls A b")


@functools.lru_cache(maxsize=None)
def problem(cid):
    """X = U(0, 1); Y = a smooth bump per output + a planted trend X A0 + b0 + 0.1 eps; the model's A, b are the planted ones moved
    by a fifth, so that the residuals keep a trend of their own; lengthscales as tests/_ens_truth.py draws them."""
    c = CASES[cid]
    rng = np.random.default_rng(9100 + ord(cid))
    X = rng.uniform(0, 1, (c.N, c.D))
    A0, b0 = rng.standard_normal((c.D, c.P)) / np.sqrt(c.D), rng.standard_normal(c.P)
    bump = np.sin(3 * X.sum(1) / np.sqrt(c.D))[:, None] * (1 + 0.1 * np.arange(c.P))[None, :]
    Y = bump + X @ A0 + b0 + 0.1 * rng.standard_normal((c.N, c.P))
    ls = rng.uniform(0.4, 1.5, c.D) * 0.5 * np.sqrt(c.D) if c.ard else np.array([0.35 * np.sqrt(c.D)])
    A = A0 * (1 + 0.2 * rng.standard_normal((c.D, c.P))) if "A" in c.parts else None
    b = b0 * (1 + 0.2 * rng.standard_normal(c.P)) if "b" in c.parts else None
    for a in (X, Y, ls, A, b):
        if a is not None:
            a.setflags(write=False)
    return Problem(c, X, Y, ls, A, b)


@functools.lru_cache(maxsize=None)
def points(cid):
    """Eight locations: row 0 ON a training point, two in and around the box, three next to training points (or the box's centre
    where there is only one), two on the diagonal -- one of them three box widths outside."""
    c = CASES[cid]
    X = problem(cid).X
    rng = np.random.default_rng(9200 + ord(cid))
    near = X[:3] if c.N >= 3 else np.full((3, c.D), 0.5)
    pool = np.vstack([X[min(5, c.N - 1)][None, :], rng.uniform(-0.05, 1.05, (2, c.D)), near[:2] + 0.013, near[2:3] - 0.02,
                      np.array([0.31, 3.0])[:, None] * np.ones((1, c.D))])
    assert pool.shape == (8, c.D)
    pool.setflags(write=False)
    return pool


@functools.lru_cache(maxsize=None)
def table(cid, M):
    """A candidate table of M rows: the eight points, then U(-0.3, 1.3)."""
    c = CASES[cid]
    rng = np.random.default_rng(9300 + ord(cid))
    tab = np.vstack([points(cid), rng.uniform(-0.3, 1.3, (max(TABLE_MS), c.D))])[:M]
    tab.setflags(write=False)
    return tab


def mean_of(A, b, x, dtype=T):
    """m(x) [M, P] in ``dtype`` for A [D, P] or None and b [P] or None."""
    x = np.asarray(x, dtype=dtype)
    P = (A.shape[1] if A is not None else len(b))
    m = np.zeros((x.shape[0], P), dtype=dtype)
    if A is not None:
        m = m + x @ np.asarray(A, dtype=dtype)
    if b is not None:
        m = m + np.asarray(b, dtype=dtype)[None, :]
    return m


# ---- the exact GP with a mean, in the arithmetic ``lin`` ------------------------------------------------------------------------------
class MeanGP(object):
    def __init__(self, fam, ard, variance, lengthscale, noise, X, Y, A, b, lin=LD):
        t = lin.dtype
        self.lin, self.X, self.A, self.b = lin, X, A, b
        self.kern = SR.Kern(fam, X.shape[1], variance, lengthscale, ard, lin)
        self.noise = t(float(noise))
        N, P = Y.shape
        self.Kf = self.kern.K(X)
        Ky = self.Kf.copy()
        Ky[np.diag_indices_from(Ky)] += self.noise + t(CONST_DIAG)
        self.L = lin.chol(Ky)[0]
        self.mX = mean_of(A, b, X, t) if (A is not None or b is not None) else np.zeros((N, P), dtype=t)
        self.R = np.asarray(Y, dtype=t) - self.mX
        self.alpha = lin.solve(self.L, lin.solve(self.L, self.R, 0), 1)                        # [N, P]
        self.logdet = 2 * np.sum(np.log(np.diag(self.L)))
        self.lml = -(N * P * np.log(2 * t(np.pi)) + P * self.logdet + np.sum(self.alpha * self.R)) / 2

    def gradients(self):
        """(dvariance, dlengthscale [1 or D], dnoise, dA [D, P], db [P])."""
        N, P = self.R.shape
        t = self.lin.dtype
        Ki = self.lin.solve(self.L, self.lin.solve(self.L, np.eye(N, dtype=t), 0), 1)
        dL_dK = (self.alpha @ self.alpha.T - P * Ki) / 2
        dvar, dls = self.kern.update_gradients_full(dL_dK, self.X)
        return dvar, dls, np.trace(dL_dK), np.asarray(self.X, dtype=t).T @ self.alpha, self.alpha.sum(0)

    def train_mean(self):
        return self.Kf @ self.alpha + self.mX

    def at(self, x):
        """(mean [M, P], variance without noise [M], with noise [M], dmdx [M, D, P], dvdx [M, D])."""
        t = self.lin.dtype
        kx = self.kern.K(x, self.X)
        w = self.lin.solve(self.L, kx.T, 0)
        P = self.R.shape[1]
        mean = kx @ self.alpha + (mean_of(self.A, self.b, x, t) if (self.A is not None or self.b is not None) else 0)
        var0 = self.kern.variance - np.sum(w * w, axis=0)
        beta = self.lin.solve(self.L, w, 1)
        dm = np.stack([self.kern.gradients_X(np.broadcast_to(self.alpha[None, :, p], kx.shape), x, self.X) for p in range(P)], axis=2)
        if self.A is not None:
            dm = dm + np.asarray(self.A, dtype=t)[None, :, :]
        dv = self.kern.gradients_X(-2 * beta.T, x, self.X)
        return mean, var0, var0 + self.noise, dm, dv


def _record(gp, xs, dtype):
    dvar, dls, dn, dA, db = gp.gradients()
    mu, v0, v1, dm, dv = gp.at(xs)
    a = lambda v: np.array(v, dtype=dtype)   # noqa: E731
    return FS.freeze(FS.namespace(lml=dtype(gp.lml), logdet=dtype(gp.logdet), alpha=a(gp.alpha), dvar=dtype(dvar), dls=a(dls),
                                  dnoise=dtype(dn), dA=a(dA), db=a(db), mu=a(mu), var=(a(v0), a(v1)), dm=a(dm), dv=a(dv),
                                  train_mean=a(gp.train_mean())))


@functools.lru_cache(maxsize=None)
def model(cid, lin=LD):
    p = problem(cid)
    return MeanGP(p.case.fam, p.case.ard, VAR, p.ls, NOISE, p.X, p.Y, p.A, p.b, lin)


@functools.lru_cache(maxsize=None)
def truth(cid):
    """Fit, gradients and the posterior at the eight points in long double."""
    return _record(model(cid), points(cid), T)


@functools.lru_cache(maxsize=None)
def closed64(cid):
    """The same formulas in float64."""
    return _record(model(cid, F64), points(cid), np.float64)


@functools.lru_cache(maxsize=None)
def truth_table(cid, M):
    out = model(cid).at(table(cid, M))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the pinned oracle, as it is, on the targets Y - m(X) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_gp(cid):
    p = problem(cid)
    c = p.case
    resid = p.Y - mean_of(p.A, p.b, p.X, np.float64)
    gp = O.OracleGP(p.X, resid, KF.make(c.fam, c.D, VAR, p.ls, c.ard, direct=True), NOISE)
    assert gp.posterior["jitter"] == 0.0
    return gp


def _oracle_at(cid, x):
    p = problem(cid)
    gp = oracle_gp(cid)
    mu, v0 = gp.predict_noiseless(x)
    dm, dv = gp.predictive_gradients(x)
    mu = mu + mean_of(p.A, p.b, x, np.float64)
    if p.A is not None:
        dm = dm + p.A[None, :, :]
    return mu, v0[:, 0], v0[:, 0] + NOISE, dm, dv


@functools.lru_cache(maxsize=None)
def oracle64(cid):
    p = problem(cid)
    gp = oracle_gp(cid)
    post = gp.posterior
    dvar, dls, dn = gp.gradients()
    mu, v0, v1, dm, dv = _oracle_at(cid, points(cid))
    train = gp.predict_noiseless(p.X)[0] + mean_of(p.A, p.b, p.X, np.float64)
    return FS.freeze(FS.namespace(lml=post["lml"], logdet=post["logdet"], alpha=post["alpha"].copy(), dvar=float(dvar),
                                  dls=np.atleast_1d(np.asarray(dls, dtype=float)).copy(), dnoise=float(dn),
                                  dA=p.X.T @ post["alpha"], db=post["alpha"].sum(0), mu=mu, var=(v0, v1), dm=dm, dv=dv,
                                  train_mean=train))


@functools.lru_cache(maxsize=None)
def oracle64_table(cid, M):
    out = _oracle_at(cid, table(cid, M))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the scores: the oracle's NumPy rules over a posterior that is given -----------------------------------------------------------
class PosteriorModel(object):
    """The model the oracle's acquisition rules ask (``OracleGPModel``'s methods), serving ONE posterior: mean [M], variance with
    noise [M], dmdx [M, D], dvdx [M, D] and fmin, whatever ``x``."""

    def __init__(self, mu, var, dm, dv, fmin):
        f = lambda v: np.asarray(v, dtype=np.float64)   # noqa: E731
        self.mu, self.v, self.dm, self.dv, self.fmin = f(mu).reshape(-1, 1), np.clip(f(var).reshape(-1, 1), 1e-10, np.inf), f(dm), f(dv), float(fmin)

    def predict(self, x, with_noise=True):
        return self.mu, np.sqrt(self.v)

    def get_fmin(self):
        return self.fmin

    def predict_withGradients(self, x):
        s = np.sqrt(self.v)
        return self.mu, s, self.dm, self.dv / (2 * s)


RULES = {"EI": (O.acq_EI_withGradients, 0.01), "LCB": (O.acq_LCB_withGradients, 2.0), "MPI": (O.acq_MPI_withGradients, 0.01)}


def scores(name, mu, var, dm, dv, fmin):
    """(negated value [M], its x-gradient [M, D]) of EI / LCB / MPI by the oracle's rule on the given posterior: what the device's
    scoring entries return."""
    rule, par = RULES[name]
    pm = PosteriorModel(mu, var, dm, dv, fmin)
    f, df = rule(pm, None, par) if name == "LCB" else rule(pm, None, par, fmin=pm.fmin)
    return -np.asarray(f, dtype=float)[:, 0], -np.asarray(df, dtype=float)


def npad(N):
    return ET.npad(N)
