"""The exact GP of one ensemble member in ``np.longdouble`` (x87 80-bit, eps 1.1e-19), and the case table of
tests/test_gpu_ensemble_sizes.py and tests/test_ens_truth_host.py: the sizes at which the ensemble entry points (api_ens.hip,
ens_rows.hip) take another path.

The truth is built from tests/_sparse_ref.py (``LD.chol`` / ``LD.solve``, ``Kern``: ``k_of_r`` / ``dk_dr`` with their constants in
long double over direct-difference distances kept in long double).  For a member (family, ard, variance, lengthscale, noise, jitter):

* ``L = chol(K + (noise + 1e-8 + jitter) I)`` and ``alpha = L^-T L^-1 y`` -- the 1e-8 is exact_gaussian_inference.py:56, which the
  device (ky_diag, api_factor.hip) and the oracle (oracle/cpu_ref.py) add as well; the jitter is the rung the ladder ended on;
* at x: mean = k*^T alpha, variance = kss - |L^-1 k*|^2 (+ noise): noise alone, the jitter and the 1e-8 enter only through L, as in
  the code and in GPy;
* dmdx, dvdx with the convention of gp.py:432-453 and stationary.py:251-258 (inverse distance 0 at r = 0);
* fmin = min(K_f alpha) over the training inputs (gpmodel.py:125-129).

The integrated rule stays ``test_gpu_ensemble.integrated`` (acquisitions._Rule in NumPy), fed with these posteriors cast to float64
or with the float64 oracle's.  ``oracle64`` is that oracle: ``OracleGP`` over ``_kernel_families.make(..., direct=True)``.
Everything is cached per (family, case, member, jitter) and read-only.  Nothing here imports the library or needs a GPU.
"""
import collections
import functools

import numpy as np

from oracle import cpu_ref as O

import _family_shapes as FS
import _kernel_families as KF
import _sparse_ref as SR

LD = SR.LD
T = np.longdouble
CONST_DIAG = 1e-8               # exact_gaussian_inference.py:56

# ---- the case table ------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id N D fams ard S reaches")
TABLE = (
    Case("p", 770, 3, ("Mat32",), True, 3, "7 tiles: two factorisation panels, the second one tile wide; one column chunk"),
    Case("q", 1024, 2, ("rbf",), False, 3, "8 tiles: the last one-chunk size, no ragged tile, N a multiple of 64"),
    Case("r", 1025, 5, ("Exponential",), True, 3, "9 tiles: the second chunk holds one live column; nmean = 2; 127 padded rows"),
    Case("s", 2048, 3, ("Mat52",), False, 2, "the cap: 16 tiles, panels 6 + 6 + 4, a full second chunk"),
    Case("t", 130, 2, ("rbf",), True, 64, "GP_ENS_MAX_S members; two tiles, ragged"),
    Case("u", 300, 64, ("Mat32", "rbf"), True, 3, "two locations per pass at GP_MAX_D (the data of _family_shapes case g)"),
    Case("v", 160, 2, ("rbf",), False, 4, "120 + 40 duplicated rows: two members climb the jitter ladder next to two that do not"),
)
CASES = {c.id: c for c in TABLE}
TRUTH_CIDS = "pqrstu"           # v is compared in its own test, with the jitter the device reports
PAIRS = tuple((f, c.id) for c in TABLE if c.id in TRUTH_CIDS for f in c.fams)

GP_TILE, PANEL_TILES, RW_CW = 128, 6, 1024
ENS_MAX_S, ENS_MAX_NPAD, ENS_TABLE_CHUNK = 64, 2048, 512
ROWS_MAX_M, ROWS_MAX_XS, GP_MAX_D = 4, 128, 64


# ---- the code's size decisions, restated (tests/test_ens_truth_host.py asserts the table against them) -------------------------
def npad(N):
    return -(-N // GP_TILE) * GP_TILE


def tiles(N):
    return npad(N) // GP_TILE


def rw_nch(R):
    """rows_body.h: column chunks of RW_CW = 1024 that row block R meets."""
    return R // 8 + 1


def rw_decode(idx):
    """rows_body.h: tile index -> (row block, chunk); groups of 8 row blocks with g + 1 chunks each, 4 g (g + 1) tiles before group g."""
    g = 0
    while 4 * (g + 1) * (g + 2) <= idx:
        g += 1
    rem = idx - 4 * g * (g + 1)
    return 8 * g + rem // (g + 1), rem % (g + 1)


def rows_tiles(nt):
    """onerow.hip: the grid of the forward and the backward pass, in tiles."""
    return sum(rw_nch(R) for R in range(nt))


def panels(nt):
    """gp_ens_fit: W = min(panel_tiles, nt), nJ = ceil(nt / W); the widths of the nJ panels in tiles."""
    W = min(PANEL_TILES, nt)
    return [min(W, nt - j) for j in range(0, nt, W)]


def table_chunks(M):
    """ens_table_scores: chunk = min(512, M rounded up to a tile); (rows, padded rows) of every pass of the loop."""
    chunk = min(ENS_TABLE_CHUNK, npad(M))
    return [(min(chunk, M - m0), npad(min(chunk, M - m0))) for m0 in range(0, M, chunk)]


def pass_width(D):
    """ens_passes: locations per pass."""
    return min(ROWS_MAX_M, ROWS_MAX_XS // D)


# ---- data ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, Y, lengthscale) of a case, read-only, from a generator seeded by the case id -- the recipe of _family_shapes.problem:
    X = U(0, 1), Y = sin(3 sum x / sqrt D) + 0.1 eps, lengthscale U(0.4, 1.5) * 0.5 sqrt D per dimension (ARD) or 0.35 sqrt D.
    Case u takes the data of _family_shapes case g; case v repeats its first 40 of 120 rows (X and Y)."""
    c = CASES[cid]
    if cid == "u":
        X, Y, _, ls = FS.problem("g")
        return X, Y, ls
    rng = np.random.default_rng(7100 + ord(cid))
    n = 120 if cid == "v" else c.N
    X = rng.uniform(0, 1, (n, c.D))
    Y = (np.sin(3 * X.sum(1) / np.sqrt(c.D)) + 0.1 * rng.standard_normal(n))[:, None]
    if cid == "v":
        X, Y = np.vstack([X, X[:40]]), np.vstack([Y, Y[:40]])
    ls = rng.uniform(0.4, 1.5, c.D) * 0.5 * np.sqrt(c.D) if c.ard else np.array([ISO_LS.get(cid, 0.35) * np.sqrt(c.D)])
    for a in (X, Y, ls):
        a.setflags(write=False)
    assert X.shape == (c.N, c.D)
    return X, Y, ls


# Conditions on the inputs (tests/test_ens_truth_host.py: the float64 oracle stays within 1e-9 of the truth).  An RBF over 1024
# points of the unit square at 0.35 sqrt D and noise 2e-3 leaves the float64 oracle's dvdx 1.9e-7 off the truth (the terms of the
# sum cancel to 1e-6 of their size under cond(Ky) ~ 1e6): case q takes 0.1 sqrt D, and cases q and t five times the noise.
ISO_LS = {"q": 0.1}
NOISE_FACTOR = {"q": 5.0, "t": 5.0}


# case v: members 1 and 3 cannot be factored without the ladder (40 exactly repeated rows under a variance whose rounding, N eps
# variance, is far above noise + 1e-8; at 1e7 the float64 oracle still factors), members 0 and 2 can.  The first rung is
# 1e-6 (variance + noise + 1e-8): cond(Ky) ~ 1.6e8.  Their lengthscale is short: the first location lies on a repeated row, where
# the variance is 1e-6 of the prior's and dvdx cancels accordingly, and at 0.1 the float64 oracle's dvdx of that row alone is
# 7e-5 of its scale off the truth, past the 1e-6 the CPU test allows this case (3.5e-7 and 1.4e-7 at 0.03).
V_MEMBERS = (np.array([1.0, 1e8, 1.0, 1e9]), np.array([[0.3], [0.03], [0.3], [0.03]]), np.array([1e-2, 1e-12, 1e-3, 1e-12]))
V_ILL = (1, 3)


@functools.lru_cache(maxsize=None)
def members(cid):
    """(variance [S], lengthscale [S, nls], noise [S]), read-only: FS.members-style triples built from the case's lengthscale --
    the case's own parameters, a smoother and noisier member, a rougher and cleaner one; case t goes on with 61 more drawn
    log-uniformly between those three (variance 0.4 .. 2.5, lengthscale factor 0.6 .. 2.2, noise between the three members')."""
    c = CASES[cid]
    if cid == "v":
        out = tuple(np.array(a) for a in V_MEMBERS)
    else:
        ls = problem(cid)[2]
        var, fac, noise = np.array([FS.VAR, 0.4, 2.5]), np.array([1.0, 2.2, 0.6]), np.array([FS.NOISE, 3e-2, 2e-3])
        noise = noise * NOISE_FACTOR.get(cid, 1.0)
        if c.S > 3:
            rng = np.random.default_rng(7200 + ord(cid))
            def more(lo, hi):
                return np.exp(rng.uniform(np.log(lo), np.log(hi), c.S - 3))
            var, fac, noise = np.r_[var, more(0.4, 2.5)], np.r_[fac, more(0.6, 2.2)], np.r_[noise, more(noise.min(), noise.max())]
        out = var[:c.S].copy(), (fac[:c.S, None] * ls[None, :]).copy(), noise[:c.S].copy()
    for a in out:
        a.setflags(write=False)
    assert out[0].shape == (c.S,) and out[1].shape == (c.S, len(problem(cid)[2])) and out[2].shape == (c.S,)
    return out


@functools.lru_cache(maxsize=None)
def points(cid):
    """Eight locations, as test_gpu_ensemble.points: row 0 ON a training point, random ones, points next to training points, a
    diagonal."""
    c = CASES[cid]
    X = problem(cid)[0]
    rng = np.random.default_rng(7300 + ord(cid))
    pool = np.vstack([X[5:6], rng.uniform(-0.05, 1.05, (2, c.D)), X[:2] + 0.013, X[2:3] - 0.02,
                      np.array([0.31, 0.77])[:, None] * np.ones((1, c.D))])
    assert pool.shape == (8, c.D) and np.array_equal(pool[0], X[5])
    pool.setflags(write=False)
    return pool


@functools.lru_cache(maxsize=None)
def table(cid, M):
    """A candidate table of M rows: the eight points, then U(-0.05, 1.05)."""
    c = CASES[cid]
    rng = np.random.default_rng(7400 + ord(cid))
    tab = np.vstack([points(cid), rng.uniform(-0.05, 1.05, (1100, c.D))])[:M]
    assert tab.shape == (M, c.D)
    tab.setflags(write=False)
    return tab


# ---- the truth -----------------------------------------------------------------------------------------------------------------
class Member(object):
    """One member's exact posterior in long double."""

    def __init__(self, fam, ard, variance, lengthscale, noise, jitter, X, Y):
        self.kern = SR.Kern(fam, X.shape[1], variance, lengthscale, ard, LD)
        self.X, self.noise = X, T(float(noise))
        Kf = self.kern.K(X)
        Ky = Kf.copy()
        Ky[np.diag_indices_from(Ky)] += self.noise + T(CONST_DIAG) + T(float(jitter))
        self.L = LD.chol(Ky)[0]
        y = np.asarray(Y[:, 0], dtype=T)
        self.alpha = LD.solve(self.L, LD.solve(self.L, y, 0), 1)
        self.fmin = np.min(Kf @ self.alpha)

    def at(self, x, grads=True):
        """(mean [M], variance without noise [M], with noise [M], dmdx [M, D], dvdx [M, D]) in long double."""
        kx = self.kern.K(x, self.X)                                        # [M, N]
        w = LD.solve(self.L, kx.T, 0)                                      # L^-1 k*
        mean, var0 = kx @ self.alpha, self.kern.variance - np.sum(w * w, axis=0)
        if not grads:
            return mean, var0, var0 + self.noise
        beta = LD.solve(self.L, w, 1)                                      # Ky^-1 k*
        dm = self.kern.gradients_X(np.broadcast_to(self.alpha[None, :], kx.shape), x, self.X)
        dv = self.kern.gradients_X(-2 * beta.T, x, self.X)                 # gp.py:451-453 (gradients_X_diag is zero)
        return mean, var0, var0 + self.noise, dm, dv


def _params(cid, z):
    var, ls, noise = members(cid)
    return float(var[z]), ls[z], float(noise[z])


@functools.lru_cache(maxsize=None)
def member(fam, cid, z, jitter=0.0):
    c = CASES[cid]
    X, Y, _ = problem(cid)
    var, ls, noise = _params(cid, z)
    return Member(fam, c.ard, var, ls, noise, jitter, X, Y)


def _pack(mu, v0, v1, dm, dv, fmin, dtype):
    a = [np.array(v, dtype=dtype) for v in (mu, v0, v1, dm, dv)]
    return FS.freeze(FS.namespace(mu=a[0], var=(a[1], a[2]), dm=a[3], dv=a[4], fmin=dtype(fmin)))


@functools.lru_cache(maxsize=None)
def truth(fam, cid, z, jitter=0.0):
    """The member's posterior at the eight points and its fmin in long double: mu [8], var = (without, with noise), dm, dv [8, D]."""
    m = member(fam, cid, z, jitter)
    return _pack(*m.at(points(cid)), fmin=m.fmin, dtype=T)


@functools.lru_cache(maxsize=None)
def truth_table(fam, cid, z, M):
    """(mean, variance with noise) [M] at the case's M-row table, long double."""
    mu, _, v1 = member(fam, cid, z).at(table(cid, M), grads=False)
    mu.setflags(write=False)
    v1.setflags(write=False)
    return mu, v1


# ---- the float64 direct-distance oracle ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_gp(fam, cid, z, jitter=0.0):
    """``OracleGP`` over direct distances.  With a jitter, the matrix the ladder ended on is factored directly (noise + jitter on
    the diagonal: no rung is climbed again) and the predictive noise is added by hand (``oracle64``)."""
    c = CASES[cid]
    X, Y, _ = problem(cid)
    var, ls, noise = _params(cid, z)
    gp = O.OracleGP(X, Y, KF.make(fam, c.D, var, ls, c.ard, direct=True), noise + jitter)
    assert gp.posterior["jitter"] == 0.0
    return gp


def _oracle_at(gp, x, noise):
    mu, v0 = gp.predict_noiseless(x)
    dm, dv = gp.predictive_gradients(x)
    return mu[:, 0], v0[:, 0], v0[:, 0] + noise, dm[:, :, 0], dv


@functools.lru_cache(maxsize=None)
def oracle64(fam, cid, z, jitter=0.0):
    gp = oracle_gp(fam, cid, z, jitter)
    return _pack(*_oracle_at(gp, points(cid), _params(cid, z)[2]), fmin=float(gp.predict(gp.X)[0].min()), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def oracle64_table(fam, cid, z, M):
    mu, v0 = oracle_gp(fam, cid, z).predict_noiseless(table(cid, M))
    out = mu[:, 0].copy(), v0[:, 0] + _params(cid, z)[2]
    for a in out:
        a.setflags(write=False)
    return out


def as64(r):
    """A truth record cast to float64 (what ``integrated`` takes)."""
    return FS.namespace(mu=r.mu.astype(np.float64), var=tuple(v.astype(np.float64) for v in r.var), dm=r.dm.astype(np.float64),
                        dv=r.dv.astype(np.float64), fmin=float(r.fmin))


# ---- the bound -------------------------------------------------------------------------------------------------------------------
MULT, FLOOR = 64.0, 1e-13


def floor_n(N):
    """FLOOR_N = 1e-13 max(1, Npad / 384): the project's floor was measured at Npad <= 384; beyond, the contraction length grows
    linearly with Npad and so, at worst, does the rounding of a sum (derived, not measured)."""
    return FLOOR * max(1.0, npad(N) / 384.0)


def e64_of(oracle, true):
    """(e64, scale): the float64 oracle's largest error against the truth, and the truth's largest entry."""
    true = np.asarray(true, dtype=T)
    err = np.max(np.abs(np.asarray(oracle, dtype=T) - true))
    return float(err), max(float(np.max(np.abs(true))), 1e-300)
