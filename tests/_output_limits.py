"""The case table of tests/test_output_limits_host.py and tests/test_gpu_output_limits.py: fits at the limits of the output count
P and of the input dimension D.

gp_set_data takes 1 <= P <= GP_MAX_RHS = 128 and D <= GP_MAX_D = 64; the gradient entries P <= GP_GRAD_MAX_P = 16 (the sparse one
GP_SPARSE_GRAD_MAX_P = 16) -- and D and P JOINTLY, by the LDS of a workgroup (lml_grad_lds_bytes, csrc/grad.hip; the formulas are
restated below): on gfx950 (163840 bytes a workgroup) the fused gradient pass fits while D + P <= 79, for a Gower model while
2 D + P <= 79.  The `fits` column of the table is that arithmetic, not a measurement; tests/test_output_limits_host.py holds the
column to the formulas.

Targets: Y[:, p] = s_p (sin(w_p X a_p + phi_p) + 0.1 eps_p), s_p = 2^((p mod 7) - 3), with a frequency vector w_p a_p of its own
per column (targets() below) and phase and noise drawn from a generator seeded by the case id: the columns are linearly
independent and of different scale (1/8 ... 8), so that a swapped or mis-strided output index moves a result by far more than
any tolerance.  Every comparison is made per output column, relative to that column's own largest magnitude (col_err).

An explicit table, every row with its reason.  No GPU and no library is needed to import this module.
"""
import collections
import functools

import numpy as np

from oracle import cpu_ref as O

import _kernel_families as KF

VAR, NOISE = 1.3, 1e-2
# the fork's Gower K carries variance^D on its diagonal while Kdiag stays the variance: below 1 (0.95^39 = 0.135) the predictive
# variance variance - k^T Ky^-1 k stays positive, ON a training point too, and can be compared relatively
GOWER_VAR = 0.95
N, M_TILE, M_SMALL, M_GRAD = 130, 130, 3, 5      # two tiles, one ragged; the tile route, the small-M route, gp_predict_grad
KERNEL_ID = {"rbf": 0, "Mat52": 1, "Mat32": 2, "Exponential": 3}   # GP_KERNEL_* of include/gphip.h
ALL_FAMILIES = ("rbf", "Mat52", "Mat32", "Exponential")

# ---- the LDS arithmetic (csrc/grad.hip, gradx.hip, sparse.hip) ------------------------------------------------------------------
LDS_GFX950 = 163840              # bytes a workgroup can have on gfx950; the library asks the device (gp_create)
GRAD_CH, TILE = 16, 128


def lds_lml_grad(D, gower, P):
    """lml_grad_lds_bytes: red[4][GRAD_CH + 2] statically (576 B), then both input tiles (twice for Gower) and both alpha tiles."""
    return 8 * 4 * (GRAD_CH + 2) + ((4 if gower else 2) * D + 2 * P) * TILE * 8


def lds_gradx(D, P):
    """gradx_lds_bytes: row and column tile of the inputs and of alpha, at least the reduction's GX_H = 2 rows of 128."""
    return max((2 * D + 2 * P) * TILE * 8, 2 * TILE * 8)


def lds_sparse_grad(D, P):
    """sparse_grad_lds_bytes: the inducing tile, the column tile of the inputs and of the P targets, at least SP_NACC = 33 rows."""
    return max((2 * D + P) * TILE * 8, (1 + 2 * GRAD_CH) * TILE * 8)


# ---- the table ------------------------------------------------------------------------------------------------------------------
# grad: "yes" the gradient entries fit and are held to the oracle; "P" refused by P > 16; "lds" refused by the LDS check
Case = collections.namedtuple("Case", "id N D P gower grad fams why")

TABLE = (
    Case("P128", N, 3, 128, False, "P", ALL_FAMILIES, "GP_MAX_RHS: the RHS tile is full"),
    Case("P127", N, 3, 127, False, "P", ALL_FAMILIES, "one short of the full RHS tile: odd, the last row of the tile is padding"),
    Case("P17", N, 3, 17, False, "P", ALL_FAMILIES, "first P the gradient entries refuse"),
    Case("P16", N, 3, 16, False, "yes", ALL_FAMILIES, "GP_GRAD_MAX_P: every SCAL_DOT_GRAD slot in use"),
    Case("P4", N, 3, 4, False, "yes", ALL_FAMILIES, "a few outputs, past the suite's P = 3"),
    Case("LA", 300, 3, 128, False, "P", ("rbf",), "three tiles with the full RHS tile: the look-ahead scheduler against single-stream"),
    Case("D64P15", N, 64, 15, False, "yes", ("rbf", "Mat32"), "D + P = 79: the last plain shape that fits, at GP_MAX_D"),
    Case("D63P16", N, 63, 16, False, "yes", ("rbf", "Mat32"), "D + P = 79 at GP_GRAD_MAX_P"),
    Case("D64P16", N, 64, 16, False, "lds", ("rbf", "Mat32"), "D + P = 80: 164416 B, the first plain shape refused; gradx fits by zero bytes"),
    Case("G39P1", N, 39, 1, True, "yes", ("rbf",), "Gower, 2 D + P = 79: fits"),
    Case("G39P2", N, 39, 2, True, "lds", ("rbf",), "Gower, 2 D + P = 80: refused"),
    Case("G40P1", N, 40, 1, True, "lds", ("rbf",), "Gower, D = 40: refused with any P"),
)
CASES = {c.id: c for c in TABLE}
OUTPUT_IDS = ("P128", "P127", "P17", "P16", "P4")
BOUNDARY_FIT = ("D64P15", "D63P16", "G39P1")
BOUNDARY_REFUSED = ("D64P16", "G39P2", "G40P1")
PAIRS = tuple((f, c.id) for c in TABLE for f in c.fams)
P_REFUSED_BY_SET_DATA = 129

# sparse model: Mz = 130 inducing inputs (two tiles, one ragged) over N = 300
SparseCase = collections.namedtuple("SparseCase", "id N Mz D P grad fams why")
SPARSE = (
    SparseCase("S16", 300, 130, 3, 16, True, ("rbf", "Mat32"), "GP_SPARSE_GRAD_MAX_P: every cm[] register in use"),
    SparseCase("S17", 300, 130, 3, 17, False, ("rbf",), "the gradient is refused, fit and predict work"),
    SparseCase("S128", 300, 130, 3, 128, False, ("rbf",), "GP_MAX_RHS through sparse_thin / sparse_outer"),
)
SPARSE_CASES = {c.id: c for c in SPARSE}
SPARSE_PAIRS = tuple((f, c.id) for c in SPARSE for f in c.fams)
SPARSE_NOISE = NOISE             # (neither ladder steps at it: asserted on the CPU and on the device)
# emulate_fp64 = 1 at P = 16: the targets as they are, and scaled by 1e3
EMULATED = (("P16", 1.0), ("P16", 1e3))
APPEND_K = 3                     # gp_append: the P16 case's first 127 rows, then its last three (across the tile edge)


def fits(c):
    """What the arithmetic says about the gradient pass of a case on gfx950."""
    return c.P <= 16 and lds_lml_grad(c.D, c.gower, c.P) <= LDS_GFX950


def _seed(cid):
    return int.from_bytes(cid.encode(), "little") % (2 ** 31)


def scales(P):
    return 2.0 ** ((np.arange(P) % 7) - 3)


def targets(rng, X, P):
    """Y[:, p] = s_p (sin(w_p X a_p + phi_p) + 0.1 eps_p) with w_p a_p = k_p: in the first three dimensions the p-th point of the
    lattice 2 pi {0 .. 5}^3 without its origin (whole harmonics of the unit cube: orthogonal there, so no two columns are alike
    on a sample of it either), plus 0.5 N(0, 1) in every dimension, so that every input matters."""
    n, D = X.shape
    q = np.arange(1, P + 1)
    k = 0.5 * rng.standard_normal((D, P))
    k[:3] += 2 * np.pi * np.stack([q % 6, (q // 6) % 6, q // 36])
    phi = rng.uniform(0, 2 * np.pi, P)
    return scales(P) * (np.sin(X @ k + phi) + 0.1 * rng.standard_normal((n, P)))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def gower_setup(cid):
    """(is_discrete [D], ranges [D], domain) of a Gower case: the first two variables discrete on {0, 1, 2}, the others continuous
    on [0, range_d] with range_d in 1 ... 2."""
    c = CASES[cid]
    disc = np.zeros(c.D, dtype=np.int32)
    disc[:2] = 1
    ranges = np.linspace(1.0, 2.0, c.D)
    domain = [{"name": "x%d" % d, "type": "discrete", "domain": (0.0, 1.0, 2.0)} if disc[d] else
              {"name": "x%d" % d, "type": "continuous", "domain": (0.0, float(ranges[d]))} for d in range(c.D)]
    return disc, ranges, domain


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, Y, Xs [M_TILE, D], lengthscale [D]) of a case, read-only.  X = U(0, 1)^D (a Gower case: drawn from its domain), Xs =
    U(-0.05, 1.05)^D with Xs[0] ON a training point, ARD lengthscales U(0.4, 1.5) 0.5 sqrt D."""
    c = CASES[cid]
    rng = np.random.default_rng(_seed(cid))
    if c.gower:
        space = O.MixedSpace(gower_setup(cid)[2])
        X, Xs = space.draw(rng, c.N), space.draw(rng, M_TILE)
    else:
        X = rng.uniform(0, 1, (c.N, c.D))
        Xs = rng.uniform(-0.05, 1.05, (M_TILE, c.D))
    Xs[0] = X[5]
    Y = targets(rng, X, c.P)
    ls = rng.uniform(0.4, 1.5, c.D) * 0.5 * np.sqrt(c.D)
    return _freeze(X, Y, Xs, ls)


def kernel(fam, cid, variance=None, ls=None):
    c = CASES[cid]
    ls = problem(cid)[3] if ls is None else ls
    if c.gower:
        return O.make_kernel(fam, c.D, GOWER_VAR if variance is None else variance, ls, ARD=True, Gower=True,
                             space=O.MixedSpace(gower_setup(cid)[2]))
    return KF.make(fam, c.D, VAR if variance is None else variance, ls, True, direct=True)


def variance_of(cid):
    return GOWER_VAR if CASES[cid].gower else VAR


def members(cid):
    """The R = 3 members of gp_fit_grad_batch: the case's own parameters, a smoother and noisier one, a rougher and cleaner one."""
    ls, v = problem(cid)[3], variance_of(cid)
    return np.array([v, 0.4 * v, 1.2 * v]), np.array([ls, ls * 2.2, ls * 0.6]), np.array([NOISE, 3e-2, 2e-3])


@functools.lru_cache(maxsize=None)
def oracle(fam, cid, member=0, scale=1.0, rows=None):
    """The float64 oracle of a case (of a member of its batch; of its targets times `scale`; of its first `rows` rows), fitted once."""
    X, Y, _, _ = problem(cid)
    var, ls, noise = members(cid)
    n = X.shape[0] if rows is None else rows
    gp = O.OracleGP(X[:n], Y[:n] * scale, kernel(fam, cid, var[member], ls[member]), noise[member])
    gp.posterior
    return gp


@functools.lru_cache(maxsize=None)
def sparse_problem(cid):
    """(X, Y, Z, Xs [M_TILE, D], lengthscale [D]) of a sparse case: Z = 65 data rows and 65 data rows moved by 0.03 N(0, 1)."""
    c = SPARSE_CASES[cid]
    rng = np.random.default_rng(_seed(cid))
    X = rng.uniform(0, 1, (c.N, c.D))
    Z = X[rng.permutation(c.N)[:c.Mz]].copy()
    Z[c.Mz // 2:] += 0.03 * rng.standard_normal((c.Mz - c.Mz // 2, c.D))
    Xs = rng.uniform(0, 1, (M_TILE, c.D))
    Y = targets(rng, X, c.P)
    ls = np.linspace(0.15, 0.35, c.D) * np.sqrt(c.D / 3.0)       # tests/_sparse_ref.case_lengthscale
    return _freeze(X, Y, Z, Xs, ls)


def col_err(got, ref, axis=-1):
    """The per-column measure: max over the columns p (along `axis`) of max |got_p - ref_p| / max |ref_p|."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g, r = np.moveaxis(got, axis, -1), np.moveaxis(ref, axis, -1)
    P = r.shape[-1]
    g, r = g.reshape(-1, P), r.reshape(-1, P)
    top = np.max(np.abs(r), axis=0)
    assert np.all(top > 0)
    return float(np.max(np.max(np.abs(g - r), axis=0) / top))
