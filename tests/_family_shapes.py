"""The case table of tests/test_gpu_family_shapes.py, tests/test_family_shapes_host.py and tools/family_shapes_instances.py: the
shapes at which the four covariance families reach every instance of the tile kernels.

kbuild_kernel / kbuild_batch_kernel / cross_k_kernel are compiled for DU in {8, 16, 0} (launch_kbuild, kbuild.hip: DU = 8 for
D <= 8, 16 for D <= 16, else 0: the run-time loop) and for the two family pairs FP (0: rbf / Mat52, 1: Mat32 / Exponential);
lml_grad_tile_kernel / lml_grad_tile_batch_kernel for the two pairs.  The ARD gradients walk the dimensions GP_GRAD_CH = 16 at a
time (lml_grad_passes, api_grad.hip; launch_predict_grad), launch_lml_grad splits a tile four ways below 256 lower tiles and not
at all from there on (grad.hip), and the one-location calls take the fused kernels while min(k, 4) * D <= ROWS_MAX_XS = 128 doubles
(rows_fused_ok, api_rows.hip).

An explicit table, every row with its reason; the data of a case is drawn from a generator seeded by the case id, so the three
users see the same numbers.  No GPU and no library is needed to import this module.
"""
import collections
import functools
import types

import numpy as np

from oracle import cpu_ref as O

import _kernel_families as KF

Case = collections.namedtuple("Case", "id N D M P ard off reaches")

TABLE = (
    Case("a", 1, 1, 1, 1, False, 0.0, "single point, one padded tile"),
    Case("b", 2, 9, 5, 1, True, 0.0, "DU = 16 lower edge, small-M route"),
    Case("c", 127, 8, 129, 1, True, 0.0, "DU = 8 upper edge, one row short of a tile, two candidate tiles"),
    Case("d", 128, 16, 5, 3, True, 0.0, "DU = 16 upper edge, one full gradient chunk, exact tile, P = 3"),
    Case("e", 129, 17, 129, 3, True, 0.0, "DU = 0, second chunk holds one dimension, one row past a tile, P = 3"),
    Case("f", 300, 33, 130, 1, True, 0.0, "three chunks; rows: M = 3 fused, M = 4 falls back"),
    Case("g", 300, 64, 2, 1, True, 0.0, "GP_MAX_D, four full chunks; rows: M = 2 fused (128 doubles), M = 3 falls back"),
    Case("h", 257, 32, 4, 1, False, 0.0, "iso with D > 16 (one pass, all dimensions in s); rows: M = 4 fused at exactly 128"),
    Case("i", 2944, 3, 64, 1, True, 0.0, "276 lower tiles: split = 1"),
    Case("j", 300, 3, 130, 1, True, 1000.0, "inputs away from the origin"),
)
CASES = {c.id: c for c in TABLE}

NEW_FAMILIES = ("Mat32", "Exponential")                       # family pair 1
ALL_FAMILIES = ("rbf", "Mat52") + NEW_FAMILIES
KERNEL_ID = {"rbf": 0, "Mat52": 1, "Mat32": 2, "Exponential": 3}   # GP_KERNEL_* of include/gphip.h
VAR, NOISE = 1.3, 1e-2

# which families run which rows: a-i the new families, j all four, e and g the old pair as well (the single-call references of
# the batched fit at D > 16).  Case i goes last per family: its references are the expensive ones.
_ROWS = {"rbf": "egj", "Mat52": "egj", "Mat32": "abcdefghji", "Exponential": "abcdefghji"}
SINGLE = tuple((fam, cid) for fam in ALL_FAMILIES for cid in _ROWS[fam])
# gp_fit_grad_batch at D > 8; c (D = 8) as well for the new families, so that the DU = 8 batch instance of pair 1 is launched here
# too, at the upper edge of its class
_BATCH_ROWS = {"rbf": "eg", "Mat52": "eg", "Mat32": "cbdefg", "Exponential": "cbdefg"}
BATCH = tuple((fam, cid) for fam in ALL_FAMILIES for cid in _BATCH_ROWS[fam])
# the emulated-fp64 repeats
EMULATED = (("Mat32", "c"), ("Mat32", "f"))


def du_class(D):
    """The DU template argument launch_kbuild / launch_cross_k pick (kbuild.hip)."""
    return 8 if D <= 8 else 16 if D <= 16 else 0


def grad_chunks(c):
    """Passes of lml_grad_passes (api_grad.hip): one per GP_GRAD_CH = 16 dimensions with ARD, one without."""
    return -(-c.D // 16) if c.ard else 1


def lower_tiles(N):
    """Tiles of the lower triangle, the grid of launch_lml_grad (grad.hip): split = 4 below 256 of them, 1 from there on."""
    nt = -(-N // 128)
    return nt * (nt + 1) // 2


def rows_fused(k, D, P=1):
    """rows_fused_ok (api_rows.hip) at the default small_m = 8: k <= 8, one output, min(k, ROWS_MAX_M = 4) * D <= ROWS_MAX_XS = 128."""
    return P == 1 and 1 <= k <= 8 and min(k, 4) * D <= 128


def rows_counts(c):
    """The row counts of the one-location calls of a case: 1, min(M, 3), min(M, 4), without repeats -- and M + 1 where the case
    has fewer than four candidates and that count is the first one past the limit (case g: 3 rows of 64 doubles)."""
    ks = {1, min(c.M, 3), min(c.M, 4)}
    if c.M < 4 and rows_fused(c.M, c.D, c.P) and not rows_fused(c.M + 1, c.D, c.P):
        ks.add(c.M + 1)
    return tuple(sorted(ks))


def rows_points(cid):
    """The locations of the one-location calls: the case's first candidates (row 0 ON a training point), and one more point
    next to a training point where rows_counts asks for more rows than the case has candidates."""
    c = CASES[cid]
    X, _, Xs, _ = problem(cid)
    k = max(rows_counts(c))
    return Xs[:k] if k <= c.M else np.vstack([Xs, X[:k - c.M] + 0.01])


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, Y, Xs, lengthscale) of a case, read-only.  X = off + U(0, 1), Y[:, p] = sin(3 (p + 1) sum(x - off) / sqrt D) + 0.1 eps,
    Xs = off + U(-0.05, 1.05) with Xs[0] = X[min(5, N - 1)] (a candidate ON a training point), lengthscale U(0.4, 1.5) * 0.5 sqrt D
    per dimension (ARD) or 0.35 sqrt D (iso)."""
    c = CASES[cid]
    rng = np.random.default_rng(7000 + ord(cid))
    X = c.off + rng.uniform(0, 1, (c.N, c.D))
    Y = np.stack([np.sin(3 * (p + 1) * (X - c.off).sum(1) / np.sqrt(c.D)) + 0.1 * rng.standard_normal(c.N) for p in range(c.P)], 1)
    Xs = c.off + rng.uniform(-0.05, 1.05, (c.M, c.D))
    Xs[0] = X[coincident_row(c)]
    ls = rng.uniform(0.4, 1.5, c.D) * 0.5 * np.sqrt(c.D) if c.ard else np.array([0.35 * np.sqrt(c.D)])
    for a in (X, Y, Xs, ls):
        a.setflags(write=False)
    return X, Y, Xs, ls


def coincident_row(c):
    return min(5, c.N - 1)


def members(cid):
    """The R = 3 members of the batched fit: the case's own parameters, a smoother and noisier one, a rougher and cleaner one."""
    ls = problem(cid)[3]
    return np.array([VAR, 0.4, 2.5]), np.array([ls, ls * 2.2, ls * 0.6]), np.array([NOISE, 3e-2, 2e-3])


def oracle(fam, cid, member=0, direct=True):
    """The oracle model of a case (or of a member of its batch), fitted once and shared by every test of a session."""
    return _oracle(fam, cid, int(member), bool(direct))


@functools.lru_cache(maxsize=None)
def _oracle(fam, cid, member, direct):
    c = CASES[cid]
    X, Y, _, _ = problem(cid)
    var, ls, noise = members(cid)
    return O.OracleGP(X, Y, KF.make(fam, c.D, var[member], ls[member], c.ard, direct=direct), noise[member])


def k_tolerance(cid):
    """The bound on |K - K_ref| / variance.  1e-13 is the project's own (tests/test_gpu_kernel_families.py).  The device divides
    every coordinate by its lengthscale and rounds it once (stage_rows_T, kbuild.hip): two roundings of 2^-53 max|x_d / l_d| per
    difference, so |dr| <= 2 sqrt(D) 2^-53 max|x_d / l_d| (|d r / d delta_d| <= 1, summed over D in the 2-norm), and
    |dk / dr| <= variance for all four families.  For inputs in the unit cube the term is below 1e-15 and is left out."""
    c = CASES[cid]
    if c.off == 0.0:
        return 1e-13
    X, _, Xs, ls = problem(cid)
    big = max(float(np.max(np.abs(X / ls))), float(np.max(np.abs(Xs / ls))))
    return 1e-13 + 2.0 * np.sqrt(c.D) * 2.0 ** -53 * big


def freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def namespace(**kw):
    return types.SimpleNamespace(**kw)
