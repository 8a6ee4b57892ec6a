"""The case table of tests/test_jitter_cases_host.py and tests/test_gpu_jitter_routes.py: inputs on which the jitter ladder
(fit_impl / ladder_step, csrc/api_factor.hip; jitchol, GPy/GPy/util/linalg.py:56-81) steps, with the failing pivot and the rung it
stops on known in advance.

The construction: X = U(0, 1)^(N x 6), isotropic lengthscale 0.25, variance 1; row b is overwritten with row a < b, and the noise
is -1e-8 - delta, so that Ky = K - delta I.  K has one null vector (e_a - e_b) and its second-smallest eigenvalue is ~1e-2, so Ky
has ONE negative eigenvalue -delta: dpotrf stops at pivot b (info = b + 1), every rung below delta leaves that eigenvalue negative
by at least the rung itself, and the first rung above delta leaves it positive by at least half the rung -- the rung decision is
nowhere near rounding (tests/test_jitter_cases_host.py asserts all of it for every row; delta = 3e-4 goes only to rows whose second
eigenvalue is above 100 delta = 3e-2).  The ladder starts at mean(diag Ky) 1e-6
= (1 - delta) 1e-6 and multiplies by ten:

    delta   jittered attempts   jitter
    3e-6    2                   (1 - delta) 1e-5
    3e-5    3                   (1 - delta) 1e-4
    3e-4    4                   (1 - delta) 1e-3
    0.5     --                  fails even with five

Families: rbf and Mat52 through the oracle's Gram-trick kernels (its r ~ 1e-8 at the exact duplicate moves K by ~1e-16 for these
two; for Mat32 / Exponential it would move the null eigenvalue visibly, so they are left out).

An explicit table, every row with its reason; the data of a case is drawn from a generator seeded by the case id.  No GPU and no
library is needed to import this module.
"""
import collections
import functools

import numpy as np

from oracle import cpu_ref as O

D, VAR, LS = 6, 1.0, 0.25
TILE = 128
KERNEL_ID = {"rbf": 0, "Mat52": 1}           # GP_KERNEL_* of include/gphip.h

DELTA = 3e-5                                  # used everywhere
TRIES = {3e-6: 2, 3e-5: 3, 3e-4: 4}           # delta -> jittered attempts the ladder needs
DELTA_FAILS = 0.5                             # not positive definite even with five attempts
MAXTRIES = 5

# multi: these shapes run on every factorisation route (10 tiles: chain-owned columns, pipelined stages and a ragged last panel
# all exist, as in tests/test_gpu_lookahead.py); the others take the single-stream route only.
Case = collections.namedtuple("Case", "id N M P pairs fam deltas multi why")

TABLE = (
    Case("t0", 1280, 300, 1, ((0, 1),), "rbf", (3e-5,), True, "first tile: fails before any stage is released"),
    Case("odd", 1280, 300, 1, ((3, 133),), "Mat52", (3e-5,), True, "odd tile: the second tile of the pair kernel"),
    Case("even", 1280, 300, 1, ((3, 261),), "rbf", (3e-6, 3e-5), True, "even tile: the first tile of a pair"),
    Case("p0last", 1280, 300, 1, ((10, 383),), "Mat52", (3e-5, 3e-4), True,
         "last pivot of tile 2: at panel_tiles = 3 the last pivot of panel 0"),
    Case("p1first", 1280, 300, 1, ((10, 384),), "rbf", (3e-5,), True, "first pivot of tile 3 and of panel 1"),
    Case("mid", 1280, 300, 1, ((200, 677),), "Mat52", (3e-6, 3e-5, 3e-4), True,
         "interior of tile 5: with pipe_start_pct = 0 stages of earlier panels are already running"),
    Case("last", 1280, 300, 1, ((7, 1279),), "rbf", (3e-5,), True,
         "last pivot, in the one-tile last panel at panel_tiles = 3"),
    Case("r257", 257, 40, 1, ((5, 256),), "Mat52", (3e-6, 3e-5, 3e-4), False,
         "one row past a tile: 127 padding rows under the failing pivot must not set the status word"),
    Case("r385", 385, 40, 1, ((5, 384),), "rbf", (3e-6, 3e-5, 3e-4), False, "one row past three tiles"),
    Case("P2", 1280, 300, 2, ((200, 677),), "rbf", (3e-5,), True, "two outputs"),
    Case("two", 1280, 300, 1, ((3, 261), (200, 677)), "Mat52", (3e-5,), True,
         "two duplicate pairs in different tiles: the first one is reported"),
)
CASES = {c.id: c for c in TABLE}
MULTI = tuple(c.id for c in TABLE if c.multi)
SINGLE = tuple((c.id, d) for c in TABLE for d in c.deltas)

# gp_append on a fit that needed jitter: (id, N0, k, pair inside the first N0 rows, family, why)
AppendCase = collections.namedtuple("AppendCase", "id N0 k pair fam why")
APPEND = (
    AppendCase("inplace", 200, 3, (7, 150), "rbf", "the border stays inside the last tile"),
    AppendCase("split", 255, 3, (7, 130), "Mat52", "the border crosses a tile boundary: two borders"),
)
# a finite border that is not positive definite: new row j duplicates training row a (the three shapes of
# tests/test_gpu_append.py::test_border_that_is_not_finite_returns_positive_and_changes_nothing)
BorderCase = collections.namedtuple("BorderCase", "id N0 k j a fam why")
BORDER = (
    BorderCase("in-place", 100, 3, 1, 7, "rbf", "in place"),
    BorderCase("second-border", 120, 9, 8, 7, "Mat52", "the second border of a split append: the first is taken back"),
    BorderCase("new-tile", 128, 2, 0, 7, "rbf", "a new tile"),
)


def noise_of(delta):
    return -1e-8 - delta


def rung(delta, tries):
    """The jitter after ``tries`` jittered attempts, as jitchol computes it: mean(diag Ky) 1e-6, then times ten per attempt."""
    j = (VAR + (noise_of(delta) + 1e-8)) * 1e-6
    for _ in range(tries - 1):
        j *= 10.0
    return j


def first_pivot(c):
    """The 0-based pivot the un-jittered (and every failing) attempt stops at."""
    return min(b for _, b in c.pairs)


def _seed(cid):
    return int.from_bytes(cid.encode(), "little") % (2 ** 31)


def _draw(seed, N, M, P):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([np.sin(3 * (p + 1) * X.sum(1) / np.sqrt(D)) + 0.1 * rng.standard_normal(N) for p in range(P)], 1)
    Xs = rng.uniform(-0.05, 1.05, (M, D))
    return X, Y, Xs


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, Y, Xs) of a case, read-only.  Xs[0] is the duplicated point itself, Xs[1] lies next to it."""
    c = CASES[cid]
    X, Y, Xs = _draw(_seed(cid), c.N, c.M, c.P)
    for a, b in c.pairs:
        X[b] = X[a]
    Xs[0] = X[c.pairs[0][0]]
    Xs[1] = X[c.pairs[0][0]] + 0.01
    return _freeze(X, Y, Xs)


def kernel(fam):
    return O.make_kernel(fam, D, VAR, np.array([LS]), ARD=False)


@functools.lru_cache(maxsize=None)
def oracle(cid, delta=DELTA):
    """The oracle model of a case, fitted once per session (its ladder runs inside)."""
    X, Y, _ = problem(cid)
    gp = O.OracleGP(X, Y, kernel(CASES[cid].fam), noise_of(delta))
    gp.posterior
    return gp


@functools.lru_cache(maxsize=None)
def append_problem(aid):
    """(X [N0 + k, D], Y, Xs) of an append case: the pair sits inside the first N0 rows, the k new rows are distinct."""
    c = {a.id: a for a in APPEND}[aid]
    X, Y, Xs = _draw(_seed("app" + aid), c.N0 + c.k, 24, 1)
    X[c.pair[1]] = X[c.pair[0]]
    Xs[0] = X[c.pair[0]]
    return _freeze(X, Y, Xs)


@functools.lru_cache(maxsize=None)
def border_problem(bid):
    """(X [N0 + k, D] distinct rows, Xbad [k, D] whose row j is training row a, Y, Xs) of a border case."""
    c = {b.id: b for b in BORDER}[bid]
    X, Y, Xs = _draw(_seed("bor" + bid), c.N0 + c.k, 24, 1)
    Xbad = X[c.N0:].copy()
    Xbad[c.j] = X[c.a]
    return _freeze(X, Xbad, Y, Xs)


# ---- the batched entry: three tiles, the failing pivot of two members in the third tile of potrf_tile_batch_kernel --------------
BATCH_N, BATCH_DUP = 300, 40     # rows 260 .. 299 duplicate rows 0 .. 39
# Members 0 .. 5 are those of tests/test_gpu_fit_grad_batch.py::test_jitter_per_member (positive parameters, as the entry
# requires).  Its hard members (variance 1e7 .. 1e8, lengthscale >= 1, noise 1e-12) are numerically singular by the smoothness of
# the kernel alone: they give way around row 40, in the FIRST tile, duplicates or not.  Members 6 and 7 put the pivot in the
# third tile: lengthscale 0.02 leaves the 260 distinct rows with lambda_min(K) = 0.019 variance, and at variance 1e9 / 1e10 the
# 1.0001e-8 the diagonal gets is below half an ulp, so rows 260 + i and i of Ky are bitwise equal -- 40 pivots that are exactly
# zero plus rounding of either sign (~1e-6), each a failure with probability 1/2 or more, none possible before row 260.  The
# first rung (variance 1e-6 = 1e3 .. 1e4) is nine orders above that rounding.
BATCH_VAR = np.array([1.0, 1e8, 1.0, 1e7, 1.0, 1e8, 1e10, 1e9])
BATCH_LS = np.array([[0.3], [2.0], [0.3], [1.5], [0.25], [1.0], [0.02], [0.02]])
BATCH_NOISE = np.array([1e-2, 1e-12, 1e-3, 1e-12, 1e-2, 1e-12, 1e-12, 1e-12])
BATCH_THIRD_TILE = (6, 7)


@functools.lru_cache(maxsize=None)
def batch_problem():
    rng = np.random.default_rng(5)
    n = BATCH_N - BATCH_DUP
    X = rng.uniform(0, 1, (n, 2))
    Y = (np.sin(2 * np.pi * X).sum(1) / np.sqrt(2) + 0.1 * rng.standard_normal(n))[:, None]
    return _freeze(np.vstack([X, X[:BATCH_DUP]]), np.vstack([Y, Y[:BATCH_DUP]]))
