"""Shapes, inputs and the NumPy statement of the border algebra shared by tests/test_append_host.py and tests/test_gpu_append.py.

``gp_append`` grows the factor of Ky = K + (noise + 1e-8 + jitter) I by k rows that lie inside ONE 128-row diagonal tile; a call
whose rows would cross a tile boundary runs as two such borders.  For a border under N rows,

    T = L11^-1 K(X, Xnew),  S = K(Xnew, Xnew) + d I - T^T T,  L22 = chol(S),  L21 = T^T,
    Li21 = -L22^-1 (L21 Li11),  Li22 = L22^-1.
"""
import numpy as np

import _kernel_families as KF

TILE = 128

# (N0, k): the smallest shapes at which each route can go wrong, and the route counts (in place, relayout) they must show
SHAPES = [
    ((100, 1), (1, 0)), ((100, 8), (1, 0)), ((120, 8), (1, 0)),      # in place; (120, 8) fills the tile exactly
    ((128, 1), (0, 1)), ((256, 5), (0, 1)),                           # a new tile
    ((120, 9), (1, 1)), ((250, 28), (1, 1)),                          # split across the boundary
    ((300, 9), (1, 0)),                                               # two tiles of history, a 9-row border: two inverse-factor passes
]
# (kernel name, device id, ARD): the four families iso, RBF and Matern-5/2 with ARD
KERNELS = [("rbf", 0, False), ("Mat52", 1, False), ("Mat32", 2, False), ("Exponential", 3, False), ("rbf", 0, True), ("Mat52", 1, True)]


def routes(N0, k):
    """(borders written in place, borders that open a new tile) of an append of k rows under N0."""
    room = -N0 % TILE
    if room == 0:
        return 0, 1
    return (1, 0) if k <= room else (1, 1)


def problem(seed, N, D, P, kname, ard, M=24):
    """Uniform X in the unit box, the lengthscales of tests/test_gpu_random_shapes.py, standard-normal targets."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = rng.standard_normal((N, P))
    Xs = rng.uniform(-0.05, 1.05, (M, D))
    ls = rng.uniform(0.4, 1.5, D) * np.sqrt(D) * 0.5 if ard else np.array([0.35 * np.sqrt(D)])
    var = float(rng.uniform(0.5, 2.5))
    return X, Y, Xs, ls, var, KF.make(kname, D, var, ls, ard)


def border(L11, Li11, K12, K22d):
    """(L21, L22, Li21, Li22) of one border: K12 = K(X, Xnew) [N, k], K22d = K(Xnew, Xnew) + d I."""
    from scipy.linalg import solve_triangular
    T = solve_triangular(L11, K12, lower=True)
    S = K22d - T.T @ T
    L22 = np.linalg.cholesky(S)
    L22i = solve_triangular(L22, np.eye(L22.shape[0]), lower=True)
    return T.T, L22, -L22i @ (T.T @ Li11), L22i


def grow(L, Li, Ky, N0, k):
    """The factor (and inverse factor) of Ky[:N0 + k, :N0 + k] from those of Ky[:N0, :N0], one border per side of a tile
    boundary, as the device carries an append out."""
    n = N0
    while n < N0 + k:
        room = -n % TILE or TILE
        kk = min(room, N0 + k - n)
        L21, L22, Li21, Li22 = border(L, Li, Ky[:n, n:n + kk], Ky[n:n + kk, n:n + kk])
        z = np.zeros((n, kk))
        L = np.block([[L, z], [L21, L22]])
        Li = np.block([[Li, z], [Li21, Li22]])
        n += kk
    return L, Li
