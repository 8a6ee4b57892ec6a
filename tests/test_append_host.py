"""CPU: the border algebra ``gp_append`` implements (csrc/append.hip, csrc/api_append.hip), pinned in NumPy against
``scipy.linalg.cholesky`` of the grown matrix; the conditioning of the inputs tests/test_gpu_append.py sends to the device; and
the argument checks of ``Handle.append`` and ``GPModel(incremental=...)`` that need no device.
"""
import numpy as np
import pytest
import scipy.linalg

import _append_cases as C
import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib

EPS = np.finfo(float).eps


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "N%d+%d" % s[0])
def test_route_counts_of_the_shapes(shape):
    (N0, k), want = shape
    assert C.routes(N0, k) == want


@pytest.mark.parametrize("kern", C.KERNELS, ids=lambda c: c[0] + ("-ard" if c[2] else ""))
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "N%d+%d" % s[0])
def test_border_algebra_is_the_cholesky_of_the_grown_matrix(shape, kern):
    """L, and L^-1 with its new rows Li21 = -L22^-1 (L21 Li11), Li22 = L22^-1, grown border by border are the factor of the grown
    matrix and its inverse.  Bound: both routes are backward stable, so they differ by a few cond(Ky) eps relative to |L|
    (|L^-1|); cond(Ky) is computed, and 1e-6 -- the bound the device is held to -- must contain it with room."""
    (N0, k), _ = shape
    kname, _, ard = kern
    X, _, _, _, _, k_or = C.problem(7 * N0 + k, N0 + k, 2 if N0 % 2 else 5, 1, kname, ard)
    Ky = k_or.K(X) + (1e-2 + 1e-8) * np.eye(N0 + k)
    cond = np.linalg.cond(Ky)
    L0 = scipy.linalg.cholesky(Ky[:N0, :N0], lower=True)
    Li0 = scipy.linalg.solve_triangular(L0, np.eye(N0), lower=True)
    L, Li = C.grow(L0, Li0, Ky, N0, k)
    Lref = scipy.linalg.cholesky(Ky, lower=True)
    Liref = scipy.linalg.solve_triangular(Lref, np.eye(N0 + k), lower=True)
    tol = 50 * cond * EPS
    assert tol < 1e-7, cond
    assert np.max(np.abs(L - Lref)) <= tol * np.max(np.abs(Lref))
    assert np.max(np.abs(Li - Liref)) <= tol * np.max(np.abs(Liref))
    assert np.array_equal(L[:N0, :N0], L0) and np.array_equal(Li[:N0, :N0], Li0)      # the old rows are not touched
    assert np.all(np.triu(L, 1) == 0) and np.all(np.triu(Li, 1) == 0)
    # log det grows by the border's diagonal alone
    assert abs(2 * np.log(np.diag(L)).sum() - np.linalg.slogdet(Ky)[1]) <= 1e-10 * (N0 + k)


@pytest.mark.parametrize("kern", C.KERNELS, ids=lambda c: c[0] + ("-ard" if c[2] else ""))
def test_inputs_of_the_gpu_cases_are_well_conditioned(kern):
    """Noise 1e-2, uniform X in the unit box, the lengthscales of tests/test_gpu_random_shapes.py: cond(Ky) eps stays orders
    below the 1e-8 (LML) and 1e-6 bounds the oracle itself is trusted at, for every shape, D in {2, 5}."""
    kname, _, ard = kern
    worst = 0.0
    for (N0, k), _ in C.SHAPES:
        for D in (2, 5):
            X, _, _, _, var, k_or = C.problem(1000 + N0 + k + D, N0 + k, D, 1, kname, ard)
            Ky = k_or.K(X) + (1e-2 + 1e-8) * np.eye(N0 + k)
            worst = max(worst, np.linalg.cond(Ky))
    print("%s%s: worst cond(Ky) %.3g, cond eps %.3g" % (kname, "-ard" if ard else "", worst, worst * EPS))
    assert worst * EPS < 1e-10


def test_stress_input_is_within_reach_of_float64():
    """Noise 1e-6 (exact_feval), N0 = 200, k = 5: cond(Ky) eps is what the oracle and the device each carry; the absolute
    variance criterion of the stress case (1e-6 max(1, |v|) + 1e-9) must contain it."""
    X, _, _, _, var, k_or = C.problem(4242, 205, 2, 1, "Mat52", False)
    cond = np.linalg.cond(k_or.K(X) + (1e-6 + 1e-8) * np.eye(205))
    print("stress: cond(Ky) %.3g, cond eps %.3g" % (cond, cond * EPS))
    assert cond * EPS * var < 1e-7


def test_gpmodel_incremental_flag():
    assert gpo.GPModel().incremental is False
    assert gpo.GPModel(incremental=True, max_iters=0).incremental is True
    with pytest.raises(ValueError, match="incremental"):
        gpo.GPModel(sparse=True, incremental=True)
    assert gpo.GPModel.fromConfig(dict(incremental=True)).incremental is True


def test_bayesian_optimization_forwards_the_flag():
    dom = [{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}]
    X, Y = np.zeros((3, 2)), np.zeros((3, 1))
    assert gpo.BayesianOptimization(f=None, domain=dom, X=X, Y=Y).model.incremental is False
    assert gpo.BayesianOptimization(f=None, domain=dom, X=X, Y=Y, incremental=True, max_iters=0).model.incremental is True


def test_is_head_is_bitwise():
    class _M(object):
        pass
    gm = gpo.GPModel(incremental=True, max_iters=0)
    gm.model = _M()
    gm.model.X = np.arange(6.0).reshape(3, 2)
    more = np.vstack([gm.model.X, [[7.0, 8.0]]])
    assert gm._is_head(more)
    assert not gm._is_head(gm.model.X)                       # nothing new
    bent = more.copy()
    bent[1, 1] = np.nextafter(bent[1, 1], 10.0)              # one bit
    assert not gm._is_head(bent)
    assert not gm._is_head(np.hstack([more, more]))


class _Recorder(object):
    """Stands in for the library: records whether gp_append was reached."""
    def __init__(self):
        self.calls = 0

    def gp_append(self, *a):
        self.calls += 1
        return 0


def _bare_handle(N, D, P):
    h = _lib.Handle.__new__(_lib.Handle)
    h.lib, h.h, h.N, h.D, h.P = _Recorder(), None, N, D, P
    return h


def test_handle_append_checks_shapes_before_the_library():
    h = _bare_handle(10, 3, 2)
    with pytest.raises(ValueError, match="columns"):
        h.append(np.zeros((2, 4)), np.zeros((12, 2)))
    with pytest.raises(ValueError, match="ALL targets"):
        h.append(np.zeros((2, 3)), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="ALL targets"):
        h.append(np.zeros((2, 3)), np.zeros((12, 1)))
    with pytest.raises(ValueError):
        h.append(np.zeros(3), np.zeros((11, 2)))
    assert h.lib.calls == 0
    h.append(np.zeros((2, 3)), np.zeros((12, 2)))
    assert h.lib.calls == 1 and h.N == 12
    fresh = _lib.Handle.__new__(_lib.Handle)
    fresh.lib, fresh.h = _Recorder(), None
    with pytest.raises(ValueError, match="set_data"):
        fresh.append(np.zeros((1, 3)), np.zeros((1, 1)))
    fresh.h = h.h = None        # (nothing to destroy)


def test_positive_return_is_a_linalg_error():
    h = _bare_handle(4, 1, 1)
    h.lib.gp_append = lambda *a: 5
    with pytest.raises(np.linalg.LinAlgError):
        h.append(np.zeros((1, 1)), np.zeros((5, 1)))
    assert h.N == 4
    h.h = None
