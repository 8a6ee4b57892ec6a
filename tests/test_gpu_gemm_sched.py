"""GPU: the scheduled K loop of the 8-wave fp64 GEMM instance (option "gemm_sched" = 1, ``gemm_nt_sched_kernel`` of csrc/gemm.hip)
against the plain loop (0), bit for bit, with that instance forced at every tile count and on every stream ("long_min_tiles" = 1,
"gemm_sched_side" = 1, no 64 x 64 work units, no paired triangular-K twin -- the twin keeps the plain loop).

The scheduled loop has three stage instances -- a stage that writes the next one and loads the one after, the last but one
(writes, loads nothing) and the last (neither, no barrier) -- and two LDS buffers that flip behind the barrier, so the shapes are
the contraction lengths at which each instance runs alone or first on either buffer: K = 16 (one stage), 32 (two), 48 (three: an
odd count, the last stage back on the first buffer) and 768.  No entry point of the library contracts fewer than 128 columns, so
these go through the test hook ``gp_debug_gemm`` (one launch through the library's instance selection, host operands), with a
rectangular set of 3 x 2 tiles away from the origin and a triangular set of 3 tile rows, C = A B^T and C -= A B^T; the hook's
results are also held to numpy within the forward error bound of a K-term dot product in any order, (K + 2) u sum |a||b| for
either side (u = 2^-53), and tiles outside the set have to keep their bits.  The launch through an explicit tile list is the same
hook at 256 x 8 = 2048 tiles (the library's threshold for the super-tile order; no option lowers it), K = 16.

Through the entry points proper: fit + predict at N = 300, M = 130 with two-tile panels (padded rows and columns; the products
with the inverted panel contract one and two blocks in their two column tiles: ``k_end_tri``), Ky^-1 at N = 384 (``k_tri``: the
product accumulated per panel, C -= A B^T with ``k_sub``, and as one launch, C = A B^T), and two members side by side with
strides (``gp_fit_grad_batch``).
"""
import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
T = 128


@pytest.fixture(scope="module")
def h():
    hd = _lib.Handle(0)
    for name, value in (("long_min_tiles", 1), ("small_below", 0), ("chain_small_below", 0), ("pair_tri", 0), ("gemm_sched_side", 1)):
        hd.set_option(name, value)
    yield hd
    hd.close()


def _both(h, fn):
    out = []
    for sched in (0, 1):
        h.set_option("gemm_sched", sched)
        out.append(fn())
    return out


_operands = {}


def _ops(r1, c1, ld):
    """C, A, B of one shape, drawn once (uniform in [-1/2, 1/2))."""
    key = (r1, c1, ld)
    if key not in _operands:
        rng = np.random.default_rng(r1 * 100003 + c1 * 1009 + ld)
        _operands[key] = tuple(rng.random((n * T, ld)) - 0.5 for n in (r1, r1, c1))
    return _operands[key]


def _tiles(r0, r1, c0, c1, tri):
    return [(i, c) for c in range(c0, c1) for i in range(c if tri else r0, r1)]


def _check_hook(h, mode, K, r0, r1, c0, c1, tri, ld):
    C, A, B = _ops(r1, c1, ld)
    plain, sched = _both(h, lambda: h.debug_gemm(mode, C, A, B, K, r0, r1, c0, c1, tri))
    assert np.array_equal(plain, sched)
    prod = A[:, :K] @ B[:, :K].T
    mag = np.abs(A[:, :K]) @ np.abs(B[:, :K]).T
    inside = np.zeros(C.shape, dtype=bool)
    for i, c in _tiles(r0, r1, c0, c1, tri):
        inside[i * T:(i + 1) * T, c * T:(c + 1) * T] = True
    assert np.array_equal(sched[~inside], C[~inside])            # tiles outside the set (and columns beyond them) keep their bits
    w = c1 * T
    want = (C[:, :w] - prod) if mode else prod
    bound = 2.0 * (K + 2) * U * (mag + (np.abs(C[:, :w]) if mode else 0.0))
    err = np.abs(sched[:, :w] - want)
    m = inside[:, :w]
    print("mode %d K %d tiles %d: max err %.3e, max err / bound %.3f" % (mode, K, m.sum() // (T * T), err[m].max(), (err[m] / bound[m]).max()))
    assert np.all(err[m] <= bound[m])


@pytest.mark.parametrize("K", [16, 32, 48, 768])
@pytest.mark.parametrize("mode", [0, 1])
def test_rectangular_3x2_tiles(h, mode, K):
    _check_hook(h, mode, K, 1, 4, 1, 3, False, max(K, 3 * T))


@pytest.mark.parametrize("K", [16, 32, 48, 768])
@pytest.mark.parametrize("mode", [0, 1])
def test_triangular_3_tile_rows(h, mode, K):
    _check_hook(h, mode, K, 0, 3, 0, 3, True, max(K, 3 * T))


def test_explicit_tile_list_2048_tiles(h):
    try:
        _check_hook(h, 1, 16, 0, 256, 0, 8, False, 8 * T)
    finally:
        _operands.pop((256, 8, 8 * T), None)   # (half a gigabyte of operands)


def _problem(N, M, seed):
    X, Y, Xs = O.synthetic_problem(N, 3, M, seed=seed)
    return X, Y, Xs, O.default_lengthscale(3, False)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_fit_predict_padded_rows_two_tile_panels(h):
    """N = 300 (three row tiles, 84 padding rows), M = 130 (two candidate tiles, 126 padding rows), panels of two tiles."""
    X, Y, Xs, ls = _problem(300, 130, 11)
    h.set_option("panel_tiles", 2)

    def run():
        h.set_data(X, Y)
        h.set_params(0, False, 1.0, ls, 1e-2)
        fit = h.fit()
        L = h.chol()
        h.set_candidates(Xs)
        mu, var = h.predict(True)
        return list(fit) + [L, h.alpha(), mu, var]
    plain, sched = _both(h, run)
    h.set_option("panel_tiles", 6)
    _same(plain, sched)
    assert np.all(np.isfinite(sched[-1])) and np.all(np.isfinite(sched[3]))


@pytest.mark.parametrize("lauum_panels", [1, 0])
def test_woodbury_inverse_k_tri(h, lauum_panels):
    """Ky^-1 = (L^-T)(L^-T)^T at N = 384: the contraction of row tile i starts at column tile i."""
    X, Y, _, ls = _problem(384, 1, 12)
    h.set_option("lauum_panels", lauum_panels)
    h.set_option("panel_tiles", 2)

    def run():
        h.set_data(X, Y)
        h.set_params(0, False, 1.0, ls, 1e-2)
        h.fit()
        return [h.woodbury_inv()]
    plain, sched = _both(h, run)
    h.set_option("lauum_panels", 1)
    h.set_option("panel_tiles", 6)
    _same(plain, sched)
    assert np.all(np.isfinite(sched[0]))


def test_two_members_with_strides(h):
    """gp_fit_grad_batch with two parameter vectors: every GEMM launch carries both members (blockIdx.y, pointer strides)."""
    X, Y, _, ls = _problem(300, 1, 13)

    def run():
        h.set_data(X, Y)
        h.set_params(0, False, 1.0, ls, 1e-2)
        fit, grad, status = h.fit_grad_batch([1.0, 1.7], np.array([ls, 0.8 * ls]).reshape(2, 1), [1e-2, 3e-2])
        assert not status.any()
        return list(fit) + list(grad)
    plain, sched = _both(h, run)
    _same(plain, sched)
    assert all(np.all(np.isfinite(x)) for x in sched)
