"""GPU: gp_lml_grad_x / gp_fit_grad_x -- the LML's gradient with respect to the training inputs (csrc/gradx.hip) against the
oracle's ``Stationary.gradients_X(dL_dK, X)`` with X2 = None (oracle/cpu_ref.py; stationary.py:336-352), all four covariance
families, iso and ARD.

Oracle: ``KF.make(fam, D, 1.3, ls, ard, direct=True)`` (direct-difference distances, tests/_kernel_families.py), then
``O.exact_gaussian_inference(kern, X, Y, 1e-2)`` and ``kern.gradients_X(p["dL_dK"], X)``.  X uniform in [0, 1]^D,
Y = sin(3 sum x) + 0.1 eps, seeded.  Tolerance: the north star as tests/test_gpu_kernel_families.py applies it, 1e-6 of the
largest reference entry; every figure is printed before it is asserted.  On these inputs the Gram-trick and direct-difference
oracles agree to between 1e-14 and 6e-10 and the direct oracle matches central differences of its own LML to 1e-7 (measured on
the CPU), so the reference alone sits three decades inside the tolerance -- except on coincident points, where the Gram-trick
oracle is 1.9e-6 off the direct one for the ARD Exponential: the direct oracle is the yardstick throughout.

Shapes, each the smallest that reaches one thing:
  N = 300, D = 3    three row tiles, the last one padded
  N = 130, D = 1    two tiles with two valid rows in the second
  N = 257, D = 17   a second pass of 16 dimensions holding one dimension
  N = 128, D = 3    no padding
  N = 130, D = 64   GP_MAX_D: four passes and the largest staging area
  N = 640, D = 2    five column tiles: a second chunk of column tiles, holding one tile (the chunks' partial sums are added
                    by the second launch)
"""
import functools

import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

import _kernel_families as KF

pytestmark = pytest.mark.gpu

VAR, NOISE, TOL = 1.3, 1e-2, 1e-6
KID = {"rbf": _lib.GP_KERNEL_RBF, "Mat52": _lib.GP_KERNEL_MATERN52, "Mat32": _lib.GP_KERNEL_MATERN32,
       "Exponential": _lib.GP_KERNEL_EXPONENTIAL}
SHAPES = [(300, 3), (130, 1), (257, 17), (128, 3), (130, 64), (640, 2)]
CASES = [pytest.param(n, d, f, a, id="N%d-D%d-%s-%s" % (n, d, f, "ard" if a else "iso"))
         for (n, d) in SHAPES for f in KID for a in (False, True)]


def _ls(D, ard):
    return np.linspace(0.4, 1.1, D) if ard else np.array([0.5])


@functools.lru_cache(maxsize=None)
def _problem(N, D, coincident=False, P=1):
    rng = np.random.default_rng(20261 + 1000 * N + D)
    X = rng.uniform(0, 1, (N, D))
    if coincident:
        X[100:110] = X[0:10]
    Y = (np.sin(3 * X.sum(1)) + 0.1 * rng.standard_normal(N))[:, None]
    if P == 2:
        Y = np.c_[Y, np.cos(2 * X.sum(1)) + 0.1 * rng.standard_normal(N)]
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def _ref(N, D, fam, ard, coincident=False, P=1):
    """The oracle's dL/dX of one case, computed once, read-only."""
    X, Y = _problem(N, D, coincident, P)
    kern = KF.make(fam, D, VAR, _ls(D, ard), ard, direct=True)
    p = O.exact_gaussian_inference(kern, X, Y, NOISE)
    g = np.asarray(kern.gradients_X(p["dL_dK"], X), dtype=float)
    g.setflags(write=False)
    return g


def _err(what, got, ref, tol=TOL):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), what
    e = float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-300)
    print("%-44s err %.3e  tol %.1e" % (what, e, tol))
    assert e <= tol, (what, e, tol)


@pytest.fixture(scope="module")
def h():
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", 0)
    yield hd
    hd.close()


def _fit(h, N, D, fam, ard, coincident=False, P=1):
    X, Y = _problem(N, D, coincident, P)
    h.set_data(X, Y)
    h.set_gower()
    h.set_params(KID[fam], ard, VAR, _ls(D, ard), NOISE)
    h.fit()
    return X, Y


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N,D,fam,ard", CASES)
def test_against_the_oracle(h, N, D, fam, ard):
    _fit(h, N, D, fam, ard)
    _err("dL_dX N=%d D=%d %s %s" % (N, D, fam, "ard" if ard else "iso"), h.lml_grad_x(), _ref(N, D, fam, ard))


@pytest.mark.parametrize("fam", list(KID))
@pytest.mark.parametrize("ard", [False, True], ids=["iso", "ard"])
def test_coincident_points(h, fam, ard):
    """Rows 100..109 equal to rows 0..9: r = 0 off the diagonal, where _inv_dist (stationary.py:251-258) is 0 and the
    Exponential's dK_dr / r is singular."""
    _fit(h, 300, 3, fam, ard, coincident=True)
    g = h.lml_grad_x()
    assert np.all(np.isfinite(g))
    _err("coincident dL_dX %s %s" % (fam, "ard" if ard else "iso"), g, _ref(300, 3, fam, ard, coincident=True))


@pytest.mark.parametrize("fam,ard", [("Mat52", True), ("Exponential", False)])
def test_two_outputs(h, fam, ard):
    _fit(h, 300, 3, fam, ard, P=2)
    _err("P = 2 dL_dX %s" % fam, h.lml_grad_x(), _ref(300, 3, fam, ard, P=2))


@pytest.mark.parametrize("N,D,fam,ard", [(300, 3, "Mat52", True), (257, 17, "Mat32", True), (640, 2, "rbf", False)])
def test_fit_grad_x_is_fit_grad_then_lml_grad_x(h, N, D, fam, ard):
    X, Y = _problem(N, D)
    nls = D if ard else 1
    h.set_data(X, Y)
    h.set_gower()
    h.set_params(KID[fam], ard, VAR, _ls(D, ard), NOISE)
    fit1, (dv1, dl1, dn1) = h.fit_grad(nls)
    gx1 = h.lml_grad_x()
    gx1b = h.lml_grad_x()
    assert _same_bits(gx1, gx1b), "gp_lml_grad_x twice in a row"
    h.set_data(X, Y)
    h.set_params(KID[fam], ard, VAR, _ls(D, ard), NOISE)
    fit2, (dv2, dl2, dn2), gx2 = h.fit_grad_x(nls)
    assert _same_bits(fit1, fit2), (fit1, fit2)
    assert _same_bits([dv1, dn1], [dv2, dn2]) and _same_bits(dl1, dl2)
    assert _same_bits(gx1, gx2)
    _err("fit_grad_x dL_dX %s" % fam, gx2, _ref(N, D, fam, ard))
    assert "lml_grad_x" in [p["name"] for p in h.phases()] and "lml_grad" in [p["name"] for p in h.phases()]


def test_other_entries_return_the_same_bits_afterwards(h):
    """gp_lml_grad, gp_predict and gp_fmin give the bits they give without the call -- asked for before it, after it, and
    in a sequence that never makes it."""
    N, D, fam, ard = 300, 3, "Mat52", True
    X, _ = _problem(N, D)
    Xs = np.random.default_rng(5).uniform(0, 1, (130, D))

    def others():
        return h.lml_grad(D), h.predict(True), h.fmin()

    _fit(h, N, D, fam, ard)
    h.set_candidates(Xs)
    without = others()
    _fit(h, N, D, fam, ard)
    h.set_candidates(Xs)
    h.predict(True)
    gx = h.lml_grad_x()
    after = others()
    gx2 = h.lml_grad_x()
    again = others()
    for got in (after, again):
        (dv0, dl0, dn0), (m0, v0), f0 = without
        (dv, dl, dn), (m, v), f = got
        assert _same_bits([dv0, dn0, f0], [dv, dn, f]) and _same_bits(dl0, dl)
        assert _same_bits(m0, m) and _same_bits(v0, v)
    assert _same_bits(gx, gx2)
    _err("dL_dX between the other entries", gx, _ref(N, D, fam, ard))


def test_emulated_fit():
    """Under "emulate_fp64" the pass stays true fp64 and reads the Ky^-1 the emulated fit produced: the same tolerance."""
    N, D, fam, ard = 300, 3, "Mat52", True
    hd = _lib.Handle(0)
    try:
        hd.set_option("emulate_fp64", 1)
        _fit(hd, N, D, fam, ard)
        _err("emulated dL_dX", hd.lml_grad_x(), _ref(N, D, fam, ard))
        X, Y = _problem(N, D)
        hd.set_data(X, Y)
        hd.set_params(KID[fam], ard, VAR, _ls(D, ard), NOISE)
        _err("emulated fit_grad_x dL_dX", hd.fit_grad_x(D)[2], _ref(N, D, fam, ard))
    finally:
        hd.close()


def test_return_codes():
    N, D = 130, 3
    X, Y = _problem(N, D)
    hd = _lib.Handle(0)
    try:
        out = np.empty((N, D))
        hd.set_data(X, Y)
        hd.set_params(_lib.GP_KERNEL_RBF, False, VAR, _ls(D, False), NOISE)
        assert hd.lib.gp_lml_grad_x(hd.h, _lib.dptr(out)) == _lib.GP_ERR_STATE        # no fit
        hd.fit()
        assert hd.lib.gp_lml_grad_x(hd.h, None) == _lib.GP_ERR_ARG                    # NULL
        assert hd.lib.gp_lml_grad_x(None, _lib.dptr(out)) == _lib.GP_ERR_ARG
        assert hd.lib.gp_lml_grad_x(hd.h, _lib.dptr(out)) == 0
        hd.set_gower(np.array([0, 1, 0]), np.array([1.0, 1.0, 2.0]))                  # Gower on
        hd.fit()
        assert hd.lib.gp_lml_grad_x(hd.h, _lib.dptr(out)) == _lib.GP_ERR_ARG
        with pytest.raises(ValueError, match="Gower"):
            hd.fit_grad_x(1)
        hd.set_gower()
        Y17 = np.tile(Y, (1, 17))                                                      # beyond the P limit
        hd.set_data(X, Y17)
        hd.fit()
        assert hd.lib.gp_lml_grad_x(hd.h, _lib.dptr(out)) == _lib.GP_ERR_ARG
        with pytest.raises(ValueError, match="P <= 16"):
            hd.fit_grad_x(1)
    finally:
        hd.close()
