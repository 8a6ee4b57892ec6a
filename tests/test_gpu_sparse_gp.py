"""GPU: the sparse GP (variational DTC) -- csrc/sparse.hip and csrc/api_sparse.hip behind the ``gp_sparse_*`` entry points
(include/gphip.h, "sparse GP"), ``SparseGPRegression``, ``GPModel(sparse=True)`` and the BO surface over it.

Reference: GPy/GPy/inference/latent_function_inference/var_dtc.py:66-277, GPy/GPy/core/sparse_gp.py:41-119, posterior.py:225-248,
GPy/GPy/core/gp.py:407-454, restated in two precisions in tests/_sparse_ref.py.

Cases (tests/_sparse_ref.py CASES; inputs uniform in [0, 1]^D, the first half of Z on data rows, the second half moved by
0.03 N(0, 1); lengthscales linspace(0.15, 0.35, D) sqrt(D / 3), iso: the first of them; variance 1.3, noise 2e-2, mc_max = 128):
  S1  N = 96,  Mz = 10,  D = 3,  P = 1   everything inside one tile; GPyOpt's default Mz
  S2  N = 300, Mz = 130, D = 3,  P = 2   N and Mz both cross a tile with padding; two outputs
  S3  N = 130, Mz = 128, D = 3,  P = 1   Mz exactly one tile, N two rows past it
  S4  N = 200, Mz = 40,  D = 17, P = 1   D crosses the GP_GRAD_CH = 16 pass boundary
  S5  N = 64,  Mz = 1,   D = 2,  P = 1   a single inducing input
All four families on S1 and S2 (ARD) and on S3 and S5 (iso); RBF and Exponential on S4, iso and ARD.  Each run asserts on its
own inputs that cond(Kmm) <= 8.9e4 and that neither jitter ladder stepped (oracle and device), so that the comparison cannot
quietly become a jitter lottery.

Tolerance rule (fit, gradients, prediction): for each quantity the bound is MULT times the float64 oracle's own error against
the long-double truth on the same inputs, with a floor of 1e-13 of the quantity's largest entry: bound = max(MULT x oracle error,
1e-13 x scale).  MULT is the smallest power of two that leaves a factor 4 over the worst ratio observed on an MI355X,
profiles/sparse_gp_errors.txt (written by tools/sparse_errors.py from this suite's own printed figures):
  "326 quantities, 10 above the floor; worst ratio above the floor 1.38 (S2 rbf ard: 130 rows noise=1 var); x 4 = 5.53 -> MULT = 8."
  "S2 rbf ard: dlengthscale   scale 5.014e+03  device 2.956e-09  oracle 5.286e-09  ratio 0.56"
  "S2 rbf ard: 130 rows noise=1 dvdx   scale 3.373e+00  device 5.389e-12  oracle 4.141e-12  ratio 1.30"
(a ratio counts where the device's error is above the floor: below it the oracle's own error is often a lucky 1e-17 -- fmin of
S3 Matern-3/2: device 2.2e-16, oracle 6.5e-19 -- and the floor is the bound).
The device applies explicit inverse factors and 128-wide MFMA contractions where LAPACK substitutes; both have forward error
proportional to cond eps, with different constants.

Also here: the noise below the 1e-8 clamp (beta = 1e8; ``dnoise`` the reference's formula value); bitwise determinism of
``gp_sparse_fit_grad`` and ``gp_sparse_predict``; a row's prediction bitwise independent of its company (tables of 1, 5 and 130
rows: 130 crosses a chunk), as include/gphip.h states; the exact model bitwise untouched by interleaved sparse calls; every
refusal; and the model level: the objective gradient of ``SparseGPRegression`` (Matern-5/2, N = 60, Mz = 8) against central
differences of its own objective with step 1e-5 at 1e-5 of the largest entry (truncation h^2 |f'''| / 6 ~ 1e-9 relative,
rounding ~ 1e-12 |f| / h ~ 1e-5 of gradients of order |f| / 100, as derived in tests/test_gpu_warped_gp.py), ``optimize`` not
increasing the objective, and two BO suggestions that keep Z's shape.
Every figure is printed before it is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib

import _sparse_ref as R

pytestmark = pytest.mark.gpu

MULT = 8.0
FLOOR = 1e-13
FAMS = ["rbf", "Mat52", "Mat32", "Exponential"]
KID = {"rbf": _lib.GP_KERNEL_RBF, "Mat52": _lib.GP_KERNEL_MATERN52, "Mat32": _lib.GP_KERNEL_MATERN32,
       "Exponential": _lib.GP_KERNEL_EXPONENTIAL}
RUNS = [("S1", f, True) for f in FAMS] + [("S2", f, True) for f in FAMS] + [("S3", f, False) for f in FAMS] + \
       [("S5", f, False) for f in FAMS] + [("S4", f, a) for f in ("rbf", "Exponential") for a in (False, True)]
IDS = ["%s-%s-%s" % (c, f, "ard" if a else "iso") for c, f, a in RUNS]
FIT_Q = ["lml", "woodbury_vector", "woodbury_inv"]
GRAD_Q = ["dvariance", "dlengthscale", "dnoise", "dZ"]
PRED_Q = ["mean", "var", "dmdx", "dvdx"]
LDT = np.longdouble


@functools.lru_cache(maxsize=None)
def _ref(case, fam, ard, noise=R.NOISE):
    """Inputs, the float64 oracle and the long-double truth of a run: fit, gradients, the 130-row table with and without the
    likelihood's noise, fmin.  Computed once and shared; read-only."""
    X, Y, Z, Xs = R.case_inputs(case)
    ls = R.case_lengthscale(X.shape[1], ard)
    out = dict(X=X, Y=Y, Z=Z, Xs=Xs, ls=ls)
    for tag, lin in (("f64", R.F64), ("ld", R.LD)):
        f = R.inference(fam, X, Z, Y, R.VARIANCE, ls, ard, noise, lin)
        for inc in (True, False):
            f["pred%d" % inc] = dict(zip(PRED_Q, R.predict(f, Z, Xs, noise, inc, lin)))
        f["fmin"] = R.fmin(f, X)
        out[tag] = f
    return out


def _handle(case, fam, ard, noise=R.NOISE):
    r = _ref(case, fam, ard, noise)
    h = _lib.Handle(0)
    h.set_option("mc_max", 128)
    h.set_data(r["X"], r["Y"])
    h.set_params(KID[fam], ard, R.VARIANCE, r["ls"], noise)
    h.sparse_set_inducing(r["Z"])
    return h, r


def _check(what, got, oracle, truth):
    """The tolerance rule of the module docstring."""
    truth = np.asarray(truth, dtype=LDT)
    got = np.asarray(got, dtype=float).reshape(truth.shape)
    assert np.all(np.isfinite(got)), what
    scale = float(np.max(np.abs(truth)))
    dev = float(np.max(np.abs(got.astype(LDT) - truth)))
    orc = float(np.max(np.abs(np.asarray(oracle, dtype=LDT).reshape(truth.shape) - truth)))
    bound = max(MULT * orc, FLOOR * scale)
    print("%-44s scale %.3e  device %.3e  oracle %.3e  ratio %7.2f  bound %.3e" % (what, scale, dev, orc, dev / max(orc, 1e-300), bound))
    assert dev <= bound, (what, dev, bound)


def _conditions(r, jitters):
    cond = float(np.linalg.cond(np.asarray(r["f64"]["Kmm"], dtype=float)))
    print("cond(Kmm) %.3g  oracle jitters %g %g  device jitters %g %g" % ((cond, r["f64"]["jitter_kmm"], r["f64"]["jitter_b"]) + jitters))
    assert cond <= 8.9e4
    assert r["f64"]["jitter_kmm"] == 0.0 and r["f64"]["jitter_b"] == 0.0 and jitters == (0.0, 0.0)


# ---- fit and gradients -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fam,ard", RUNS, ids=IDS)
def test_fit_and_gradients_against_long_double(case, fam, ard):
    h, r = _handle(case, fam, ard)
    try:
        lml0, jk, jb = h.sparse_fit()
        _conditions(r, (jk, jb))
        wv, wi = h.sparse_posterior()
        lml, (dv, dl, dn, dZ) = h.sparse_fit_grad(r["ls"].size)
        assert lml == lml0                                   # the fit of gp_sparse_fit_grad is gp_sparse_fit's
        got = dict(lml=lml, woodbury_vector=wv, woodbury_inv=wi, dvariance=dv, dlengthscale=dl, dnoise=dn, dZ=dZ)
        for q in FIT_Q + GRAD_Q:
            _check("%s %s %s: %s" % (case, fam, "ard" if ard else "iso", q), got[q], r["f64"][q], r["ld"][q])
        # the same inputs give the same bits
        lml2, (dv2, dl2, dn2, dZ2) = h.sparse_fit_grad(r["ls"].size)
        assert (lml2, dv2, dn2) == (lml, dv, dn) and np.array_equal(dl2, dl) and np.array_equal(dZ2, dZ)
        wv2, wi2 = h.sparse_posterior()
        assert np.array_equal(wv2, wv) and np.array_equal(wi2, wi)
    finally:
        h.close()


def test_noise_below_the_clamp():
    """noise = 1e-9 < 1e-8: beta = 1e8 (an unclamped 1e9 would move the LML by O(N)), and dnoise is the reference's formula value."""
    h, r = _handle("S1", "Mat32", True, 1e-9)
    try:
        assert float(r["ld"]["beta"]) == pytest.approx(1e8, rel=1e-15)
        lml, (dv, dl, dn, dZ) = h.sparse_fit_grad(3)
        got = dict(lml=lml, dvariance=dv, dlengthscale=dl, dnoise=dn, dZ=dZ)
        for q in ["lml"] + GRAD_Q:
            _check("S1 Mat32 noise 1e-9: %s" % q, got[q], r["f64"][q], r["ld"][q])
        m, v = h.sparse_predict(r["Xs"][:5], include_noise=True)
        _check("S1 Mat32 noise 1e-9: var + noise", v[:, 0], r["f64"]["pred1"]["var"][:5], r["ld"]["pred1"]["var"][:5])
    finally:
        h.close()


# ---- prediction ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fam,ard", RUNS, ids=IDS)
def test_predictions_against_long_double(case, fam, ard):
    h, r = _handle(case, fam, ard)
    try:
        _, jk, jb = h.sparse_fit()
        _conditions(r, (jk, jb))
        tag = "%s %s %s" % (case, fam, "ard" if ard else "iso")
        full = {}
        for inc in (True, False):
            m, v, dm, dvx = h.sparse_predict(r["Xs"], include_noise=inc, grad=True)
            full[inc] = (m, v, dm, dvx)
            for q, g in zip(PRED_Q, (m, v[:, 0], dm, dvx)):
                _check("%s: 130 rows noise=%d %s" % (tag, inc, q), g, r["f64"]["pred%d" % inc][q], r["ld"]["pred%d" % inc][q])
        # the same table twice: the same bits; a row alone, among five, without gradients: the bits it has in the 130-row table
        again = h.sparse_predict(r["Xs"], include_noise=True, grad=True)
        assert all(np.array_equal(a, b) for a, b in zip(again, full[True]))
        for rows in (slice(0, 1), slice(0, 5), slice(129, 130), slice(127, 130)):
            sub = h.sparse_predict(r["Xs"][rows], include_noise=True, grad=True)
            assert all(np.array_equal(a, b[rows]) for a, b in zip(sub, full[True])), rows
            m, v = h.sparse_predict(r["Xs"][rows], include_noise=False)
            assert np.array_equal(m, full[False][0][rows]) and np.array_equal(v, full[False][1][rows])
        _check("%s: fmin" % tag, h.sparse_fmin(), r["f64"]["fmin"], r["ld"]["fmin"])
    finally:
        h.close()


# ---- the exact model is untouched ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["S2", "S1"])
def test_exact_model_bits_survive_interleaved_sparse_calls(case):
    """S2: two outputs over padded tiles; S1: one output, so that the cached fmin is part of the comparison.  Compared: the fit's
    scalars, the posterior of the resident candidates, alpha, fmin (P = 1), the factor and Ky^-1 built from the inverse factor."""
    r = _ref(case, "Mat52", True)
    one = r["Y"].shape[1] == 1

    def exact(h):
        fit = h.fit()
        h.set_candidates(r["Xs"])
        return fit, h.predict(include_noise=True), h.alpha(), h.fmin() if one else None

    def setup():
        h = _lib.Handle(0)
        h.set_option("mc_max", 128)
        h.set_data(r["X"], r["Y"])
        h.set_params(KID["Mat52"], True, R.VARIANCE, r["ls"], R.NOISE)
        return h

    fresh = setup()
    want = exact(fresh)
    want_chol, want_wi = fresh.chol(), fresh.woodbury_inv()
    fresh.close()
    h = setup()
    try:
        first = exact(h)
        h.sparse_set_inducing(r["Z"])
        h.sparse_fit()
        m1, v1 = h.predict(include_noise=True)                  # the resident candidates and their posterior between sparse calls
        f1 = h.fmin() if one else None                          # the cached fmin, read between sparse calls
        h.sparse_fit_grad(3)
        h.sparse_fmin()
        h.sparse_predict(r["Xs"][:7], grad=True)
        a1 = h.alpha()
        chol1, wi1 = h.chol(), h.woodbury_inv()                 # the factor, and Ky^-1 through the inverse factor
        h.sparse_posterior()
        second = exact(h)
        h.sparse_predict(r["Xs"], grad=True)
        m2, v2 = h.predict(include_noise=True)
        assert one == (want[3] is not None) and f1 == want[3]
        assert np.array_equal(chol1, want_chol) and np.array_equal(wi1, want_wi)
        h.sparse_fit()
        assert np.array_equal(h.woodbury_inv(), want_wi) and (not one or h.fmin() == want[3])
        for got in (first, second):
            assert got[0] == want[0] and got[3] == want[3]
            assert np.array_equal(got[1][0], want[1][0]) and np.array_equal(got[1][1], want[1][1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(m1, want[1][0]) and np.array_equal(v1, want[1][1]) and np.array_equal(a1, want[2])
        assert np.array_equal(m2, want[1][0]) and np.array_equal(v2, want[1][1])
    finally:
        h.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_return_codes():
    lib = _lib.load()
    r = _ref("S1", "rbf", True)
    D = 3
    d = ctypes.c_double()
    buf = np.zeros(4096)
    p = _lib.dptr(buf)
    Z = np.ascontiguousarray(r["Z"])

    def ptr(a):
        return _lib.dptr(np.ascontiguousarray(a))

    assert lib.gp_sparse_set_inducing(None, ptr(Z), 10) == _lib.GP_ERR_ARG
    h = _lib.Handle(0)
    try:
        g = h.h
        assert lib.gp_sparse_set_inducing(g, ptr(Z), 10) == _lib.GP_ERR_STATE              # no data
        assert lib.gp_sparse_fit(g, 5, None, None, None) == _lib.GP_ERR_STATE
        h.set_data(r["X"], r["Y"])
        assert lib.gp_sparse_fit(g, 5, None, None, None) == _lib.GP_ERR_STATE              # no parameters
        h.set_params(KID["rbf"], True, R.VARIANCE, r["ls"], R.NOISE)
        assert lib.gp_sparse_fit(g, 5, None, None, None) == _lib.GP_ERR_STATE              # no inducing inputs
        assert b"gp_sparse_set_inducing" in lib.gp_last_error()
        assert lib.gp_sparse_predict(g, p, 1, 1, p, p, None, None) == _lib.GP_ERR_STATE
        assert lib.gp_sparse_set_inducing(g, None, 10) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_set_inducing(g, p, 0) == _lib.GP_ERR_ARG
        big = np.zeros((2049, D))
        assert lib.gp_sparse_set_inducing(g, ptr(big), 2049) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_set_inducing(g, ptr(big[:2048]), 2048) == 0
        h.sparse_set_inducing(Z)
        for call in (lambda: lib.gp_sparse_predict(g, p, 1, 1, p, p, None, None), lambda: lib.gp_sparse_posterior(g, p, p),
                     lambda: lib.gp_sparse_fmin(g, ctypes.byref(d))):
            assert call() == _lib.GP_ERR_STATE                                             # no sparse fit yet
        assert lib.gp_sparse_fit_grad(g, 5, None, None, p, ctypes.byref(d), p) == _lib.GP_ERR_ARG   # null gradient pointers
        assert lib.gp_sparse_fit(g, 5, None, None, None) == 0
        assert lib.gp_sparse_predict(g, None, 1, 1, p, p, None, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_predict(g, p, 0, 1, p, p, None, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_posterior(g, None, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_fmin(g, None) == _lib.GP_ERR_ARG
        # the fit is dropped by new parameters and by new data; Z survives both
        h.set_params(KID["rbf"], True, R.VARIANCE, r["ls"], 2 * R.NOISE)
        assert lib.gp_sparse_fmin(g, ctypes.byref(d)) == _lib.GP_ERR_STATE
        assert lib.gp_sparse_fit(g, 5, None, None, None) == 0
        h.set_data(r["X"][:50], r["Y"][:50])
        assert lib.gp_sparse_fmin(g, ctypes.byref(d)) == _lib.GP_ERR_STATE
        assert lib.gp_sparse_fit(g, 5, None, None, None) == 0 and h.sparse_posterior()[0].shape == (10, 1)
        # the Gower option and an output warp are refused
        h.set_gower(np.zeros(D, dtype=np.int32), np.ones(D))
        assert lib.gp_sparse_fit(g, 5, None, None, None) == _lib.GP_ERR_STATE
        h.set_gower()
        h.set_output_warp(np.array([[1.0, 1.0, 0.0]]), 1.0)
        assert lib.gp_sparse_fit(g, 5, None, None, None) == _lib.GP_ERR_STATE
        h.set_output_warp(None)
        assert lib.gp_sparse_fit(g, 5, None, None, None) == 0
        # P > 16 for the gradient call only
        Y17 = np.tile(r["Y"], (1, 17))
        h.set_data(r["X"], Y17)
        assert lib.gp_sparse_fit(g, 5, None, None, None) == 0
        assert lib.gp_sparse_fit_grad(g, 5, None, ctypes.byref(d), p, ctypes.byref(d), p) == _lib.GP_ERR_ARG
        assert h.sparse_predict(r["Xs"][:3])[0].shape == (3, 17)
    finally:
        h.close()


# ---- model level -----------------------------------------------------------------------------------------------------------------
def _model_data(N=60, D=2, seed=21):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    return X, Y


def test_model_objective_gradient_and_optimize():
    X, Y = _model_data()
    np.random.seed(3)
    m = gpo.models.SparseGPRegression(X, Y, kernel=gpo.kern.Matern52(2, ARD=True), num_inducing=8)
    try:
        m.kern.lengthscale.set([0.4, 0.6])
        m.likelihood.variance.set(0.05)
        assert m.num_inducing == 8 and m.optimizer_array.size == 8 * 2 + 1 + 2 + 1
        x = m.optimizer_array.copy()
        f0, g0 = m._obj_grad(x)
        num = np.empty_like(x)
        for i in range(x.size):
            e = np.zeros_like(x)
            e[i] = 1e-5
            num[i] = (m._obj_grad(x + e)[0] - m._obj_grad(x - e)[0]) / 2e-5
        err = float(np.max(np.abs(num - g0)) / np.max(np.abs(g0)))
        print("objective %.6f; gradient against central differences: %.2e of the largest entry %.3e" % (f0, err, np.max(np.abs(g0))))
        assert err <= 1e-5
        m.optimizer_array = x
        start = m.objective_function()
        m.optimize(max_iters=20)
        end = m.objective_function()
        print("optimize(max_iters=20): %.6f -> %.6f" % (start, end))
        assert end <= start
        mean, var = m.predict(X[:9])
        assert mean.shape == (9, 1) and var.shape == (9, 1) and np.all(var > 0)
        wv, wi = m.posterior.woodbury_vector, m.posterior.woodbury_inv
        assert wv.shape == (8, 1) and wi.shape == (8, 8)
    finally:
        m.close()


def test_bayesian_optimization_over_a_sparse_model():
    X0, Y0 = _model_data(N=30)
    domain = [{'name': 'x%d' % i, 'type': 'continuous', 'domain': (0.0, 1.0)} for i in range(2)]
    np.random.seed(5)
    model = gpo.GPModel(sparse=True, num_inducing=8, exact_feval=True, max_iters=50, optimize_restarts=1, verbose=False)
    bo = gpo.BayesianOptimization(lambda x: np.sin(3 * np.atleast_2d(x).sum(1))[:, None], domain, X=X0, Y=Y0, model=model,
                                  acquisition_type='EI')
    x1 = bo.suggest_next_locations()
    print("first suggestion", x1)
    assert x1.shape == (1, 2) and np.all((x1 >= 0.0) & (x1 <= 1.0))
    assert isinstance(model.model, gpo.models.SparseGPRegression) and model.model.Z_values.shape == (8, 2)
    assert not bo.acquisition._device_ok()
    bo.X = np.vstack([bo.X, x1])
    bo.Y = np.vstack([bo.Y, np.sin(3 * x1.sum(1))[:, None]])
    x2 = bo.suggest_next_locations()
    print("second suggestion", x2)
    assert x2.shape == (1, 2) and np.all((x2 >= 0.0) & (x2 <= 1.0))
    assert model.model.Z_values.shape == (8, 2) and model.model.num_data == 31
    model.model.close()
