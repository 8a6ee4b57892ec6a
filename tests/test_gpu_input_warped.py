"""GPU: the input-warped GP -- the Kumaraswamy warp of a candidate table on the device (gp_set_candidates_kumar,
csrc/gradx.hip), ``InputWarpedGP`` (gradient, checkgrad, predictions, optimize) and the BO surface
``model_type='input_warped_GP'``.

Reference: GPy/GPy/util/input_warping_functions.py:60-258, GPy/GPy/models/input_warped_gp.py,
GPyOpt/GPyOpt/models/input_warped_gpmodel.py, GPyOpt/GPyOpt/util/arguments_manager.py:137-147.

Yardsticks.  The warp kernel: the formula in ``np.longdouble``; bound per (a, b) pair = four times the largest error of NumPy's
own float64 evaluation against those long-double values on the same inputs, floor 1e-15 (NumPy's error is 1e-16 to 8e-16 for
three of the pairs and 6.4e-13 for (4, 0.2), where (1 - u^a)^b amplifies the cancellation near u = 1; the device ``pow`` may be
an ulp or two off NumPy's, twice in a chain, hence four; a wrong pairing, dimension or epsilon is off by 1e-7 or more).  Route
against route (device warp against host warp): 1e-9 of the largest entry, the figure of tests/test_gpu_rows.py.  The model:
the oracle composed here -- the oracle's GP at the warped inputs (warped in NumPy from the closed form), its hyper-gradients,
and sum_i dL_dX[i, q] dw/da, dw/db for the warping parameters -- at the north star, 1e-6 of the largest entry.
Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd.parameterization import Logexp, Logistic
from oracle import cpu_ref as O

import _kernel_families as KF

pytestmark = pytest.mark.gpu

EPS = 1e-6
TOL = 1e-6
N, D = 300, 3
VAR, NOISE = 1.3, 1e-2
LS = np.array([0.4, 0.7, 1.1])
WA, WB = np.array([0.6, 1.7, 1.0]), np.array([2.2, 0.8, 1.0])


def _err(what, got, ref, tol, scale=None):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), what
    s = float(np.max(np.abs(ref))) if scale is None else float(scale)
    e = float(np.max(np.abs(got - ref))) / max(s, 1e-300)
    print("%-44s err %.3e  tol %.1e" % (what, e, tol))
    assert e <= tol, (what, e, tol)


def _kumar(X, a, b, lo, hi, cols, dtype=np.float64):
    """The closed form, column by column, in ``dtype``; lo / hi already widened."""
    X = np.asarray(X, dtype=dtype)
    out = X.copy()
    for q in cols:
        u = (X[:, q] - dtype(lo[q])) / (dtype(hi[q]) - dtype(lo[q]))
        out[:, q] = 1 - np.power(1 - np.power(u, dtype(a[q])), dtype(b[q]))
    return out


# ---- the warp kernel -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table():
    rng = np.random.default_rng(11)
    Xs = rng.uniform(0, 1, (130, 3))
    Xs[0], Xs[1] = 0.0, 1.0              # u = eps-scale and 1 - eps-scale
    Xs.setflags(write=False)
    return Xs


@pytest.fixture(scope="module")
def hw():
    """A handle with three-dimensional data and candidate chunks of 128 rows: the 130-row table crosses a chunk boundary."""
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (N, D))
    Y = (np.sin(3 * X.sum(1)) + 0.1 * rng.standard_normal(N))[:, None]
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", 0)
    hd.set_option("mc_max", 128)
    hd.set_data(X, Y)
    hd.set_params(_lib.GP_KERNEL_MATERN52, True, VAR, LS, NOISE)
    hd.fit()
    yield hd
    hd.close()


@pytest.mark.parametrize("a,b", [(1.0, 1.0), (0.3, 2.5), (4.0, 0.2), (9.5, 9.5)])
def test_warp_kernel_against_long_double(hw, a, b):
    Xs = _table()
    lo, hi = np.zeros(3) - EPS, np.ones(3) + EPS
    av, bv = np.array([a, 7.7, a]), np.array([b, 0.123, b])      # (the middle entries belong to a column that is not warped)
    exact = _kumar(Xs, av, bv, lo, hi, (0, 2), np.longdouble)
    host = _kumar(Xs, av, bv, lo, hi, (0, 2))
    numpy_err = float(np.max(np.abs(host.astype(np.longdouble) - exact)))
    bound = max(4.0 * numpy_err, 1e-15)
    got = hw.set_candidates_kumar(Xs, [1, 0, 1], av, bv, lo, hi, want_warped=True)
    assert got.shape == Xs.shape and np.all(np.isfinite(got))
    assert got[:, 1].tobytes() == Xs[:, 1].tobytes(), "the column that is not warped comes back bit-equal"
    dev_err = float(np.max(np.abs(got.astype(np.longdouble) - exact)))
    print("kumar (a, b) = (%g, %g): device %.3e  NumPy %.3e  bound %.3e" % (a, b, dev_err, numpy_err, bound))
    assert dev_err <= bound
    assert np.all(got[:, [0, 2]] >= 0.0) and np.all(got[:, [0, 2]] <= 1.0)
    assert hw.M == 130


def test_warp_outside_the_bounds_and_refused_arguments(hw):
    lo, hi = np.zeros(3) - EPS, np.ones(3) + EPS
    Xs = np.array([[-0.5, 0.2, 0.3], [0.5, 0.2, 1.5], [0.5, -4.0, 0.5]])
    av, bv = np.array([0.3, 1.0, 0.3]), np.array([2.5, 1.0, 2.5])
    with np.errstate(invalid="ignore"):
        ref = _kumar(Xs, av, bv, lo, hi, (0, 2))
    got = hw.set_candidates_kumar(Xs, [1, 0, 1], av, bv, lo, hi, want_warped=True)
    assert np.isnan(ref[0, 0]) and np.isnan(ref[1, 2])                      # NumPy's power, as the reference sees it
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert got[2].tobytes()[8:16] == Xs[2].tobytes()[8:16]
    _err("rows inside the bounds", got[2], ref[2], 1e-14, 1.0)
    ok = dict(a=np.ones(3), b=np.ones(3), xmin=lo, xmax=hi)
    for key, bad in (("a", 0.0), ("a", -1.0), ("b", np.nan), ("b", np.inf), ("a", np.inf)):
        args = {k: v.copy() for k, v in ok.items()}
        args[key][2] = bad
        with pytest.raises(ValueError, match="positive and finite"):
            hw.set_candidates_kumar(Xs, [1, 0, 1], args["a"], args["b"], args["xmin"], args["xmax"])
    args = {k: v.copy() for k, v in ok.items()}
    args["xmax"][0] = args["xmin"][0]
    with pytest.raises(ValueError, match="xmax <= xmin"):
        hw.set_candidates_kumar(Xs, [1, 0, 1], args["a"], args["b"], args["xmin"], args["xmax"])
    args["a"][1] = -3.0                                                      # a column that is not warped is not read
    args["xmax"][0] = 1.0
    hw.set_candidates_kumar(Xs, [1, 0, 1], args["a"], args["b"], args["xmin"], args["xmax"])


def test_predictions_after_the_device_warp(hw):
    Xs = _table()
    lo, hi = np.zeros(3) - EPS, np.ones(3) + EPS
    hw.set_candidates_kumar(Xs, [1, 0, 1], WA, WB, lo, hi)
    m1, v1 = hw.predict(True)
    hw.set_candidates(_kumar(Xs, WA, WB, lo, hi, (0, 2)))
    m0, v0 = hw.predict(True)
    _err("mean: device warp against host warp", m1, m0, 1e-9)
    _err("variance: device warp against host warp", v1, v0, 1e-9)


# ---- the model -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem():
    rng = np.random.default_rng(20262)
    X = rng.uniform(0, 1, (N, D))
    Y = (np.sin(3 * X.sum(1)) + 0.1 * rng.standard_normal(N))[:, None]
    Xs = rng.uniform(0, 1, (130, D))
    for a in (X, Y, Xs):
        a.setflags(write=False)
    return X, Y, Xs


LO, HI = np.zeros(D) - EPS, np.ones(D) + EPS


def _du(X):
    return (np.asarray(X, dtype=float) - LO) / (HI - LO)


@functools.lru_cache(maxsize=None)
def _oracle():
    """The oracle GP at the warped training inputs, its natural gradients composed with the warp's, computed once."""
    X, Y, Xs = _problem()
    Xw = _kumar(X, WA, WB, LO, HI, range(D))
    kern = KF.make("Mat52", D, VAR, LS, True, direct=True)
    gp = O.OracleGP(Xw, Y, kern, NOISE)
    dv, dl, dn = gp.gradients()
    dL_dX = kern.gradients_X(gp.posterior["dL_dK"], Xw)
    u = _du(X)
    ua = np.power(u, WA)
    dw_da = WB * np.power(1 - ua, WB - 1) * ua * np.log(u)
    dw_db = -np.power(1 - ua, WB) * np.log(1 - ua)
    da, db = np.sum(dL_dX * dw_da, 0), np.sum(dL_dX * dw_db, 0)
    natural = np.r_[dv, dl, dn, np.c_[da, db].ravel()]
    natural.setflags(write=False)
    return gp, natural


def _model():
    X, Y, _ = _problem()
    m = gpo.models.InputWarpedGP(X, Y, kernel=gpo.kern.Matern52(D, VAR, LS, ARD=True), Xmin=np.zeros(D), Xmax=np.ones(D))
    m.likelihood.variance.set(NOISE)
    for q in range(D):
        m.warping_function.params[q][0].set(WA[q])
        m.warping_function.params[q][1].set(WB[q])
    return m


@pytest.fixture(scope="module")
def model():
    m = _model()
    yield m
    m.close()


def test_gradient_against_the_composed_oracle(model):
    gp, natural = _oracle()
    lml = model.log_likelihood()
    print("LML %.12f oracle %.12f" % (lml, gp.log_likelihood()))
    assert abs(lml - gp.log_likelihood()) <= 1e-8 * abs(gp.log_likelihood())
    names = model.parameter_names_flat().tolist()
    assert [n.split(".")[-1] for n in names[-6:]] == ["a0", "b0", "a1", "b1", "a2", "b2"], names
    g = model.gradient
    print("natural gradient", g, "\noracle          ", natural)
    _err("InputWarpedGP.gradient", g, natural, TOL)
    # a new parameter vector goes down as ONE gp_fit_grad_x: the same numbers
    model.kern.variance.set(VAR)
    assert model._dirty
    _err("InputWarpedGP.gradient through gp_fit_grad_x", model.gradient, natural, TOL)
    assert "lml_grad_x" in [p["name"] for p in model._h.phases()]


def test_objective_adds_the_priors_in_closed_form(model):
    gp, natural = _oracle()
    ab = np.c_[WA, WB].ravel()
    sigma2 = 0.75 ** 2
    lnpdf = -0.5 * np.log(2 * np.pi * sigma2) - 0.5 * np.log(ab) ** 2 / sigma2 - np.log(ab)
    lnpdf_grad = -(np.log(ab) / sigma2 + 1.0) / ab
    f0 = -(gp.log_likelihood() + lnpdf.sum())
    f = model.objective_function()
    print("objective %.12f composed %.12f" % (f, f0))
    assert abs(f - f0) <= 1e-8 * abs(f0)
    nat = natural.copy()
    nat[-6:] += lnpdf_grad
    values = np.r_[VAR, LS, NOISE, ab]
    factor = np.r_[-np.expm1(-values[:5]), ab * (10.0 - ab) / 10.0]        # Logexp: 1 - exp(-f); Logistic(0, 10): f (10 - f) / 10
    assert isinstance(model.kern.variance.transform, Logexp) and isinstance(model.warping_function.params[0][0].transform, Logistic)
    _err("objective_function_gradients", model.objective_function_gradients(), -nat * factor, TOL)


def test_checkgrad(model):
    np.random.seed(3)
    assert model.checkgrad()
    assert model.checkgrad(verbose=True)


@pytest.mark.parametrize("rows", [5, 130])
def test_predict_and_predictive_gradients(model, rows):
    gp, _ = _oracle()
    _, _, Xs = _problem()
    Xs = Xs[:rows]
    Xsw = _kumar(Xs, WA, WB, LO, HI, range(D))
    u = _du(Xs)
    J = WA * WB * np.power(u, WA - 1) * np.power(1 - np.power(u, WA), WB - 1) / (HI - LO)
    mu0, var0 = gp.predict(Xsw)
    dm0, dv0 = gp.predictive_gradients(Xsw)
    fused0 = model._h.rows_stats()["fused"]
    mu, var = model.predict(Xs)
    _err("predict mean, %d rows" % rows, mu, mu0, TOL)
    _err("predict variance, %d rows" % rows, var, var0, TOL)
    _, var_nl = model.predict_noiseless(Xs)
    _err("predict_noiseless variance, %d rows" % rows, var_nl, gp.predict_noiseless(Xsw)[1], TOL)
    dm, dv = model.predictive_gradients(Xs)
    _err("d mean / dx (un-warped), %d rows" % rows, dm, dm0 * J[:, :, None], TOL)
    _err("d var / dx (un-warped), %d rows" % rows, dv, dv0 * J, TOL)
    if rows <= 8:
        assert model._h.rows_stats()["fused"] > fused0
    else:
        _err("transform_data on the device", model.transform_data(Xs, test_data=True, device=True), Xsw, 1e-12, 1.0)


def test_optimize_learns_a_known_warp():
    """Data generated through w(x) = x^0.4 (a = 0.4, b = 1) in one dimension: from a = b = 1 the search ends at a higher log
    posterior than it started, and at a higher LML than the un-warped GP optimised from the same kernel start."""
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 1, (80, 1))
    Y = np.sin(9.0 * X ** 0.4) + 0.05 * rng.standard_normal((80, 1))
    m = gpo.models.InputWarpedGP(X, Y, kernel=gpo.kern.RBF(1, 1.0, 0.3), Xmin=[0.0], Xmax=[1.0])
    g = gpo.models.GPRegression(X, Y, kernel=gpo.kern.RBF(1, 1.0, 0.3), noise_var=1.0)
    try:
        start = -m.objective_function()
        m.optimize(max_iters=200)
        end = -m.objective_function()
        g.optimize(max_iters=200)
        a, b = m.warping_function.values()
        print("log posterior %.4f -> %.4f; LML warped %.4f, un-warped %.4f; a = %.3f b = %.3f" %
              (start, end, m.log_likelihood(), g.log_likelihood(), a[0], b[0]))
        assert np.isfinite(end) and end > start
        assert m.log_likelihood() > g.log_likelihood()
    finally:
        m.close()
        g.close()


def test_bo_surface_suggests_through_the_host_adapter():
    rng = np.random.default_rng(5)
    np.random.seed(5)
    domain = [{'name': 'x', 'type': 'continuous', 'domain': (0.0, 2.0)}, {'name': 'y', 'type': 'continuous', 'domain': (-1.0, 1.0)}]
    X = np.c_[rng.uniform(0, 2, 40), rng.uniform(-1, 1, 40)]
    Y = (np.sin(4 * np.sqrt(X[:, 0])) + X[:, 1] ** 2 + 0.05 * rng.standard_normal(40))[:, None]
    bo = gpo.BayesianOptimization(f=None, domain=domain, X=X, Y=Y, model_type='input_warped_GP')
    x = bo.suggest_next_locations()
    print("suggested", x)
    assert x.shape == (1, 2) and np.all(np.isfinite(x))
    assert 0.0 <= x[0, 0] <= 2.0 and -1.0 <= x[0, 1] <= 1.0
    assert isinstance(bo.model, gpo.models.InputWarpedGPModel) and isinstance(bo.model.model, gpo.models.InputWarpedGP)
    assert not bo.acquisition._device_ok()
    stats = bo.model.model._h.rows_stats()
    print("rows stats", stats)
    assert stats["fused"] > 0
    bo.model.model.close()
