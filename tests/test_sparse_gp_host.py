"""Host side of the sparse GP (no GPU): the oracle of tests/_sparse_ref.py held to central differences of its own LML, to the
exact model in the Z = X limit and -- where the reference tree is at hand -- to the reference's own functions; the conditions
of the GPU suite's cases; and the host classes' logic over a handle answered by the oracle.

Reference: GPy/GPy/inference/latent_function_inference/var_dtc.py:66-277, GPy/GPy/core/sparse_gp.py:41-119,
GPy/GPy/models/sparse_gp_regression.py:33-66, GPyOpt/GPyOpt/models/gpmodel.py:31-76.

Bounds.
* Central differences (step 1e-6, 1e-7 for the noise; Z moved off the data rows: across a coincident pair the Exponential's
  difference quotient straddles the kink and is not the reference's value).  The bound on the float64 quotient's distance
  from the true derivative is taken from difference quotients alone: the truncation c h^2 is |q(2h) - q(h)| / 3 of the
  long-double oracle's quotients at h and 2 h, and the rounding is the float64 LML's distance from the long-double LML at the
  two evaluation points, over 2 h.  The float64 analytic gradient has to lie within twice their sum of the float64 quotient
  (plus 1e-12 of it).  No analytic gradient, in either precision, enters the bound, and a second test shows the check failing
  on gradients that are wrong by 1e-6 of their size.
* Z = X: to first order the sparse LML differs from the exact one by the jitter's trace term, 0.5 P beta N 1e-8 = 2.4e-5 at
  N = 96, beta = 50.  The issue's figures, measured on its author's prototype: 1.7e-5 (Matern-3/2), 2.7e-5 (Exponential);
  posterior mean / variance 1.4e-8 / 1.0e-8 from ``OracleGP``.  Measured here with this oracle: 2.1e-5 and 2.3e-5; 7.2e-9 / 4.8e-9
  and 4.0e-9 / 1.5e-10.  Asserted: the LML within 4x the first-order term, the posterior within 10x the issue's
  figures.
* The pin to the reference: the oracle's pieces against ``_compute_dL_dpsi``, ``_compute_dL_dR`` and
  ``_compute_log_marginal_likelihood`` compiled out of the reference file's syntax tree, at 1e-13 of the largest entry (the same
  float64 operations in the same order up to BLAS).
Every figure is printed before it is asserted.
"""
import ast
import functools
import os

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

import _kernel_families as KF
import _sparse_ref as R

FAMS = ["rbf", "Mat52", "Mat32", "Exponential"]
KID = {0: "rbf", 1: "Mat52", 2: "Mat32", 3: "Exponential"}
REF_VARDTC = "/root/reference/GPy/GPy/inference/latent_function_inference/var_dtc.py"


def _small(seed=5, N=40, Mz=6, D=2, P=2):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] * np.array([1.0, 0.6])[:P] + 0.1 * rng.standard_normal((N, P))
    Z = X[:Mz] + 0.05 * rng.standard_normal((Mz, D))      # off the data rows
    return X, Y, Z


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_float64_covariances_are_the_oracles(fam):
    X, _, Z = _small()
    ls = np.array([0.3, 0.5])
    k = R.Kern(fam, 2, 1.3, ls, True, R.F64)
    ko = KF.make(fam, 2, 1.3, ls, True, direct=True)
    for a, b in ((X, Z), (Z, None)):
        e = np.max(np.abs(k.K(a, b) - ko.K(a, b)))
        print("%s K: %.2e" % (fam, e))
        assert e <= 4e-16 * 1.3
    W = np.random.RandomState(1).standard_normal((X.shape[0], Z.shape[0]))
    dv, dl = k.update_gradients_full(W, X, Z)
    dvo, dlo = ko.update_gradients_full(W, X, Z)
    gx, gxo = k.gradients_X(W.T, Z, X), ko.gradients_X(W.T, Z, X)
    for what, got, ref in (("dvariance", dv, dvo), ("dlengthscale", dl, dlo), ("gradients_X", gx, gxo)):
        e = np.max(np.abs(np.asarray(got) - np.asarray(ref))) / np.max(np.abs(ref))
        print("%s %s: %.2e" % (fam, what, e))
        assert e <= 1e-13


def _lml(fam, X, Z, Y, var, ls, noise, lin):
    return R.inference(fam, X, Z, Y, var, ls, True, noise, lin, grads=False)["lml"]


_CD_VAR, _CD_LS, _CD_NOISE = 1.3, np.array([0.3, 0.5]), 2e-2


@functools.lru_cache(maxsize=None)
def _difference_quotients(fam):
    """Per parameter (variance, lengthscales, noise, Z row-major): the float64 oracle's central difference quotient of its own
    LML at step h, and a bound on that quotient's distance from the true derivative which no analytic gradient enters:
    truncation from the long-double quotients at h and 2 h (q(h) = f' + c h^2 + O(h^4), so |q(2h) - q(h)| / 3 is c h^2), rounding
    from the float64 LML's distance to the long-double LML at the two evaluation points over 2 h."""
    X, Y, Z = _small()

    def at(i, h, lin):
        v, l, n, z = _CD_VAR, _CD_LS.copy(), _CD_NOISE, Z.copy()
        if i == 0:
            v = v + h
        elif i <= 2:
            l[i - 1] += h
        elif i == 3:
            n = n + h
        else:
            z.reshape(-1)[i - 4] += h
        return _lml(fam, X, z, Y, v, l, n, lin)

    names = ["variance", "lengthscale[0]", "lengthscale[1]", "noise"] + ["Z[%d,%d]" % (m, q) for m in range(Z.shape[0]) for q in range(2)]
    out = []
    for i, name in enumerate(names):
        h = 1e-7 if name == "noise" else 1e-6
        up64, dn64, upld, dnld = at(i, h, R.F64), at(i, -h, R.F64), at(i, h, R.LD), at(i, -h, R.LD)
        q64, qld = float(up64 - dn64) / (2 * h), (upld - dnld) / (2 * h)
        qld2 = (at(i, 2 * h, R.LD) - at(i, -2 * h, R.LD)) / (4 * h)
        truncation = abs(float(qld2 - qld)) / 3
        rounding = float(abs(up64 - upld) + abs(dn64 - dnld)) / (2 * h)
        out.append((name, q64, truncation, rounding))
    return out


def _against_quotients(fam, analytic):
    """The worst |analytic - quotient| / bound over the parameters, bound = 2 (truncation + rounding) + 1e-12 |quotient|."""
    worst = 0.0
    for (name, q64, truncation, rounding), a in zip(_difference_quotients(fam), analytic):
        bound = 2 * (truncation + rounding) + 1e-12 * abs(q64)
        err = abs(float(a) - q64)
        worst = max(worst, err / bound)
        print("%-12s %-16s analytic %+.9e quotient %+.9e |diff| %.2e bound %.2e (truncation %.1e rounding %.1e)"
              % (fam, name, float(a), q64, err, bound, truncation, rounding))
    return worst


def _analytic(g):
    return np.concatenate([[float(g["dvariance"])], np.asarray(g["dlengthscale"], dtype=float), [float(g["dnoise"])],
                           np.asarray(g["dZ"], dtype=float).reshape(-1)])


@pytest.mark.parametrize("fam", FAMS)
def test_analytic_gradients_against_central_differences_of_the_lml(fam):
    X, Y, Z = _small()
    g = _analytic(R.inference(fam, X, Z, Y, _CD_VAR, _CD_LS, True, _CD_NOISE, R.F64))
    worst = _against_quotients(fam, g)
    print("%s worst error / bound %.3f" % (fam, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("fam", FAMS)
def test_the_central_difference_check_rejects_wrong_gradients(fam):
    """The same check on gradients that are wrong by a little: each of dvariance x (1 + 1e-6), dlengthscale x (1 + 1e-6),
    dnoise + 1e-2 (of 1e4 .. 1e5) and dZ x (1 + 1e-6) alone must fail it."""
    X, Y, Z = _small()
    g = _analytic(R.inference(fam, X, Z, Y, _CD_VAR, _CD_LS, True, _CD_NOISE, R.F64))
    for what, rows, change in (("dvariance", slice(0, 1), lambda v: v * (1 + 1e-6)), ("dlengthscale", slice(1, 3), lambda v: v * (1 + 1e-6)),
                               ("dnoise", slice(3, 4), lambda v: v + 1e-2), ("dZ", slice(4, None), lambda v: v * (1 + 1e-6))):
        bad = g.copy()
        bad[rows] = change(bad[rows])
        worst = _against_quotients(fam, bad)
        print("%s perturbed %s: worst error / bound %.1f" % (fam, what, worst))
        assert worst > 1.0, (fam, what)


@pytest.mark.parametrize("fam", ["Mat32", "Exponential"])
def test_every_data_row_an_inducing_input_is_the_exact_model(fam):
    N, D, noise = 96, 3, 0.02
    rng = np.random.RandomState(11)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    Xs = rng.uniform(0, 1, (20, D))
    ls = R.case_lengthscale(D, True)
    fit = R.inference(fam, X, X.copy(), Y, R.VARIANCE, ls, True, noise, R.F64, grads=False)
    mean, var = R.predict(fit, X, Xs, noise, False, R.F64, grads=False)
    exact = O.OracleGP(X, Y, KF.make(fam, D, R.VARIANCE, ls, True, direct=True), noise_var=noise)
    first_order = 0.5 * 1 * (1.0 / noise) * N * 1e-8
    d_lml = abs(float(fit["lml"]) - float(exact.log_likelihood()))
    em, ev = exact._raw_predict(Xs)
    d_mean, d_var = np.max(np.abs(mean - em)), np.max(np.abs(var - np.ravel(ev)))
    print("%s Z = X: |lml - exact| %.2e (first-order term %.2e); mean %.2e var %.2e" % (fam, d_lml, first_order, d_mean, d_var))
    assert fit["jitter_kmm"] == 0.0 and fit["jitter_b"] == 0.0
    assert d_lml <= 4 * first_order
    assert d_mean <= 10 * 1.4e-8 and d_var <= 10 * 1.0e-8


def _reference_functions():
    """``_compute_dL_dpsi``, ``_compute_dL_dR`` and ``_compute_log_marginal_likelihood`` compiled out of the reference file's
    syntax tree (module-level NumPy functions: they need np, dtrtrs and backsub_both_sides)."""
    tree = ast.parse(open(REF_VARDTC).read())
    want = {"_compute_dL_dpsi", "_compute_dL_dR", "_compute_log_marginal_likelihood"}
    mod = ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want], type_ignores=[])
    ns = {"np": np, "dtrtrs": O.dtrtrs, "backsub_both_sides": lambda L, X, transpose='left': R.backsub_both_sides(R.F64, L, X)}
    exec(compile(mod, REF_VARDTC, "exec"), ns)
    assert want <= set(ns)
    return ns


@pytest.mark.skipif(not os.path.exists(REF_VARDTC), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("fam", FAMS)
def test_pieces_against_the_references_own_functions(fam):
    ns = _reference_functions()
    X, Y, Z = _small()
    N, P = Y.shape
    Mz = Z.shape[0]
    f = R.inference(fam, X, Z, Y, 1.3, np.array([0.3, 0.5]), True, 2e-2, R.F64)
    beta = np.array([[float(f["beta"])]])       # precision[:, None] of var_dtc.py:82-83

    class Lik(object):
        size = 1

    psi0, psi1, psi2 = ns["_compute_dL_dpsi"](Mz, N, P, beta, f["Lm"], f["VVT_factor"], f["woodbury_vector"], f["DBi_plus_BiPBi"],
                                             f["psi1"], False, False)
    lml = ns["_compute_log_marginal_likelihood"](Lik(), N, P, beta, False, f["psi0"], f["A"], f["LB"], f["trYYT"], f["data_fit"], Y)
    dR = ns["_compute_dL_dR"](Lik(), False, False, f["LB"], f["LBi_Lmi_psi1Vf"], f["DBi_plus_BiPBi"], f["Lm"], f["A"], f["psi0"],
                              f["psi1"], beta, f["data_fit"], N, P, f["trYYT"], Y, f["VVT_factor"])
    assert psi2 is None
    for what, got, ref in (("dL_dpsi0", f["dL_dpsi0"], psi0), ("dL_dpsi1", f["dL_dpsi1"], psi1), ("lml", f["lml"], lml),
                           ("dL_dR", f["dnoise"], dR)):
        ref = np.asarray(ref, dtype=float)
        e = np.max(np.abs(np.asarray(got, dtype=float) - ref.reshape(np.shape(got)))) / np.max(np.abs(ref))
        print("%s %-10s %.2e" % (fam, what, e))
        assert e <= 1e-13


# ---- the GPU suite's cases -----------------------------------------------------------------------------------------------------
RUNS = [("S1", f, True) for f in FAMS] + [("S2", f, True) for f in FAMS] + [("S3", f, False) for f in FAMS] + \
       [("S5", f, False) for f in FAMS] + [("S4", f, a) for f in ("rbf", "Exponential") for a in (False, True)]


def test_conditions_of_the_gpu_cases():
    """cond(Kmm) <= 8.9e4, no ladder step on Kmm or B, smallest sparse predictive variance at the data >= 2.9e-3 (the 1e-15 clip
    is never reached), for every run of tests/test_gpu_sparse_gp.py."""
    for case, fam, ard in RUNS:
        X, Y, Z, _ = R.case_inputs(case)
        D = X.shape[1]
        f = R.inference(fam, X, Z, Y, R.VARIANCE, R.case_lengthscale(D, ard), ard, R.NOISE, R.F64, grads=False)
        cond = np.linalg.cond(f["Kmm"])
        vmin = R.predict(f, Z, X, R.NOISE, False, R.F64, grads=False)[1].min()
        print("%s %-12s ard=%d cond(Kmm) %.3g  jitter %g %g  min var %.3g" % (case, fam, ard, cond, f["jitter_kmm"], f["jitter_b"], vmin))
        assert cond <= 8.9e4 and f["jitter_kmm"] == 0.0 and f["jitter_b"] == 0.0 and vmin >= 2.9e-3
        half = Z.shape[0] // 2
        assert all(np.any(np.all(X == z, axis=1)) for z in Z[:half])          # the first half coincides with data rows


# ---- host logic over a handle answered by the oracle ---------------------------------------------------------------------------
class _OracleHandle(object):
    """What SparseGPRegression asks of _lib.Handle, answered by tests/_sparse_ref.py in float64 (no device)."""
    fits = 0

    def __init__(self, device=0):
        self.device, self.h = device, object()

    def close(self):
        self.h = None

    def set_option(self, name, value):
        pass

    def set_gower(self, *a):
        assert not a

    def set_data(self, X, Y):
        self.X, self.Y = np.array(X, dtype=float), np.array(Y, dtype=float)
        self.N, self.D, self.P = X.shape[0], X.shape[1], Y.shape[1]

    def set_params(self, kernel, ard, variance, lengthscale, noise):
        self.par = (KID[kernel], float(variance), np.array(lengthscale, dtype=float), bool(ard), float(noise))

    def sparse_set_inducing(self, Z):
        self.Z = np.array(Z, dtype=float)
        self.Mz = self.Z.shape[0]

    def _fit(self, grads):
        fam, var, ls, ard, noise = self.par
        type(self).fits += 1
        self.f = R.inference(fam, self.X, self.Z, self.Y, var, ls, ard, noise, R.F64, grads=grads)
        return self.f

    def sparse_fit(self, maxtries=5):
        f = self._fit(False)
        return float(f["lml"]), f["jitter_kmm"], f["jitter_b"]

    def sparse_fit_grad(self, nls, maxtries=5):
        f = self._fit(True)
        assert f["dlengthscale"].size == nls
        return float(f["lml"]), (float(f["dvariance"]), f["dlengthscale"], float(f["dnoise"]), f["dZ"])

    def sparse_posterior(self):
        return self.f["woodbury_vector"], self.f["woodbury_inv"]

    def sparse_predict(self, Xs, include_noise=True, grad=False):
        r = R.predict(self.f, self.Z, Xs, self.par[4], include_noise, R.F64, grads=grad)
        return (r[0], r[1][:, None]) + tuple(r[2:])

    def sparse_fmin(self):
        return float(R.fmin(self.f, self.X))


@pytest.fixture
def oracle_handle(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", _OracleHandle)
    _OracleHandle.fits = 0
    return _OracleHandle


def test_parameter_order_names_and_default_inducing_inputs(oracle_handle):
    X, Y, _ = _small(N=30)
    np.random.seed(123)
    m = gpo.models.SparseGPRegression(X, Y, num_inducing=4)
    np.random.seed(123)
    want = X[np.random.permutation(30)[:4]]
    assert np.array_equal(m.Z_values, want) and m.num_inducing == 4
    assert isinstance(m.kern, gpo.kern.RBF) and float(m.likelihood.variance) == 1.0 and m.name == "sparse_gp"
    names = list(m.parameter_names_flat())
    assert names[:8] == ["sparse_gp.inducing_inputs[[%d]]" % i for i in range(8)]
    assert names[8:] == ["sparse_gp.rbf.variance", "sparse_gp.rbf.lengthscale", "sparse_gp.Gaussian_noise.variance"]
    assert np.array_equal(m.param_array, np.concatenate([want.reshape(-1), [1.0, 1.0, 1.0]]))
    # Z is unconstrained: the optimiser sees its entries as they are
    assert np.array_equal(m.optimizer_array[:8], want.reshape(-1))
    # more inducing inputs than data rows: every row, as the reference's min(num_inducing, N)
    assert gpo.models.SparseGPRegression(X[:3], Y[:3], num_inducing=10).num_inducing == 3
    # a given Z is taken as it is; set_XY keeps it, set_Z replaces it (another count included)
    Zg = X[5:8] + 0.01
    m2 = gpo.models.SparseGPRegression(X, Y, kernel=gpo.kern.Matern32(2, ARD=True), Z=Zg)
    assert np.array_equal(m2.Z_values, Zg)
    m2.set_XY(X[:20], Y[:20])
    assert np.array_equal(m2.Z_values, Zg) and m2.num_data == 20
    m2.set_Z(X[:5])
    assert m2.num_inducing == 5 and m2.param_array.size == 5 * 2 + 1 + 2 + 1
    with pytest.raises(NotImplementedError):
        m2.predict(X[:2], full_cov=True)


def test_objective_gradient_and_one_fit_per_evaluation(oracle_handle):
    X, Y, Z = _small(N=30)
    m = gpo.models.SparseGPRegression(X, Y, kernel=gpo.kern.Matern52(2, ARD=True), Z=Z)
    m.kern.lengthscale.set([0.3, 0.5])
    m.likelihood.variance.set(0.05)
    x = m.optimizer_array.copy()
    before = oracle_handle.fits
    f0, g0 = m._obj_grad(x)
    assert oracle_handle.fits == before + 1                 # ONE device call for objective and gradient
    assert f0 == -m.log_likelihood() and oracle_handle.fits == before + 1
    worst = 0.0
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = 1e-6
        num = (m._obj_grad(x + e)[0] - m._obj_grad(x - e)[0]) / 2e-6
        worst = max(worst, abs(num - g0[i]) / max(abs(g0[i]), 1.0))
    print("transformed-space gradient against central differences: %.2e" % worst)
    assert worst <= 1e-5
    m.optimizer_array = x
    f_start = m.objective_function()
    m.optimize(max_iters=10)
    assert m.objective_function() <= f_start
    mean, var = m.predict(X[:3])
    assert mean.shape == (3, 2) and var.shape == (3, 1)
    dm, dv = m.predictive_gradients(X[:3])
    assert dm.shape == (3, 2, 2) and dv.shape == (3, 2)
    assert m.posterior.woodbury_vector.shape == (6, 2) and m.posterior.woodbury_inv.shape == (6, 6)
    q = m.predict_quantiles(X[:3])
    assert len(q) == 2 and q[0].shape == (3, 2)


def test_gpmodel_sparse_constructs_and_routes(oracle_handle):
    X, Y, _ = _small(N=30, P=1)
    np.random.seed(4)
    gm = gpo.GPModel(sparse=True, num_inducing=5, exact_feval=True, max_iters=0, verbose=False)
    assert gm.sparse and gm.num_inducing == 5
    gm.updateModel(X, Y, None, None)
    assert isinstance(gm.model, gpo.models.SparseGPRegression) and gm.model.num_inducing == 5
    assert isinstance(gm.model.kern, gpo.kern.Matern52)
    assert gm.model.likelihood.variance.is_fixed and float(gm.model.likelihood.variance) == 1e-6
    gb = gpo.GPModel(sparse=True, num_inducing=5, noise_var=0.3, max_iters=0)
    gb.updateModel(X, Y, None, None)
    assert float(gb.model.likelihood.variance) == 1.0                       # noise_var is not passed on (gpmodel.py:69-71)
    assert (gb.model.likelihood.variance.transform.lower, gb.model.likelihood.variance.transform.upper) == (1e-9, 1e6)
    mean, std = gm.predict(X[:4])
    assert mean.shape == (4, 1) and std.shape == (4, 1)
    m, s, dm, ds = gm.predict_withGradients(X[:4])
    assert dm.shape == (4, 2) and ds.shape == (4, 2)
    assert gm.get_fmin() == pytest.approx(float(gm.model.predict(X)[0].min()), abs=1e-12)
    acq = gpo.AcquisitionEI(gm, optimizer=None)
    assert not acq._device_ok()                                             # the host rule over predict / predict_withGradients
    assert acq.acquisition_function(X[:4]).shape == (4, 1)
    Z0 = gm.model.Z_values.copy()
    gm.updateModel(np.vstack([X, [[0.5, 0.5]]]), np.vstack([Y, [[0.1]]]), None, None)
    assert np.array_equal(gm.model.Z_values, Z0)                            # new data keep Z


def test_refusals(oracle_handle):
    with pytest.raises(ValueError, match="parallel_restarts"):
        gpo.GPModel(sparse=True, parallel_restarts=True)
    X, Y, _ = _small(N=30, P=1)
    with pytest.raises(NotImplementedError, match="outside the accelerated path"):
        gpo.BayesianOptimization(f=None, domain=[{'name': 'x%d' % i, 'type': 'continuous', 'domain': (0, 1)} for i in range(2)],
                                 X=X, Y=Y, model_type='sparseGP')
    with pytest.raises(ValueError):
        gpo.models.SparseGPRegression(X, Y, Z=np.zeros((2049, 2)))
