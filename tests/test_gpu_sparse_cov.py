"""GPU: the sparse GP's joint posterior -- csrc/sparse_cov.hip and csrc/api_sparse_cov.hip behind ``gp_sparse_predict_full_cov``,
``gp_sparse_posterior_samples``, ``gp_sparse_cov_set_points`` / ``gp_sparse_cov_between`` (include/gphip.h, "sparse GP"),
``SparseGPRegression`` (``full_cov``, ``posterior_samples_f``, ``posterior_covariance_between_points``) and entropy search over
``GPModel(sparse=True)``.

Reference: posterior.py:229-232 over ``_predictive_variable = Z`` restated in two precisions in tests/_sparse_cov_ref.py on the
fits of tests/_sparse_ref.py.  Runs: those of tests/test_gpu_sparse_gp.py (S1 / S2 ARD and S3 / S5 iso in all four families, S4 rbf
and Exponential iso and ARD), the 130-row ``Xs`` of ``case_inputs`` as the prediction set with mc_max = 256 (two tiles with
padding), the sub-tables M = 128 (one tile exactly), 5 and 1; for the between-points entry R in {1, 50, 130} (the first rows of
``Xs``) and M1 in {1, 5, 8, 9, 130} rows of a second draw (nine crosses the eight-location block).

Tolerance rule (mean, full covariance with and without noise, its diagonal against the unclipped variance, between-points
covariance): that of tests/test_gpu_sparse_gp.py, bound = max(MULT x float64-oracle error, 1e-13 x largest entry), both errors
against the long-double truth; a ratio counts only where the device's error is above the floor.  MULT is the smallest power of
two that leaves a factor 4 over the worst ratio observed on an MI355X, profiles/sparse_cov_errors.txt (written by
tools/sparse_cov_errors.py from this suite's own printed figures):
  "642 quantities, 44 above the floor; worst ratio above the floor 3.84 (S3 Exponential iso: between R=1 M1=1); x 4 = 15.35 -> MULT = 16."
  "S3 Exponential iso: between R=1 M1=1   scale 2.261e-05  device 1.542e-17  oracle 4.017e-18  ratio 3.84"
That is above the sparse suite's 8 because the rule's floor follows the largest entry of the RESULT, while every entry is a
difference of terms of the order of the prior variance 1.3 (ulp 2.9e-16): in a 1 x 1 block of size 2.3e-5 both errors are a few
hundredths of one rounding of the terms, and their quotient is luck.  No mean or full-covariance quantity comes above the floor at
all (the factored form); on the 130 x 130 between-points block the ratio is 1.24 (S2 rbf ard).

Bits: cov == cov.T; the same call twice; row 0 of the between-points covariance in the company of M1 = 1, 5, 9, 130 and for
R = 50 against the first 50 columns of R = 130.  Samples: Z = I gives the factor C (upper triangle exactly zero), the mean is the
full-covariance entry's bit for bit, max|C C^T - cov - jit I| <= 1e-12 max|cov| (the figure tests/test_gpu_round2_api.py holds
the exact model's factor to), jit == 0 on every run (tests/test_sparse_cov_host.py asserts a smallest eigenvalue >= 1e-7 of the
noiseless covariance per run), and with the noise in C and four fixed draws against numpy's Cholesky of the oracle's covariance at
the exact test's 1e-6 of the largest entry.  The singular case (S1 Matern-5/2, 20 duplicated rows, noise out): finite draws, jit
on jitchol's ladder of the covariance's mean diagonal, the factor at the exact test's 1e-10.  Refusals, the G cache across a
refit, the exact model's and the sparse model's other results bitwise untouched by interleaved calls, the model level and
entropy search (1e-9 of the largest |value|: the project's rule for posterior-derived scores at noise >= 1e-2).
Every figure is printed before it is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import entropy_search as E

import _sparse_ref as R
import _sparse_cov_ref as C
from test_gpu_sparse_gp import RUNS, IDS, KID

pytestmark = pytest.mark.gpu

MULT = 16.0
FLOOR = 1e-13
LDT = np.longdouble
SUB_M = (128, 5, 1)
BETWEEN_R = (1, 50, 130)
BETWEEN_M1 = (1, 5, 8, 9, 130)


@functools.lru_cache(maxsize=None)
def _ref(case, fam, ard):
    """Inputs, the float64 oracle and the long-double truth of a run: mean, covariance with and without noise, the unclipped
    variance, and the covariance between the second draw and ``Xs``.  Computed once and shared; read-only."""
    X, Y, Z, Xs = R.case_inputs(case)
    ls = R.case_lengthscale(X.shape[1], ard)
    X1 = C.second_draw(case)
    out = dict(X=X, Y=Y, Z=Z, Xs=Xs, X1=X1, ls=ls)
    for tag, lin in (("f64", R.F64), ("ld", R.LD)):
        f = R.inference(fam, X, Z, Y, R.VARIANCE, ls, ard, R.NOISE, lin, grads=False)
        mean, cov0, var = C.full_cov(f, Z, Xs, R.NOISE, False, lin)
        cov1 = cov0 + lin.dtype(R.NOISE) * np.eye(Xs.shape[0], dtype=lin.dtype)
        out[tag] = dict(mean=mean, cov0=cov0, cov1=cov1, var=var, between=C.cov_between(f, Z, X1, Xs, lin))
    return out


def _handle(case, fam, ard, mc_max=256):
    r = _ref(case, fam, ard)
    h = _lib.Handle(0)
    h.set_option("mc_max", mc_max)
    h.set_data(r["X"], r["Y"])
    h.set_params(KID[fam], ard, R.VARIANCE, r["ls"], R.NOISE)
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


def _tag(case, fam, ard):
    return "%s %s %s" % (case, fam, "ard" if ard else "iso")


# ---- accuracy and bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fam,ard", RUNS, ids=IDS)
def test_full_covariance_against_long_double(case, fam, ard):
    h, r = _handle(case, fam, ard)
    try:
        _, jk, jb = h.sparse_fit()
        assert (jk, jb) == (0.0, 0.0)
        tag = _tag(case, fam, ard)
        full = {}
        for inc in (True, False):
            m, cov = h.sparse_predict_full_cov(r["Xs"], include_noise=inc)
            full[inc] = (m, cov)
            assert np.array_equal(cov, cov.T), "not bitwise symmetric"
            _check("%s: 130 rows noise=%d mean" % (tag, inc), m, r["f64"]["mean"], r["ld"]["mean"])
            _check("%s: 130 rows noise=%d cov" % (tag, inc), cov, r["f64"]["cov%d" % inc], r["ld"]["cov%d" % inc])
            m2, cov2 = h.sparse_predict_full_cov(r["Xs"], include_noise=inc)
            assert np.array_equal(m2, m) and np.array_equal(cov2, cov)
        _check("%s: 130 rows diag against var" % tag, np.diag(full[False][1]), r["f64"]["var"], r["ld"]["var"])
        assert np.array_equal(full[True][0], full[False][0])
        for M in SUB_M:
            for inc in (True, False):
                m, cov = h.sparse_predict_full_cov(r["Xs"][:M], include_noise=inc)
                assert m.shape == (M, r["Y"].shape[1]) and cov.shape == (M, M) and np.array_equal(cov, cov.T)
                _check("%s: %d rows noise=%d mean" % (tag, M, inc), m, r["f64"]["mean"][:M], r["ld"]["mean"][:M])
                _check("%s: %d rows noise=%d cov" % (tag, M, inc), cov, r["f64"]["cov%d" % inc][:M, :M], r["ld"]["cov%d" % inc][:M, :M])
    finally:
        h.close()


@pytest.mark.parametrize("case,fam,ard", RUNS, ids=IDS)
def test_between_points_against_long_double(case, fam, ard):
    h, r = _handle(case, fam, ard)
    try:
        h.sparse_fit()
        tag = _tag(case, fam, ard)
        got = {}
        for Rn in BETWEEN_R:
            h.sparse_cov_set_points(r["Xs"][:Rn])
            for M1 in BETWEEN_M1:
                c = h.sparse_cov_between(r["X1"][:M1])
                assert c.shape == (M1, Rn)
                got[Rn, M1] = c
                _check("%s: between R=%d M1=%d" % (tag, Rn, M1), c, r["f64"]["between"][:M1, :Rn], r["ld"]["between"][:M1, :Rn])
                assert np.array_equal(h.sparse_cov_between(r["X1"][:M1]), c)          # the same call, the same bits
            for M1 in BETWEEN_M1:                                                       # a row's bits do not depend on its company
                n = min(M1, 8)
                assert np.array_equal(got[Rn, M1][:n], got[Rn, 130][:n]), (Rn, M1)
            # ... nor on its slot: row 8 alone and as the first row of the second block of eight
            assert np.array_equal(h.sparse_cov_between(r["X1"][8:9]), got[Rn, 130][8:9])
        for M1 in BETWEEN_M1:                                                           # ... nor on how R is cut
            assert np.array_equal(got[50, M1], got[130, M1][:, :50]), M1
            assert np.array_equal(got[1, M1], got[130, M1][:, :1]), M1
    finally:
        h.close()


# ---- samples ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fam,ard", RUNS, ids=IDS)
def test_samples_factor_and_draws(case, fam, ard):
    h, r = _handle(case, fam, ard)
    try:
        h.sparse_fit()
        tag = _tag(case, fam, ard)
        Xs = r["Xs"]
        M = Xs.shape[0]
        for inc in (True, False):
            mean0, cov = h.sparse_predict_full_cov(Xs, include_noise=inc)
            mean, dev, jit = h.sparse_posterior_samples(Xs, np.eye(M), include_noise=inc)
            Cf = dev.T
            assert np.array_equal(mean, mean0)
            assert np.all(np.triu(Cf, 1) == 0.0)
            fig = float(np.max(np.abs(Cf @ Cf.T - cov - jit * np.eye(M)))) / float(np.max(np.abs(cov)))
            print("%-44s jitter %g  |C C^T - cov - jit I| / max|cov| %.3e" % ("%s: samples noise=%d" % (tag, inc), jit, fig))
            assert jit == 0.0
            assert fig <= 1e-12
        C0 = np.linalg.cholesky(np.asarray(r["f64"]["cov1"], dtype=float))
        mean, dev, jit = h.sparse_posterior_samples(Xs, np.eye(M), include_noise=True)
        fig = float(np.max(np.abs(dev.T - C0))) / float(np.max(np.abs(C0)))
        print("%-44s factor against numpy's %.3e" % ("%s: samples noise=1" % tag, fig))
        assert fig <= 1e-6
        Zn = np.random.RandomState(3).standard_normal((4, M))
        mean, dev, jit = h.sparse_posterior_samples(Xs, Zn, include_noise=True)
        want = Zn @ C0.T
        fig = float(np.max(np.abs(dev - want))) / float(np.max(np.abs(want)))
        print("%-44s four draws against Z C0^T %.3e" % ("%s: samples noise=1" % tag, fig))
        assert dev.shape == (4, M) and jit == 0.0 and fig <= 1e-6
    finally:
        h.close()


def test_samples_of_a_singular_covariance():
    """S1 Matern-5/2 with rows 20..39 copies of rows 0..19, noise out: the covariance is singular to rounding."""
    h, r = _handle("S1", "Mat52", True)
    try:
        h.sparse_fit()
        Xs = r["Xs"][:40].copy()
        Xs[20:40] = Xs[:20]
        _, cov = h.sparse_predict_full_cov(Xs, include_noise=False)
        maxtries = 5
        mean, dev, jit = h.sparse_posterior_samples(Xs, np.eye(40), include_noise=False, maxtries=maxtries)
        assert np.all(np.isfinite(dev))
        ladder = [0.0] + [float(np.mean(np.diag(cov))) * 1e-6 * 10.0 ** k for k in range(maxtries)]
        fig = float(np.max(np.abs(dev.T @ dev - cov - jit * np.eye(40)))) / float(np.max(np.abs(cov)))
        print("singular case: jitter %g (ladder %s)  |C C^T - cov - jit I| / max|cov| %.3e" % (jit, ladder, fig))
        assert any(jit == v or abs(jit - v) <= 1e-12 * v for v in ladder)
        assert fig <= 1e-10
    finally:
        h.close()


# ---- state, refusals, isolation -----------------------------------------------------------------------------------------------------
def test_return_codes_leave_the_context_as_it_was():
    lib = _lib.load()
    h, r = _handle("S1", "rbf", True)
    try:
        g = h.h
        buf = np.zeros(130 * 130)
        p = _lib.dptr(buf)
        pv = buf.ctypes.data
        Xs = np.ascontiguousarray(r["Xs"])
        x = _lib.dptr(Xs)
        xv = Xs.ctypes.data
        d = ctypes.c_double()
        # no sparse fit
        assert lib.gp_sparse_predict_full_cov(g, x, 5, 1, p, p) == _lib.GP_ERR_STATE
        assert lib.gp_sparse_posterior_samples(g, x, 5, 1, p, 1, 5, p, p, ctypes.byref(d)) == _lib.GP_ERR_STATE
        assert lib.gp_sparse_cov_between(g, xv, 5, pv) == _lib.GP_ERR_STATE
        h.sparse_fit()
        assert lib.gp_sparse_cov_between(g, xv, 5, pv) == _lib.GP_ERR_STATE               # no points yet
        assert b"gp_sparse_cov_set_points" in lib.gp_last_error()
        h.sparse_cov_set_points(Xs[:50])
        want = (h.sparse_predict_full_cov(Xs, include_noise=True), h.sparse_cov_between(r["X1"][:9]),
                h.sparse_posterior_samples(Xs[:40], np.eye(40), include_noise=True), h.sparse_predict(Xs))
        # null pointers
        assert lib.gp_sparse_predict_full_cov(None, x, 5, 1, p, p) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_predict_full_cov(g, None, 5, 1, p, p) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_predict_full_cov(g, x, 5, 1, p, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_posterior_samples(g, None, 5, 1, p, 1, 5, p, p, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_posterior_samples(g, x, 5, 1, None, 1, 5, p, p, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_posterior_samples(g, x, 5, 1, p, 1, 5, p, None, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_cov_set_points(None, x, 5) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_cov_set_points(g, None, 5) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_cov_between(None, xv, 5, pv) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_cov_between(g, None, 5, pv) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_cov_between(g, xv, 5, None) == _lib.GP_ERR_ARG
        # counts below 1, and past mc_max (256)
        assert lib.gp_sparse_predict_full_cov(g, x, 0, 1, p, p) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_posterior_samples(g, x, 0, 1, p, 1, 5, p, p, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_posterior_samples(g, x, 5, 1, p, 0, 5, p, p, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_cov_set_points(g, x, 0) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_cov_between(g, xv, 0, pv) == _lib.GP_ERR_ARG
        big = np.zeros((257, 3))
        bp = _lib.dptr(big)
        assert lib.gp_sparse_predict_full_cov(g, bp, 257, 1, None, p) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_posterior_samples(g, bp, 257, 1, p, 1, 5, None, p, None) == _lib.GP_ERR_ARG
        assert lib.gp_sparse_cov_set_points(g, bp, 257) == _lib.GP_ERR_ARG
        # a resident mean function
        h.mean_set(np.ones((3, 1)), np.zeros(1))
        assert lib.gp_sparse_predict_full_cov(g, x, 5, 1, p, p) == _lib.GP_ERR_STATE
        assert lib.gp_sparse_posterior_samples(g, x, 5, 1, p, 1, 5, p, p, None) == _lib.GP_ERR_STATE
        assert lib.gp_sparse_cov_set_points(g, x, 5) == _lib.GP_ERR_STATE
        assert lib.gp_sparse_cov_between(g, xv, 5, pv) == _lib.GP_ERR_STATE
        h.mean_set(None, None)
        # everything as it was: the fit, the points (50 of them), G
        h.sparse_fit()
        got = (h.sparse_predict_full_cov(Xs, include_noise=True), h.sparse_cov_between(r["X1"][:9]),
               h.sparse_posterior_samples(Xs[:40], np.eye(40), include_noise=True), h.sparse_predict(Xs))
        for a, b in zip(want, got):
            assert all(np.array_equal(u, v) for u, v in zip(a, b)) if isinstance(a, tuple) else np.array_equal(a, b)
    finally:
        h.close()


def test_a_refit_rebuilds_g_and_keeps_the_points():
    h, r = _handle("S2", "Mat32", True)
    try:
        h.sparse_fit()
        h.sparse_cov_set_points(r["Xs"][:50])
        before = h.sparse_cov_between(r["X1"][:9])
        ls2 = 1.3 * r["ls"]
        h.set_params(KID["Mat32"], True, 0.9, ls2, R.NOISE)
        h.sparse_fit()
        after = h.sparse_cov_between(r["X1"][:9])             # no new gp_sparse_cov_set_points
        assert not np.array_equal(before, after)
        f = R.inference("Mat32", r["X"], r["Z"], r["Y"], 0.9, ls2, True, R.NOISE, R.F64, grads=False)
        want = C.cov_between(f, r["Z"], r["X1"][:9], r["Xs"][:50], R.F64)
        fig = float(np.max(np.abs(after - want))) / float(np.max(np.abs(want)))
        print("between-points after a refit against the float64 oracle of the new fit: %.3e" % fig)
        assert fig <= 1e-9      # (the new fit, not the old one: the two differ by O(1))
        fresh, _ = _handle("S2", "Mat32", True)
        try:
            fresh.set_params(KID["Mat32"], True, 0.9, ls2, R.NOISE)
            fresh.sparse_fit()
            fresh.sparse_cov_set_points(r["Xs"][:50])
            assert np.array_equal(fresh.sparse_cov_between(r["X1"][:9]), after)
        finally:
            fresh.close()
    finally:
        h.close()


def _joint_calls(h, r):
    """The four new calls, as interleaved between others."""
    h.sparse_predict_full_cov(r["Xs"], include_noise=True)
    h.sparse_posterior_samples(r["Xs"][:40], np.eye(40), include_noise=False)
    h.sparse_cov_set_points(r["Xs"][:50])
    h.sparse_cov_between(r["X1"][:3])
    h.sparse_cov_between(r["X1"][:20])


@pytest.mark.parametrize("case", ["S2", "S1"])
def test_exact_model_bits_survive_interleaved_joint_calls(case):
    """The pattern of test_exact_model_bits_survive_interleaved_sparse_calls over the four new entries; gp_predict_full_cov too."""
    r = _ref(case, "Mat52", True)
    one = r["Y"].shape[1] == 1

    def exact(h):
        fit = h.fit()
        h.set_candidates(r["Xs"])
        return fit, h.predict(include_noise=True), h.alpha(), h.fmin() if one else None

    def setup():
        h = _lib.Handle(0)
        h.set_option("mc_max", 256)
        h.set_data(r["X"], r["Y"])
        h.set_params(KID["Mat52"], True, R.VARIANCE, r["ls"], R.NOISE)
        return h

    fresh = setup()
    want = exact(fresh)
    want_full = fresh.predict_full_cov(include_noise=True)
    want_pred = fresh.predict(include_noise=True)
    fresh.close()
    h = setup()
    try:
        first = exact(h)
        h.sparse_set_inducing(r["Z"])
        h.sparse_fit()
        _joint_calls(h, r)
        m1, v1 = h.predict(include_noise=True)                  # the resident candidates' posterior between the new calls
        _joint_calls(h, r)
        full1 = h.predict_full_cov(include_noise=True)
        _joint_calls(h, r)
        m2, v2 = h.predict(include_noise=True)
        second = exact(h)
        for got in (first, second):
            assert got[0] == want[0] and got[3] == want[3]
            assert np.array_equal(got[1][0], want[1][0]) and np.array_equal(got[1][1], want[1][1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(m1, want[1][0]) and np.array_equal(v1, want[1][1])
        assert np.array_equal(full1[0], want_full[0]) and np.array_equal(full1[1], want_full[1])
        assert np.array_equal(m2, want_pred[0]) and np.array_equal(v2, want_pred[1])
    finally:
        h.close()


def test_sparse_model_bits_survive_interleaved_joint_calls():
    """gp_sparse_predict and gp_sparse_acq (a cached table posterior) are bitwise what they are without the new calls."""
    def sparse(h, r, between):
        h.sparse_fit()
        h.sparse_set_candidates(r["Xs"])
        out = [h.sparse_predict(r["Xs"], include_noise=True, grad=True)]
        between()
        out.append((h.sparse_acq(_lib.GP_ACQ_EI, 0.01, 0.1),))          # fills the table cache
        between()
        out.append((h.sparse_acq(_lib.GP_ACQ_LCB, 2.0, 0.1),))          # ... and is served from it
        between()
        out.append(h.sparse_predict(r["Xs"][:7], include_noise=False))
        return out

    plain, r = _handle("S1", "Mat52", True)
    mixed, _ = _handle("S1", "Mat52", True)
    try:
        want = sparse(plain, r, lambda: None)
        got = sparse(mixed, r, lambda: _joint_calls(mixed, r))
        for a, b in zip(want, got):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finally:
        plain.close()
        mixed.close()


# ---- model level ------------------------------------------------------------------------------------------------------------------
def _model(P=2, normalizer=True, Mz=12, N=60, D=2, seed=21):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = 3.0 + 2.0 * np.sin(3 * X.sum(1))[:, None] * np.linspace(1.0, 0.5, P)[None, :] + 0.1 * rng.standard_normal((N, P))
    m = gpo.models.SparseGPRegression(X, Y, kernel=gpo.kern.Matern52(D, variance=1.2, lengthscale=0.4), Z=X[:Mz].copy(),
                                      normalizer=normalizer)
    m.likelihood.variance.set(2e-2)
    return m, X, Y


def test_model_full_cov_samples_and_between_points():
    m, X, Y = _model()
    try:
        rng = np.random.RandomState(4)
        Xn = rng.uniform(0, 1, (9, 2))
        mean, cov = m.predict(Xn, full_cov=True)
        mu1, var1 = m.predict(Xn)
        raw_mean, raw_cov = m._raw_predict(Xn, full_cov=True)
        std = np.asarray(m.normalizer.std, dtype=float).reshape(-1)
        assert mean.shape == (9, 2) and cov.shape == (9, 9, 2) and raw_cov.shape == (9, 9)
        noise = float(m.likelihood.variance)
        fig = float(np.max(np.abs(cov - (raw_cov + noise * np.eye(9))[:, :, None] * std[None, None, :] ** 2)))
        print("model: full_cov with the normaliser undone against the raw covariance x std^2: %.3e" % fig)
        assert fig <= 1e-13 * float(np.max(np.abs(cov)))
        assert np.max(np.abs(mean - mu1)) <= 1e-12 * np.max(np.abs(mu1))
        # (var1 of P = 2 is [9, 2] by inverse_variance; its column d is the diagonal of cov[:, :, d])
        assert np.max(np.abs(np.diagonal(cov, axis1=0, axis2=1).T - var1)) <= 1e-10 * np.max(np.abs(var1))
        nl_mean, nl_cov = m.predict_noiseless(Xn, full_cov=True)
        assert np.max(np.abs(nl_cov - raw_cov[:, :, None] * std[None, None, :] ** 2)) <= 1e-13 * np.max(np.abs(nl_cov))
        # samples: shape, reproducible with given normals, the normaliser's std on the deviations
        normals = np.random.RandomState(8).standard_normal((2, 6, 9))
        f1 = m.posterior_samples_f(Xn, size=6, normals=normals)
        f2 = m.posterior_samples_f(Xn, size=6, normals=normals)
        assert f1.shape == (9, 2, 6) and np.array_equal(f1, f2) and m.posterior_samples_jitter_ == 0.0
        Cf = np.linalg.cholesky(raw_cov)
        want = nl_mean[:, :, None] + np.einsum("ij,dsj->ids", Cf, normals) * std[None, :, None]
        fig = float(np.max(np.abs(f1 - want))) / float(np.max(np.abs(want)))
        print("model: posterior_samples_f against numpy's factor of the device's covariance: %.3e" % fig)
        assert fig <= 1e-6
        assert m.posterior_samples_f(Xn, size=3).shape == (9, 2, 3)
        # between points: the block of the stacked full covariance; X1 resident across calls
        X1, X2 = Xn[:5], rng.uniform(0, 1, (4, 2))
        calls = []
        real = m._h.sparse_cov_set_points
        m._h.sparse_cov_set_points = lambda pts: (calls.append(pts.shape), real(pts))[1]
        blk = m.posterior_covariance_between_points(X1, X2)
        again = m.posterior_covariance_between_points(X1, X2[:2])
        _, stacked = m._raw_predict(np.vstack([X1, X2]), full_cov=True)
        f = R.inference("Mat52", X, m.Z_values, (Y - m.normalizer.mean) / m.normalizer.std, 1.2, np.array([0.4]), False, noise, R.F64,
                        grads=False)
        fl = R.inference("Mat52", X, m.Z_values, (Y - m.normalizer.mean) / m.normalizer.std, 1.2, np.array([0.4]), False, noise, R.LD,
                         grads=False)
        truth = C.cov_between(fl, m.Z_values, X1, X2, R.LD)
        _check("model: between points", blk, C.cov_between(f, m.Z_values, X1, X2, R.F64), truth)
        _check("model: block of the stacked covariance", stacked[:5, 5:], C.cov_between(f, m.Z_values, X1, X2, R.F64), truth)
        assert blk.shape == (5, 4) and np.array_equal(again, blk[:, :2])
        assert calls == [(5, 2)], calls                       # X1 was uploaded once
        m.kern.lengthscale.set(0.5)                           # a refit keeps the points on the device
        m.posterior_covariance_between_points(X1, X2)
        assert calls == [(5, 2)], calls
        m.posterior_covariance_between_points(X2, X1)
        assert calls == [(5, 2), (4, 2)], calls
    finally:
        m.close()


class _FixedSampler(E.McmcSampler):
    def __init__(self, space, points):
        super().__init__(space)
        self.points = points

    def get_samples(self, n_samples, log_p_function, burn_in_steps=50):
        pts = self.points[:n_samples]
        return pts, -0.5 * np.sum((pts - 0.5) ** 2, axis=1).reshape(-1, 1)      # fixed log values


def test_entropy_search_over_a_sparse_model_matches_the_oracle():
    rng = np.random.RandomState(31)
    N, D, Mz = 60, 2, 10
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    np.random.seed(9)
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(D, variance=R.VARIANCE, lengthscale=0.4), sparse=True, num_inducing=Mz, max_iters=0,
                     verbose=False)
    gm.updateModel(X, Y, None, None)
    gm.model.likelihood.variance.set(R.NOISE)
    try:
        space = gpo.Design_space([{"name": "x", "type": "continuous", "domain": (0.0, 1.0), "dimensionality": D}])
        pts = rng.uniform(0, 1, (12, D))
        es = gpo.AcquisitionEntropySearch(gm, space, _FixedSampler(space, pts), num_samples=20, num_representer_points=12)
        Xc = rng.uniform(0, 1, (7, D))
        got = es.acquisition_function(Xc)
        # the same arithmetic fed from the float64 oracle's sparse posterior (Y normalised as the model holds it); the class
        # returns the negated score (base.py:33-39)
        gp = gm.model
        Yn = Y if gp.normalizer is None else (Y - gp.normalizer.mean) / gp.normalizer.std
        f = R.inference("Mat52", X, gp.Z_values, Yn, R.VARIANCE, np.array([0.4]), False, R.NOISE, R.F64, grads=False)

        def undo_mean(a):
            return a if gp.normalizer is None else gp.normalizer.inverse_mean(a)

        def undo_var(a):
            return a if gp.normalizer is None else gp.normalizer.inverse_variance(a)
        mu_r, cov_r, _ = C.full_cov(f, gp.Z_values, pts, R.NOISE, True, R.F64)
        mu_r, cov_r = np.ravel(undo_mean(mu_r)), np.maximum(undo_var(cov_r), 1e-10)
        logP, dMu, dSigma, dMuMu = E.joint_min(mu_r, cov_r, None)
        Q = E.quadratic_forms(dSigma, dMuMu)
        logs = -0.5 * np.sum((pts - 0.5) ** 2, axis=1).reshape(-1, 1)
        _, _, var_c = C.full_cov(f, gp.Z_values, Xc, R.NOISE, False, R.F64)
        sd = np.sqrt(np.maximum(undo_var(np.clip(var_c, 1e-15, np.inf)[:, None]), 1e-10))
        cb = C.cov_between(f, gp.Z_values, pts, Xc, R.F64)
        want = -np.array([[E.score(cb[:, [j]] / sd[j], logP.reshape(-1, 1), logs, dMu, Q, es.W)] for j in range(7)])
        fig = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
        print("entropy search over a sparse model against the oracle's posterior: %.3e (largest |value| %.3g)" % (fig, np.max(np.abs(want))))
        assert got.shape == (7, 1) and fig <= 1e-9
    finally:
        gm.model.close()


def test_bayesian_optimization_with_entropy_search_over_a_sparse_model():
    rng = np.random.RandomState(21)
    X0 = rng.uniform(0, 1, (30, 2))
    Y0 = np.sin(3 * X0.sum(1))[:, None] + 0.1 * rng.standard_normal((30, 1))
    domain = [{'name': 'x%d' % i, 'type': 'continuous', 'domain': (0.0, 1.0)} for i in range(2)]
    np.random.seed(5)
    model = gpo.GPModel(sparse=True, num_inducing=10, exact_feval=True, max_iters=20, optimize_restarts=1, verbose=False)
    bo = gpo.BayesianOptimization(lambda x: np.sin(3 * np.atleast_2d(x).sum(1))[:, None], domain, X=X0, Y=Y0, model=model,
                                  acquisition_type='ES', num_representer_points=12, num_samples=20, burn_in_steps=5, sampler_seed=1)
    assert isinstance(bo.acquisition, gpo.AcquisitionEntropySearch)
    x1 = bo.suggest_next_locations()
    print("first suggestion", x1)
    assert x1.shape == (1, 2) and np.all((x1 >= 0.0) & (x1 <= 1.0))
    bo.X = np.vstack([bo.X, x1])
    bo.Y = np.vstack([bo.Y, np.sin(3 * x1.sum(1))[:, None]])
    x2 = bo.suggest_next_locations()
    print("second suggestion", x2)
    assert x2.shape == (1, 2) and np.all((x2 >= 0.0) & (x2 <= 1.0))
    assert isinstance(model.model, gpo.models.SparseGPRegression)
    model.model.close()
