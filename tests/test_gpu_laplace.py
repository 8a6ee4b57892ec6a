"""GPU: GP classification -- the Laplace probit fit on the device (gp_laplace_fit, gp_laplace_fit_grad), the latent posterior
through the existing prediction entries on the Laplace-fitted handle, repeatability, state hygiene, and binary constraints in
``FeasibilityModel`` / ``BayesianOptimization`` -- against the long-double truth of tests/_laplace_truth.py.

Tolerances are the north-star figures of tests/test_gpu_parity.py: log Z and log|B| 1e-8 relative, alpha and f 1e-6 of their
largest element, gradient entries 1e-6 of max(|entry|, 1); the posterior entries as tests/test_gpu_rows.py and
tests/test_gpu_feas.py hold them (mean 1e-6 max(1, |m|), sd 1e-6 sd + 1e-12, dmdx 1e-6 max(|dmdx|_max, 1e-3), dvdx 1e-6 variance);
the class probability what those propagate to through Phi (_laplace_truth.posterior: tol_p).  Every test prints its figures
before it asserts (tools/laplace_errors.py collects them)."""
import ctypes
import functools

import numpy as np
import pytest
from scipy.special import ndtr

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd._lib import dptr

import _feas_truth as FT
import _laplace_truth as LT

pytestmark = pytest.mark.gpu

KID = {"RBF": _lib.GP_KERNEL_RBF, "Mat52": _lib.GP_KERNEL_MATERN52, "Mat32": _lib.GP_KERNEL_MATERN32,
       "Exponential": _lib.GP_KERNEL_EXPONENTIAL}
KERN = {"RBF": "RBF", "Mat52": "Matern52", "Mat32": "Matern32", "Exponential": "Exponential"}
CASE_IDS = [c.id for c in LT.TABLE]
FEAS = _lib.GP_ACQ_TIMES_FEAS


def _f(a):
    return np.asarray(a, dtype=np.float64)


def _handle(cid, noise=0.37):
    """A handle with the case's data and kernel (the noise is ignored by the Laplace fit), not fitted."""
    p = LT.problem(cid)
    c = LT.CASES[cid]
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    if c.lookahead:
        h.set_option("lookahead_min_tiles", 0)      # the look-ahead factorisation inside the Newton loop (tests/test_gpu_lookahead.py)
    h.set_data(p.X, p.labels01)
    h.set_params(KID[c.fam], int(c.ard), c.variance, p.ls_arg, noise)
    return h


Fitted = LT.collections.namedtuple("Fitted", "h logz logdet iters halvings grad alpha f W")


@functools.lru_cache(maxsize=None)
def fitted(cid):
    """The case's handle after gp_laplace_fit_grad, with what it returned: made once, shared, left Laplace-fitted."""
    p = LT.problem(cid)
    h = _handle(cid)
    (lz, ld, it, hv), (dv, dl) = h.laplace_fit_grad(p.y, p.ls_arg.size)
    f, W = h.laplace_mode()
    return Fitted(h, lz, ld, it, hv, np.r_[dv, dl], h.alpha().ravel(), f, W)


# ---- 1. the fit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_fit_against_the_truth(cid):
    ft, r = LT.fit(cid), fitted(cid)
    e_z = abs(r.logz - float(ft.logZ)) / abs(float(ft.logZ))
    e_d = abs(r.logdet - float(ft.logdetB)) / abs(float(ft.logdetB))
    e_a = float(np.abs(r.alpha - ft.a).max() / np.abs(ft.a).max())
    e_f = float(np.abs(r.f - ft.f).max() / np.abs(ft.f).max())
    it, hv, wmin, wmax = r.h.laplace_info()
    print("LAPLACE fit case %s: log Z %.3g, log|B| %.3g relative; alpha %.3g, f %.3g of the largest; %d steps, %d halvings, "
          "W in [%.3g, %.3g]" % (cid, e_z, e_d, e_a, e_f, it, hv, wmin, wmax))
    assert e_z <= 1e-8 and e_d <= 1e-8
    assert e_a <= 1e-6 and e_f <= 1e-6
    assert (it, hv) == (r.iters, r.halvings) and 1 <= it <= LT.CAP
    assert abs(wmin - float(ft.W.min())) <= 1e-6 * float(ft.W.min()) and abs(wmax - float(ft.W.max())) <= 1e-6
    # gp_laplace_fit alone: the same fit, the same bits -- and the converged flag, through the C entry itself
    h2 = _handle(cid)
    lz, ld, it2, hv2 = h2.laplace_fit(LT.problem(cid).y)
    assert (lz, ld, it2, hv2) == (r.logz, r.logdet, r.iters, r.halvings)
    y = np.ascontiguousarray(LT.problem(cid).y)
    z, d = ctypes.c_double(), ctypes.c_double()
    n_it, n_hv, flag = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = h2.lib.gp_laplace_fit(h2.h, dptr(y), LT.CAP, ctypes.byref(z), ctypes.byref(d), ctypes.byref(n_it), ctypes.byref(n_hv),
                               ctypes.byref(flag))
    assert rc == 0 and flag.value == 1 and n_it.value == r.iters <= LT.CAP and z.value == r.logz
    rc = h2.lib.gp_laplace_fit(h2.h, dptr(y), 1, None, None, ctypes.byref(n_it), None, ctypes.byref(flag))
    assert rc == _lib.GP_LAPLACE_NOT_CONVERGED and flag.value == 0 and n_it.value == 1      # one step never suffices
    h2.close()


def test_a_fit_that_reaches_the_cap_raises_and_leaves_no_fit():
    p = LT.problem("f")
    h = _handle("f")
    with pytest.raises(RuntimeError, match="did not converge"):
        h.laplace_fit(p.y, cap=2)
    rc = h.lib.gp_laplace_fit(h.h, dptr(p.y.copy()), 2, None, None, None, None, None)
    assert rc == _lib.GP_LAPLACE_NOT_CONVERGED > 0
    with pytest.raises(RuntimeError, match="gp_fit first"):
        h.alpha()
    with pytest.raises(ValueError, match="label"):
        h.laplace_fit(np.where(p.y > 0, 1.0, 0.0))
    h.close()


# ---- 2. the gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gradient_against_the_truth(cid):
    g, r = LT.gradient(cid), fitted(cid)
    err = np.abs(r.grad - g) / np.maximum(np.abs(g), 1)
    print("LAPLACE gradient case %s (%s, %s): worst entry %.3g of max(|entry|, 1)" % (
        cid, LT.CASES[cid].fam, "ARD" if LT.CASES[cid].ard else "iso", float(err.max())))
    assert r.grad.size == 1 + LT.problem(cid).ls_arg.size
    assert np.all(err <= 1e-6)


# ---- 3. the latent posterior through the existing entries ----------------------------------------------------------------------------
def _check_post(tag, po, sl, mean, var, noise, dm=None, dv=None):
    m0, v0 = po.mean[sl], po.var[sl] + (1 if noise else 0)
    e_m = float((np.abs(mean.ravel() - m0) / np.maximum(1, np.abs(m0))).max())
    sd, sd0 = np.sqrt(var.ravel()), np.sqrt(v0)
    e_s = float((np.abs(sd - sd0) / (1e-6 * sd0 + 1e-12)).max())
    msg = "LAPLACE posterior %s: mean %.3g of max(1, |m|), sd %.3g of its tolerance" % (tag, e_m, e_s)
    ok = e_m <= 1e-6 and e_s <= 1.0
    if dm is not None:
        e_dm = float(np.abs(dm.reshape(po.dmdx[sl].shape) - po.dmdx[sl]).max() / max(float(np.abs(po.dmdx[sl]).max()), 1e-3))
        e_dv = float((np.abs(dv - po.dvdx[sl]).max(1) / po.var[sl]).max())
        msg += ", dmdx %.3g of max(|dmdx|, 1e-3), dvdx %.3g of the variance" % (e_dm, e_dv)
        ok = ok and e_dm <= 1e-6 and e_dv <= 1e-6
    print(msg)
    assert ok, msg


@pytest.mark.parametrize("cid", CASE_IDS)
def test_posterior_through_the_existing_entries(cid):
    p, po, h = LT.problem(cid), LT.posterior(cid), fitted(cid).h
    M = p.Xs.shape[0]
    # the table route: gp_predict without and with the noise, gp_predict_grad
    h.set_candidates(p.Xs)
    m, v = h.predict(include_noise=False)
    _check_post("case %s table" % cid, po, slice(0, M), m, v, False)
    m1, v1 = h.predict(include_noise=True)
    dm, dv = h.predict_grad()
    _check_post("case %s table + noise + gradients" % cid, po, slice(0, M), m1, v1, True, dm, dv)
    # p(y = 1 | x) = Phi(m / sqrt(1 + s^2)) within what the posterior tolerances propagate to
    prob = ndtr(m1.ravel() / np.sqrt(v1.ravel()))
    e_p = float((np.abs(prob - po.p) / po.tol_p).max())
    print("LAPLACE class probability case %s: %.3g of the propagated tolerance (largest %.3g)" % (cid, e_p, float(po.tol_p.max())))
    assert e_p <= 1.0
    # the rows entries: one location, a narrow pass (4), a wide pass (8), two groups (9); with and without gradients
    for lo, hi in ((0, 1), (1, 5), (0, 8), (0, 9)):
        mr, vr, dmr, dvr = h.predict_rows(p.Xs[lo:hi], include_noise=True, grad=True)
        _check_post("case %s rows [%d, %d) + gradients" % (cid, lo, hi), po, slice(lo, hi), mr, vr, True, dmr, dvr)
        mr, vr = h.predict_rows(p.Xs[lo:hi], include_noise=False)
        _check_post("case %s rows [%d, %d) latent" % (cid, lo, hi), po, slice(lo, hi), mr, vr, False)


def test_the_model_class_predicts_probabilities():
    cid = "b"
    p, po, c = LT.problem(cid), LT.posterior(cid), LT.CASES[cid]
    k = getattr(gpo.kern, KERN[c.fam])(c.D, c.variance, p.ls_arg, ARD=c.ard)
    m = gpo.models.GPClassification(p.X, p.labels01, kernel=k)
    assert abs(m.log_likelihood() - float(LT.fit(cid).logZ)) <= 1e-8 * abs(float(LT.fit(cid).logZ))
    prob, var = m.predict(p.Xs)
    assert prob.shape == (p.Xs.shape[0], 1) and np.isnan(var)
    assert np.all(np.abs(prob.ravel() - po.p) <= po.tol_p)
    ml, vl = m.predict_noiseless(p.Xs)
    assert np.all(np.abs(ml.ravel() - po.mean) <= 1e-6 * np.maximum(1, np.abs(po.mean)))
    assert np.all(np.abs(np.sqrt(vl.ravel()) - np.sqrt(po.var)) <= 1e-6 * np.sqrt(po.var) + 1e-12)
    dm, dv = m.predictive_gradients(p.Xs)
    assert np.abs(dm[:, :, 0] - po.dmdx).max() <= 1e-6 * max(float(np.abs(po.dmdx).max()), 1e-3)
    # the objective's gradient in the optimiser's space against the truth's through the Logexp chain rule
    g = m.objective_function_gradients()
    th = np.r_[c.variance, p.ls_arg]
    want = -_f(LT.gradient(cid)) * (1 - np.exp(-th))          # d theta / d x of theta = log(1 + e^x)
    assert np.all(np.abs(g - want) <= 1e-6 * np.maximum(np.abs(want), 1))
    f0 = m.objective_function()
    m.optimize(max_iters=5)
    assert m.objective_function() <= f0 + 1e-9 and m.newton_iters_ >= 1
    m.close()


# ---- 4. repeatability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["c", "fl"])
def test_two_fits_give_the_same_bits(cid):
    p, r = LT.problem(cid), fitted(cid)
    h = _handle(cid)
    (lz, ld, it, hv), (dv, dl) = h.laplace_fit_grad(p.y, p.ls_arg.size)
    assert (lz, ld, it, hv) == (r.logz, r.logdet, r.iters, r.halvings)
    assert np.array_equal(np.r_[dv, dl], r.grad)
    assert np.array_equal(h.alpha().ravel(), r.alpha) and np.array_equal(h.chol(), r.h.chol())
    # ... and once more on the same handle
    lz2 = h.laplace_fit(p.y)[0]
    assert lz2 == lz and np.array_equal(h.chol(), r.h.chol())
    h.close()


def test_a_location_has_the_same_bits_whatever_its_slot_and_company():
    p = LT.problem("e")
    h = _handle("e")
    h.set_option("rows_build", 1)          # the fused rows path from the first call on
    h.laplace_fit(p.y)
    x = p.Xs[3:4]
    alone = h.predict_rows(x, include_noise=True, grad=True)
    for lo, hi in ((2, 6), (0, 4), (0, 8), (3, 9)):
        got = h.predict_rows(p.Xs[lo:hi], include_noise=True, grad=True)
        for a, b in zip(alone, got):
            assert np.array_equal(a[0], b[3 - lo]), (lo, hi)
    assert h.rows_stats()["fused"] >= 5
    h.close()


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------
def _regression_bits(h):
    lml, logdet, jit = h.fit()
    return lml, logdet, jit, h.alpha(), h.chol(), h.predict(include_noise=True)


def test_regression_after_laplace_and_the_reverse_match_a_fresh_handle_bitwise():
    p = LT.problem("d")
    fresh = _handle("d")
    fresh.set_candidates(p.Xs)
    want = _regression_bits(fresh)
    h = _handle("d")
    h.set_candidates(p.Xs)
    lz = h.laplace_fit(p.y)
    lap_pred = h.predict(include_noise=True)
    got = _regression_bits(h)                  # no set_params in between: the noise it gave is back in force
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a[0] if isinstance(a, tuple) else a), np.asarray(b[0] if isinstance(b, tuple) else b))
    assert np.array_equal(want[5][1], got[5][1])
    with pytest.raises(RuntimeError, match="not Laplace-fitted"):
        h.laplace_info()
    # the reverse: a Laplace fit on a handle that held a regression fit
    assert h.laplace_fit(p.y) == lz
    again = h.predict(include_noise=True)
    assert np.array_equal(again[0], lap_pred[0]) and np.array_equal(again[1], lap_pred[1])
    assert np.array_equal(h.chol(), fitted("d").h.chol())
    # gp_set_params clears the state as well
    c = LT.CASES["d"]
    h.set_params(KID[c.fam], int(c.ard), c.variance, p.ls_arg, 0.37)
    with pytest.raises(RuntimeError, match="gp_fit first"):
        h.predict(include_noise=True)
    got = _regression_bits(h)
    assert got[0] == want[0] and np.array_equal(got[4], want[4])
    fresh.close()
    h.close()


def test_refused_entries_return_their_error_code_on_a_laplace_fitted_handle():
    cid = "a"
    p, h = LT.problem(cid), fitted(cid).h
    lib, N, D = h.lib, p.X.shape[0], p.X.shape[1]
    h.set_candidates(p.Xs)
    before = h.predict(include_noise=True)
    d, out, big = ctypes.c_double(), np.zeros(N * D), np.zeros((N + 1) * (N + 1))
    one = np.ones(1)
    codes = {
        "gp_fmin": lib.gp_fmin(h.h, ctypes.byref(d)),
        "gp_lml_grad": lib.gp_lml_grad(h.h, ctypes.byref(d), dptr(out), ctypes.byref(d)),
        "gp_lml_grad_x": lib.gp_lml_grad_x(h.h, dptr(out)),
        "gp_get_dl_dk": lib.gp_get_dl_dk(h.h, dptr(big)),
        "gp_append": lib.gp_append(h.h, dptr(p.Xs[:1].copy()), 1, dptr(big), None, None),
        "gp_mean_set": lib.gp_mean_set(h.h, None, dptr(one)),
        "gp_mean_grad": lib.gp_mean_grad(h.h, dptr(out), dptr(out)),
        "gp_mes_set": lib.gp_mes_set(h.h, dptr(one), 1),
        "gp_kg_set_points": lib.gp_kg_set_points(h.h, dptr(p.Xs[:2].copy()), 2, 0.0, 1.0, out.ctypes.data),
        "gp_es_set_representers": lib.gp_es_set_representers(h.h, dptr(p.Xs[:2].copy()), 2, 0.0, 1.0, dptr(out), dptr(big)),
    }
    print("LAPLACE refusals:", codes)
    assert all(rc == _lib.GP_ERR_STATE for rc in codes.values()), codes
    assert b"Laplace-fitted" in lib.gp_last_error()
    for call in (lambda: h.paths_set(np.zeros((16, D)), np.zeros(16), np.zeros((1, 16)), np.zeros((1, N))),
                 lambda: h.qei_rows(p.Xs[:2]),
                 lambda: h.cost_set(p.X, np.zeros(N), 0, 0, 1.0, [0.3]),
                 lambda: h.fit_grad_batch([1.0], [list(p.ls_arg)], [0.1]),
                 lambda: h.fit_grad_x_batch(p.X[None], [1.0], [list(p.ls_arg)], [0.1]),
                 lambda: h.fit_grad_warp_batch(np.zeros((1, 1, 3)), [1.0], [1.0], [list(p.ls_arg)], [0.1]),
                 lambda: h.fmin_rows([0, 1]),
                 lambda: h.mes_logsurv([0.0]),
                 lambda: h.mes_bracket(),
                 lambda: h.acq(_lib.GP_ACQ_MES, 0.0, 0.0),
                 lambda: h.acq(_lib.GP_ACQ_EI | _lib.GP_ACQ_PER_COST, 0.01, 0.0)):
        with pytest.raises(RuntimeError, match="Laplace-fitted"):
            call()
    after = h.predict(include_noise=True)      # a refused call launches and changes nothing
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert h.laplace_info()[0] == fitted(cid).iters


def test_calls_that_overwrite_or_replace_the_fit_clear_the_state():
    p, c = LT.problem("a"), LT.CASES["a"]
    fresh = _handle("a")
    fresh.set_candidates(p.Xs)
    want = _regression_bits(fresh)
    # gp_kernel_matrix overwrites dA: the Laplace state goes with the factor, and the noise of gp_set_params is back
    h = _handle("a")
    h.set_candidates(p.Xs)
    h.laplace_fit(p.y)
    K = h.kernel_matrix()
    assert np.abs(K - _f(LT.fit("a").K)).max() <= 1e-12 * c.variance
    with pytest.raises(RuntimeError, match="not Laplace-fitted"):
        h.laplace_info()
    with pytest.raises(RuntimeError, match="not Laplace-fitted"):
        h.laplace_mode()
    got = _regression_bits(h)
    assert got[:3] == want[:3] and np.array_equal(got[4], want[4]) and np.array_equal(got[5][1], want[5][1])
    # a sparse fit is a regression fit: it clears the state and reads the noise gp_set_params gave, bit for bit; the entries over
    # a sparse fit are refused while the handle is Laplace-fitted (they read the context's noise)
    Z = p.X[:16].copy()
    fresh.sparse_set_inducing(Z)
    want_sparse = fresh.sparse_fit()
    want_pred = fresh.sparse_predict(p.Xs, include_noise=True)
    h.sparse_set_inducing(Z)
    assert h.sparse_fit() == want_sparse
    h.laplace_fit(p.y)
    with pytest.raises(RuntimeError, match="Laplace-fitted"):
        h.sparse_predict(p.Xs, include_noise=True)
    assert h.laplace_info()[0] >= 1                       # refused: the state stands
    assert h.sparse_fit() == want_sparse                  # ... and this clears it
    with pytest.raises(RuntimeError, match="not Laplace-fitted"):
        h.laplace_info()
    got_pred = h.sparse_predict(p.Xs, include_noise=True)
    for a, b in zip(want_pred, got_pred):
        assert np.array_equal(a, b)
    fresh.close()
    h.close()


def test_a_group_refuses_to_score_a_laplace_fitted_member_and_its_fit_clears_the_state():
    p, c = LT.problem("a"), LT.CASES["a"]
    grp = _lib.Group((0, 0))                              # two replicas on one device
    grp.set_data(p.X, p.labels01)
    grp.set_params(KID[c.fam], int(c.ard), c.variance, p.ls_arg, 0.37)
    want = grp.fit()
    fmin = grp.fmin()
    grp.set_candidates(p.Xs)
    best = grp.acq_argbest(_lib.GP_ACQ_EI, 0.01, fmin, -1)
    member = ctypes.c_void_p()
    assert grp.lib.gp_group_member(grp.h, 1, ctypes.byref(member)) == 0
    y = np.ascontiguousarray(p.y)
    assert grp.lib.gp_laplace_fit(member, dptr(y), LT.CAP, None, None, None, None, None) == 0
    for call in (grp.fmin, lambda: grp.acq_argbest(_lib.GP_ACQ_EI, 0.01, fmin, -1),
                 lambda: grp.acq_topk(_lib.GP_ACQ_EI, 0.01, fmin, -1, 2),
                 lambda: grp.acq_lp_argbest(_lib.GP_ACQ_EI, 0.01, fmin, 0, -1)):
        with pytest.raises(RuntimeError, match="Laplace-fitted"):
            call()
    assert grp.fit() == want                              # goes through, and clears the member's state
    assert grp.fmin() == fmin and grp.acq_argbest(_lib.GP_ACQ_EI, 0.01, fmin, -1) == best
    grp.close()


def test_a_regression_handle_is_untouched_by_a_laplace_fit_on_another_handle():
    p = LT.problem("c")
    reg = _handle("c")
    reg.set_candidates(p.Xs)
    want = _regression_bits(reg)
    want_rows = reg.predict_rows(p.Xs[:4], include_noise=True, grad=True)
    other = _handle("c")
    other.laplace_fit_grad(p.y, p.ls_arg.size)
    got_rows = reg.predict_rows(p.Xs[:4], include_noise=True, grad=True)
    for a, b in zip(want_rows, got_rows):
        assert np.array_equal(a, b)
    got = _regression_bits(reg)
    assert got[:3] == want[:3] and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    assert np.array_equal(got[5][0], want[5][0]) and np.array_equal(got[5][1], want[5][1])
    reg.close()
    other.close()


# ---- 6. binary constraints ----------------------------------------------------------------------------------------------------------
def _disc():
    """A 2-D problem whose feasible region is the disc of radius 0.3 around the centre of the unit square; N = 30."""
    rng = np.random.default_rng(77)
    X = rng.uniform(0, 1, (30, 2))
    X[0] = (0.5, 0.5)

    def f(x):
        x = np.atleast_2d(x)
        return (np.sin(3 * x[:, 0]) + (x[:, 1] - 0.3) ** 2)[:, None]

    def value(x):
        x = np.atleast_2d(x)
        return (x[:, 0] + x[:, 1] - 1.3)[:, None]

    def crashed(x):
        """1 where the run failed: outside the disc."""
        x = np.atleast_2d(x)
        return ((((x - 0.5) ** 2).sum(1) - 0.09) > 0).astype(float)[:, None]
    return X, f, value, crashed


def _mixed():
    X, f, value, crashed = _disc()
    Y, C = f(X), np.hstack([value(X), crashed(X)])
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, 1.0, 0.4), noise_var=1e-3, max_iters=0, verbose=False)
    gm.updateModel(X, (Y - Y.mean()) / Y.std(), None, None)
    fm = gpo.FeasibilityModel(2, [0.0, 0.0], kinds=['value', 'binary'], noise_var=1e-3, max_iters=0, verbose=False)
    fm.models[0].kernel = gpo.kern.Matern52(2, 1.0, 0.4)
    fm.models[1].kernel = gpo.kern.Matern52(2, 4.0, 0.3)
    fm.update(X, C)
    return X, Y, C, gm, fm


def test_a_value_and_a_binary_constraint_against_the_truth_fed_the_two_posteriors():
    X, Y, C, gm, fm = _mixed()
    pack = fm.device_pack()
    assert pack is not None and pack.K == 2 and type(fm.models[1]) is gpo.GPClassModel
    assert fm.c_mean[1] == 0.0 and fm.c_std[1] == 1.0 and fm.bounds[1] == 0.0
    assert fm.models[1].model._h.laplace_info()[0] >= 1
    rng = np.random.default_rng(5)
    for M in (1, 4, 8, 20):
        x = rng.uniform(0.05, 0.95, (M, 2))
        logF, dlogF = fm.log_probability_withGradients(x)
        hostF, dhostF = fm.log_probability_withGradients(x, host=True)
        post = [m.model._h.predict_rows(x[i:i + 1], include_noise=True, grad=True) for m in fm.models for i in range(M)]
        mean = np.array([q[0][0, 0] for q in post]).reshape(2, M)
        var = np.array([q[1][0, 0] for q in post]).reshape(2, M)
        dm = np.array([q[2][0, :, 0] for q in post]).reshape(2, M, 2)
        dv = np.array([q[3][0] for q in post]).reshape(2, M, 2)
        g = FT.fold(mean, var, dm, dv, pack.c_mean, pack.c_std, pack.bounds)       # the long-double fold of the two posteriors
        # two float64 routes to one posterior agree to 1e-9 (1e-8 for d var / dx), propagated through the fold: the bound of
        # tests/test_gpu_feas.py (_route_tolerance)
        d_dm = np.broadcast_to(1e-9 * np.maximum(np.abs(dm).max(axis=(1, 2)), 1e-3)[:, None, None], dm.shape)
        tl, td = FT.propagate(g, pack.c_std, 1e-9 * np.maximum(1.0, np.abs(mean)), 1e-9 * np.sqrt(var) + 1e-12, d_dm,
                              1e-8 * var[:, :, None] * np.ones_like(dv), dm, dv)
        e1 = float((np.abs(logF - g.logF) / (g.bound_logF + tl)).max())
        e2 = float((np.abs(dlogF - g.dlogF) / (g.bound_dlogF + td)).max())
        e3 = float((np.abs(logF - hostF) / (2 * (g.bound_logF + tl))).max())
        e4 = float((np.abs(dlogF - dhostF) / (2 * (g.bound_dlogF + td))).max())
        print("LAPLACE constraints M = %d: log F %.3g, its gradient %.3g of the bound against the truth; %.3g, %.3g against the "
              "host comparator" % (M, e1, e2, e3, e4))
        assert max(e1, e2, e3, e4) <= 1.0
        # the binary column alone is log p(label 0 | x)
        m1, s1 = fm.models[1].predict(x)
        assert np.all(np.abs(g.terms[1] - LT.log_ndtr(-m1.ravel() / s1.ravel())) <= 1e-7 * np.maximum(1, np.abs(_f(g.terms[1]))))


@pytest.mark.parametrize("cls", [gpo.AcquisitionEI, gpo.AcquisitionMPI])
def test_weighted_acquisition_table_and_arg_best(cls):
    X, Y, C, gm, fm = _mixed()
    ok = fm.feasible(C)
    assert 0 < ok.sum() < 30 and np.array_equal(ok, (C[:, 0] <= 0) & (C[:, 1] == 0))
    acq = cls(gm, jitter=0.01, feasibility=fm)
    assert acq._acq_id == acq._rule.device_id | FEAS and acq._route() is not None
    tab = np.random.default_rng(8).uniform(0, 1, (200, 2))
    v = acq.acquisition_function(tab)                       # gp_feas_table + GP_ACQ_TIMES_FEAS
    assert gm.model._h.feas_info() == (2, 200)
    fmin = gm.predict(X[ok], with_noise=False)[0].min()
    val = acq._rule.gradient(0.01, fmin, *gm.predict_withGradients(tab))[0]
    want = -(val * np.exp(fm.log_probability(tab, host=True))[:, None])
    assert np.max(np.abs(v - want)) <= 1e-6 * np.abs(want).max()
    i, best = acq.argbest(tab, -1)
    assert i == int(np.argmin(v)) and best == v[i, 0]
    a, da = acq.acquisition_function_withGradients(tab[:3])  # gp_acq_rows_feas
    assert np.max(np.abs(a - v[:3])) <= 1e-6 * np.abs(v).max() and np.all(np.isfinite(da))


def test_probability_of_feasibility_alone_while_no_row_is_feasible():
    X, f, value, crashed = _disc()
    Y = f(X)
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, 1.0, 0.4), noise_var=1e-3, max_iters=0, verbose=False)
    gm.updateModel(X, (Y - Y.mean()) / Y.std(), None, None)
    fm = gpo.FeasibilityModel(1, kinds=['binary'], max_iters=5, verbose=False)
    fm.update(X, np.ones((30, 1)))                          # every run crashed: one class only, fitted without a search
    assert fm.feasible_rows.size == 0
    acq = gpo.AcquisitionEI(gm, jitter=0.01, feasibility=fm)
    assert acq._acq_id == _lib.GP_ACQ_POF | FEAS
    x = np.random.default_rng(2).uniform(0.1, 0.9, (3, 2))
    a, da = acq.acquisition_function_withGradients(x)
    logF, dlogF = fm.log_probability_withGradients(x, host=True)
    assert np.all(logF < np.log(0.5))                        # crashes everywhere: satisfaction is improbable
    assert np.max(np.abs(a[:, 0] + np.exp(logF))) <= 1e-9 * np.exp(logF).max() + 1e-300
    assert np.max(np.abs(da + np.exp(logF)[:, None] * dlogF)) <= 1e-9 * np.abs(np.exp(logF)[:, None] * dlogF).max() + 1e-300


def test_bayesian_optimization_with_a_binary_constraint():
    X, f, value, crashed = _disc()
    np.random.seed(3)
    bo = gpo.BayesianOptimization(f, domain=[{"name": "x", "type": "continuous", "domain": (0, 1), "dimensionality": 2}], X=X[:10],
                                  constraint_function=crashed, constraint_kinds=['binary'], max_iters=0, exact_feval=True)
    assert bo.feasibility.kinds == ('binary',) and crashed(X[:10]).min() == 0.0
    x_opt, fx_opt = bo.run_optimization(max_iter=3)
    assert bo.X.shape[0] == 13 and bo.C.shape == (13, 1) and bo.feasibility.generation >= 3
    assert np.all(np.isfinite(bo.X)) and np.all((bo.X >= 0) & (bo.X <= 1))     # every suggestion finite and inside the domain
    assert crashed(x_opt)[0, 0] == 0.0                                          # the reported optimum is a feasible row
    ok = bo.feasibility.feasible(bo.C)
    assert fx_opt == bo.Y[ok, 0].min()
