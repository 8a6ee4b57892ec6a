"""GPU: all four covariance families against the direct-distance oracle at the shapes of tests/_family_shapes.py -- every DU class
of kbuild_kernel / kbuild_batch_kernel / cross_k_kernel for the Matern-3/2 / Exponential pair, ARD gradients of one to four
passes of GP_GRAD_CH dimensions, split = 1 of launch_lml_grad, the one-location route at its argument limit, gp_fit_grad_batch
at D > 8, and inputs a thousand lengthscales from the origin.

References: OracleGP / OracleGPModel over KF.make(..., direct=True), one per (family, case), computed once and read-only.
tests/test_family_shapes_host.py holds that oracle to the Gram-trick one on every unshifted case, and shows why the shifted case
needs it.

Tolerances are the project's own (tests/test_gpu_parity.py, tests/test_gpu_kernel_families.py): K and K(X, Xs) 1e-13 of the
variance against distances kept in long double (case j: the derived bound of _family_shapes.k_tolerance), LML 1e-8, log det
1e-10, everything else 1e-6 of the largest reference entry, hyper-gradients scaled as _grad_err scales them.  Every comparison
prints its figure before it asserts.
"""
import functools

import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

import _family_shapes as FS
import _kernel_families as KF
from test_gpu_kernel_families import ACQS, TOL, _close, _err, _grad_err, _same_row_or_tie

pytestmark = pytest.mark.gpu

VAR, NOISE = FS.VAR, FS.NOISE


def _params(pairs):
    return [pytest.param(f, c, id="%s-%s" % (f, c)) for f, c in pairs]


SINGLE = _params(FS.SINGLE)
SINGLE_P1 = _params((f, c) for f, c in FS.SINGLE if FS.CASES[c].P == 1)


@functools.lru_cache(maxsize=None)
def _ref(fam, cid):
    """The oracle's numbers of one case, computed once and shared (read-only) by every test that needs them."""
    c = FS.CASES[cid]
    X, Y, Xs, ls = FS.problem(cid)
    gp = FS.oracle(fam, cid)
    p = gp.posterior
    r = FS.namespace(gp=gp, lml=p["lml"], logdet=p["logdet"], alpha=p["alpha"], jitter=p["jitter"])
    r.dv, r.dl, r.dn = gp.gradients()
    r.mu, r.var = gp.predict(Xs)
    _, r.var0 = gp.predict_noiseless(Xs)
    _, r.cov = gp.predict(Xs, full_cov=True)
    r.dmdx, r.dvdx = gp.predictive_gradients(Xs)
    kd = KF.make(fam, c.D, VAR, ls, c.ard, direct=True, extended=True)
    r.K, r.Kx = kd.K(X).astype(np.float64), kd.K(X, Xs).astype(np.float64)
    if c.P == 1:
        gm = r.gm = O.OracleGPModel(gp)
        r.fmin = float(gm.get_fmin())
        fns = {"EI": lambda: O.acq_EI_withGradients(gm, Xs, 0.01, r.fmin), "LCB": lambda: O.acq_LCB_withGradients(gm, Xs, 2.0),
               "MPI": lambda: O.acq_MPI_withGradients(gm, Xs, 0.01, r.fmin)}
        r.neg, r.dneg = {}, {}
        for name, fn in fns.items():
            f, df = fn()
            r.neg[name], r.dneg[name] = -f, -df
            r.neg[name].setflags(write=False)
            r.dneg[name].setflags(write=False)
    return FS.freeze(r)


@pytest.fixture(scope="module")
def h():
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", 0)
    yield hd
    hd.close()


def _set(h, fam, cid):
    c = FS.CASES[cid]
    X, Y, Xs, ls = FS.problem(cid)
    h.set_data(X, Y)
    h.set_params(FS.KERNEL_ID[fam], int(c.ard), VAR, ls, NOISE)
    return c, X, Y, Xs, ls


def _fit(h, fam, cid):
    c, X, Y, Xs, ls = _set(h, fam, cid)
    out = h.fit()
    h.set_candidates(Xs)
    return c, Xs, out


# ---- matrices ------------------------------------------------------------------------------------------------------------------
def _check_matrices(h, fam, cid):
    c, X, Y, Xs, ls = _set(h, fam, cid)
    r = _ref(fam, cid)
    ktol = FS.k_tolerance(cid)
    K = h.kernel_matrix()
    _err("K(X, X)", K, r.K, ktol, VAR)
    assert np.all(np.diag(K) == VAR) and np.array_equal(K, K.T)
    Kx = h.cross_kernel_matrix(Xs)
    _err("K(X, Xs)", Kx, r.Kx, ktol, VAR)
    assert Kx[FS.coincident_row(c), 0] == VAR                   # the coincident pair: r = 0 exactly


@pytest.mark.parametrize("fam,cid", SINGLE)
def test_matrices(h, fam, cid):
    _check_matrices(h, fam, cid)


# ---- fit and prediction --------------------------------------------------------------------------------------------------------
def _check_fit(h, fam, cid):
    c, X, Y, Xs, ls = _set(h, fam, cid)
    r = _ref(fam, cid)
    assert r.jitter == 0.0
    lml, logdet, jit = h.fit()
    assert jit == 0.0
    _err("lml", lml, r.lml, 1e-8)
    _err("logdet", logdet, r.logdet, 1e-10)
    _err("alpha", h.alpha(), r.alpha, TOL)
    if c.P == 1:
        _err("fmin", h.fmin(), r.fmin, TOL, max(1.0, abs(r.fmin)))
    else:
        with pytest.raises(ValueError):                        # gp_fmin is the acquisitions' incumbent: one output only
            h.fmin()
    g = h.lml_grad(ls.size)
    _grad_err("lml_grad", g, (r.dv, r.dl, r.dn))
    (lml2, logdet2, jit2), g2 = h.fit_grad(ls.size)
    print("fit_grad - (fit, lml_grad): lml %.3e, gradients %.3e" % (abs(lml2 - lml), float(np.max(np.abs(np.r_[g2[0] - g[0], g2[1] - g[1], g2[2] - g[2]])))))
    assert (lml2, logdet2, jit2) == (lml, logdet, jit)
    assert g2[0] == g[0] and np.array_equal(g2[1], g[1]) and g2[2] == g[2]          # one call == two calls
    _grad_err("fit_grad", g2, (r.dv, r.dl, r.dn))


def _check_prediction(h, fam, cid):
    r = _ref(fam, cid)
    c, Xs, (lml, _, _) = _fit(h, fam, cid)
    mu, var = h.predict(True)
    assert mu.shape == (c.M, c.P)
    _err("mean", mu, r.mu, TOL)
    _err("var / var_ref (with noise)", var / r.var, np.ones_like(r.var), TOL)
    mu0, var0 = h.predict(False)
    _err("mean (noiseless call)", mu0, r.mu, TOL)
    _err("var (noiseless)", var0, r.var0, TOL, VAR)
    (lml1, _, _), mu1, var1 = h.fit_predict(True)
    assert lml1 == lml and np.array_equal(mu1, mu) and np.array_equal(var1, var)    # bitwise, as include/gphip.h promises
    assert c.M <= 200
    mu2, cov = h.predict_full_cov(True)
    _err("full_cov mean", mu2, r.mu, TOL)
    _err("full_cov", cov, r.cov, TOL)
    dm, dv = h.predict_grad()
    for p in range(c.P):
        _err("dmdx, output %d" % p, dm[:, :, p], r.dmdx[:, :, p], TOL)
    _err("dvdx", dv, r.dvdx, TOL)
    _err("dmdx row 0 (on a training point)", dm[0], r.dmdx[0], TOL, np.max(np.abs(r.dmdx)))
    _err("dvdx row 0 (on a training point)", dv[0], r.dvdx[0], TOL, np.max(np.abs(r.dvdx)))
    dm_only = h.predict_grad(mean_only=True)
    for p in range(c.P):
        _err("dmdx alone, output %d" % p, dm_only[:, :, p], r.dmdx[:, :, p], TOL)


@pytest.mark.parametrize("fam,cid", SINGLE)
def test_fit_and_gradients(h, fam, cid):
    _check_fit(h, fam, cid)


@pytest.mark.parametrize("fam,cid", SINGLE)
def test_prediction(h, fam, cid):
    _check_prediction(h, fam, cid)


# ---- acquisitions (P = 1) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", SINGLE_P1)
def test_acquisitions(h, fam, cid):
    r = _ref(fam, cid)
    _fit(h, fam, cid)
    for t, par, name in ACQS:
        ref, dref = r.neg[name], r.dneg[name]
        atol = TOL * float(np.max(np.abs(ref)))
        _err(name, h.acq(t, par, r.fmin), ref, TOL)
        a, da = h.acq_grad(t, par, r.fmin)
        _err(name + " (gradient call)", a, ref, TOL)
        _err("d" + name, da, dref, TOL)
        for sense, pick in ((-1, np.argmin), (+1, np.argmax)):
            idx, val = h.acq_argbest(t, par, r.fmin, sense)
            _same_row_or_tie("%s argbest %+d" % (name, sense), idx, int(pick(ref[:, 0])), ref[:, 0], atol)
            assert abs(val - ref[idx, 0]) <= atol


# ---- one-location calls (P = 1) --------------------------------------------------------------------------------------------------
ROWS_NAMES = ("mean", "var", "dmdx", "dvdx", "EI", "dEI", "dmdx alone")


def _rows_bundle(h, x, fmin, via):
    """(mean, var, dmdx, dvdx, EI, dEI, dmdx alone) of the rows x: through gp_predict_rows / gp_acq_rows, or through
    gp_set_candidates and the batched entry points -- what the fallback of api_rows.hip calls."""
    t, par, _ = ACQS[0]
    if via == "rows":
        mu, var, dm, dv = h.predict_rows(x, True, grad=True)
        a, da = h.acq_rows(x, t, par, fmin, grad=True)
        dm1 = h.mean_grad_rows(x)
    else:
        h.set_candidates(x)
        mu, var = h.predict(True)
        dm, dv = h.predict_grad()
        a, da = h.acq_grad(t, par, fmin)
        dm1 = h.predict_grad(mean_only=True)
    return [np.array(q) for q in (mu, var, dm[:, :, 0], dv, a, da, dm1[:, :, 0])]


@pytest.mark.parametrize("fam,cid", SINGLE_P1)
def test_one_location_calls(h, fam, cid):
    """gp_predict_rows (with gradients), gp_acq_rows (EI, with gradients) and the mean's gradient alone for k = 1, min(M, 3) and
    min(M, 4) rows (case g: k = 3 as well, its first count past the limit).  rows_fused_ok (api_rows.hip) sends k <= small_m = 8
    rows of a single-output model to the fused kernels while min(k, ROWS_MAX_M = 4) * D <= ROWS_MAX_XS = 128 doubles, and to
    gp_set_candidates + the batched entry points otherwise; a model of N <= 4096 always has the inverse factor (rows_use_factor).
    The counters of gp_rows_stats must say so, three calls per k.  The two routes agree to 1e-9 of each quantity's largest entry
    and each agrees with the oracle at 1e-6.  Row 0 is ON a training point."""
    c = FS.CASES[cid]
    r = _ref(fam, cid)
    _fit(h, fam, cid)
    assert c.N <= 4096
    for k in FS.rows_counts(c):
        x = np.array(FS.rows_points(cid)[:k])
        assert x.shape == (k, c.D)
        batched = _rows_bundle(h, x, r.fmin, "batched")
        s0 = h.rows_stats()
        rows = _rows_bundle(h, x, r.fmin, "rows")
        s1 = h.rows_stats()
        fused = k <= 8 and min(k, 4) * c.D <= 128              # rows_fused_ok, api_rows.hip
        assert fused == FS.rows_fused(k, c.D)
        print("k = %d, %d doubles: %s; counters %s -> %s" % (k, min(k, 4) * c.D, "fused" if fused else "fallback", s0, s1))
        assert s1["fused"] - s0["fused"] == (3 if fused else 0) and s1["fallback"] - s0["fallback"] == (0 if fused else 3)
        m0, sd0, dm0, ds0 = r.gm.predict_withGradients(x)
        f0, df0 = O.acq_EI_withGradients(r.gm, x, 0.01, r.fmin)
        oracle = [m0, sd0 ** 2, dm0, ds0 * 2 * sd0, -f0, -df0, dm0]
        for q, name in enumerate(ROWS_NAMES):
            label = "k = %d %s" % (k, "fused" if fused else "fallback")
            _err("%s vs batched: %s" % (label, name), rows[q], batched[q], 1e-9)
            _err("%s vs oracle: %s" % (label, name), rows[q], oracle[q], TOL)
            _err("batched k = %d vs oracle: %s" % (k, name), batched[q], oracle[q], TOL)


# ---- emulated arithmetic ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", _params(FS.EMULATED))
def test_emulated_fp64(fam, cid):
    """Matrices, fit and prediction with the bulk contractions on the int8 matrix cores (option emulate_fp64 = 1), on a handle of
    its own: the same tolerances.  The family only enters kernels that the emulation does not replace, so two cases are enough."""
    hd = _lib.Handle(0)
    try:
        hd.set_option("emulate_fp64", 1)
        _check_matrices(hd, fam, cid)
        _check_fit(hd, fam, cid)
        _check_prediction(hd, fam, cid)
    finally:
        hd.close()


# ---- gp_fit_grad_batch at D > 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", _params(FS.BATCH))
def test_fit_grad_batch_members(h, fam, cid):
    """R = 3 members (tests/_family_shapes.members) through kbuild_batch_kernel<16, *> / <0, *> and one to four passes of
    lml_grad_tile_batch_kernel: each member against the single gp_fit_grad under tests/test_gpu_fit_grad_batch.py's criterion
    (1e-12; the same bits where Npad <= 768, below one panel) and against the oracle."""
    c, X, Y, Xs, ls0 = _set(h, fam, cid)
    var, ls, noise = FS.members(cid)
    (lml, logdet, jit), (dv, dl, dn), status = h.fit_grad_batch(var, ls, noise)
    assert status.shape == (3,) and not status.any()
    exact = 0
    for m in range(3):
        h.set_params(FS.KERNEL_ID[fam], int(c.ard), var[m], ls[m], noise[m])
        (l1, d1, j1), (dv1, dl1, dn1) = h.fit_grad(ls0.size)
        got, ref = np.r_[lml[m], logdet[m], jit[m], dv[m], dl[m], dn[m]], np.r_[l1, d1, j1, dv1, dl1, dn1]
        assert np.all(np.isfinite(got)) and got[2] == ref[2]
        print("member %d: max |batch - single| = %.3e" % (m, float(np.max(np.abs(got - ref)))))
        assert _close(got, ref), (m, got, ref)
        exact += int(np.array_equal(got, ref))
        gp = FS.oracle(fam, cid, m)
        assert gp.posterior["jitter"] == 0.0 and jit[m] == 0.0
        _err("member %d lml" % m, lml[m], gp.log_likelihood(), 1e-8)
        _grad_err("member %d" % m, (dv[m], dl[m], dn[m]), gp.gradients())
    if -(-c.N // 128) * 128 <= 768:
        assert exact == 3
