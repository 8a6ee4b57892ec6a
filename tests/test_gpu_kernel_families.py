"""GPU: the Matern-3/2 and Exponential covariances (GP_KERNEL_MATERN32 / GP_KERNEL_EXPONENTIAL) through every entry point, against
the oracle with the two families of tests/_kernel_families.py.

Problem: X uniform in [0, 1]^3, N = 300 (three 128-tiles, the last one padded), Y = sin(3 sum x) + 0.1 eps, variance 1.3, noise
1e-2, M = 130 candidates (two tiles, the second padded) with Xs[0] = X[5]: a candidate ON a training point, r = 0, where the
Exponential's dK_dr / r is singular and the reference's _inv_dist (stationary.py:251-258) is 0.

Tolerances are the north star as tests/test_gpu_parity.py applies it: LML 1e-8, log det 1e-10, everything else 1e-6 of the
largest reference entry; K 1e-13 of the variance against direct-difference distances in long double.  Every comparison prints
its figure before it asserts.

The oracle of everything evaluated at the candidates takes its distances by direct differences (KF.make(..., direct=True)): with
Xs[0] = X[5] every such case holds a coincident pair, and on these inputs the Gram trick of stationary.py:155-173 returns r ~ 1e-8
there instead of 0.  For the Exponential (not differentiable at r = 0) that is 5e-6 of the variance at that candidate (2e-7 of
the largest one), 1e-7 of the largest dv/dx entry and, through log EI in the tail, 5e-6 of the largest penalised value: the oracle's error, measured between
the two oracle variants on the CPU (tests/test_kernel_families_host.py holds them to 1e-9 of each other everywhere else).  The fit-only
comparisons (gp_fit_grad_batch members, restarts) keep the Gram-trick oracle.
"""
import functools
import types

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

import _kernel_families as KF

pytestmark = pytest.mark.gpu

N, D, M = 300, 3, 130
VAR, NOISE, TOL = 1.3, 1e-2, 1e-6
KID = {"Mat32": _lib.GP_KERNEL_MATERN32, "Exponential": _lib.GP_KERNEL_EXPONENTIAL}
CASES = [pytest.param(f, a, id="%s-%s" % (f, "ard" if a else "iso")) for f in ("Mat32", "Exponential") for a in (False, True)]
ACQS = ((_lib.GP_ACQ_EI, 0.01, "EI"), (_lib.GP_ACQ_LCB, 2.0, "LCB"), (_lib.GP_ACQ_MPI, 0.01, "MPI"))
LP_L = 3.1


def _ls(ard):
    return np.array([0.4, 0.7, 1.1]) if ard else np.array([0.5])


@functools.lru_cache(maxsize=None)
def _problem():
    rng = np.random.default_rng(20260)
    X = rng.uniform(0, 1, (N, D))
    Y = (np.sin(3 * X.sum(1)) + 0.1 * rng.standard_normal(N))[:, None]
    Xs = rng.uniform(0, 1, (M, D))
    Xs[0] = X[5]
    Y2 = np.c_[Y, np.cos(2 * X.sum(1)) + 0.1 * rng.standard_normal(N)]
    for a in (X, Y, Xs, Y2):
        a.setflags(write=False)
    return X, Y, Xs, Y2


def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


@functools.lru_cache(maxsize=None)
def _ref(fam, ard):
    """The oracle's numbers of one case, computed once and shared (read-only) by every test that needs them."""
    X, Y, Xs, _ = _problem()
    gp = O.OracleGP(X, Y, KF.make(fam, D, VAR, _ls(ard), ard, direct=True), NOISE)
    gm = O.OracleGPModel(gp)
    p = gp.posterior
    r = types.SimpleNamespace(gp=gp, gm=gm, lml=p["lml"], logdet=p["logdet"], alpha=p["alpha"], Wi=p["Wi"], dL_dK=p["dL_dK"])
    r.dv, r.dl, r.dn = gp.gradients()
    r.mu, r.var = gp.predict(Xs)
    _, r.var0 = gp.predict_noiseless(Xs)
    _, r.cov = gp.predict(Xs, full_cov=True)
    r.dmdx, r.dvdx = gp.predictive_gradients(Xs)
    r.fmin = float(gm.get_fmin())
    fns = {"EI": lambda: O.acq_EI_withGradients(gm, Xs, 0.01, r.fmin), "LCB": lambda: O.acq_LCB_withGradients(gm, Xs, 2.0),
           "MPI": lambda: O.acq_MPI_withGradients(gm, Xs, 0.01, r.fmin)}
    r.neg, r.dneg = {}, {}
    for name, fn in fns.items():
        f, df = fn()
        r.neg[name], r.dneg[name] = -f, -df
        r.neg[name].setflags(write=False)
        r.dneg[name].setflags(write=False)
    r.Xb = np.array(Xs[[20, 41]] + 0.013)                     # nb = 2 batch points of the local penalisation
    r.r0, r.s0 = O.lp_hammer_precompute(gm, r.Xb, LP_L, float(Y.min()))
    return _freeze(r)


def _err(what, got, ref, tol, scale=None):
    """max |got - ref| against tol * (the largest reference entry, or `scale`); printed, then asserted."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), what
    s = float(np.max(np.abs(ref))) if scale is None else float(scale)
    e = float(np.max(np.abs(got - ref))) / max(s, 1e-300)
    print("%-34s err %.3e  tol %.1e" % (what, e, tol))
    assert e <= tol, (what, e, tol)


def _grad_err(what, got, ref, tol=TOL):
    """LML gradients as test_gpu_parity.py holds them: kernel entries against max(|dvariance|, max |dlengthscale|, 1), the noise
    entry against max(|dnoise|, 1)."""
    (dv, dl, dn), (dv0, dl0, dn0) = got, ref
    scale = max(abs(float(dv0)), float(np.max(np.abs(dl0))), 1.0)
    _err(what + " dvariance", dv, dv0, tol, scale)
    _err(what + " dlengthscale", dl, dl0, tol, scale)
    _err(what + " dnoise", dn, dn0, tol, max(abs(float(dn0)), 1.0))


@pytest.fixture(scope="module")
def h():
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", 0)
    yield hd
    hd.close()


def _fit(h, fam, ard, X=None, Y=None):
    Xd, Yd, Xs, _ = _problem()
    h.set_data(Xd if X is None else X, Yd if Y is None else Y)
    h.set_params(KID[fam], int(ard), VAR, _ls(ard), NOISE)
    out = h.fit()
    h.set_candidates(Xs)
    return out


# ---- 1. fit and matrices ------------------------------------------------------------------------------------------------------
def _check_fit_and_matrices(h, fam, ard):
    X, Y, Xs, _ = _problem()
    r = _ref(fam, ard)
    h.set_data(X, Y)
    h.set_params(KID[fam], int(ard), VAR, _ls(ard), NOISE)
    kd = KF.make(fam, D, VAR, _ls(ard), ard, direct=True, extended=True)
    K = h.kernel_matrix()
    _err("K(X, X)", K, kd.K(X).astype(np.float64), 1e-13, VAR)
    assert np.all(np.diag(K) == VAR) and np.array_equal(K, K.T)
    Kx = h.cross_kernel_matrix(Xs)
    _err("K(X, Xs)", Kx, kd.K(X, Xs).astype(np.float64), 1e-13, VAR)
    assert Kx[5, 0] == VAR                                     # the coincident pair: r = 0 exactly
    lml, logdet, jit = h.fit()
    assert jit == 0.0
    _err("lml", lml, r.lml, 1e-8)
    _err("logdet", logdet, r.logdet, 1e-10)
    _err("alpha", h.alpha(), r.alpha, TOL)
    rows = [0, 5, 127, 128, 255, 256, N - 1]
    Wi = h.woodbury_inv()
    assert np.array_equal(Wi, Wi.T)
    _err("woodbury_inv rows", Wi[rows], r.Wi[rows], TOL, np.max(np.abs(r.Wi)))
    _err("fmin", h.fmin(), r.fmin, TOL, max(1.0, abs(r.fmin)))
    g = h.lml_grad(_ls(ard).size)
    _grad_err("lml_grad", g, (r.dv, r.dl, r.dn))
    _err("dL_dK", h.dL_dK(), r.dL_dK, TOL)
    (lml2, logdet2, jit2), g2 = h.fit_grad(_ls(ard).size)
    assert (lml2, logdet2, jit2) == (lml, logdet, jit)
    assert g2[0] == g[0] and np.array_equal(g2[1], g[1]) and g2[2] == g[2]          # one call == two calls
    _grad_err("fit_grad", g2, (r.dv, r.dl, r.dn))


@pytest.mark.parametrize("fam,ard", CASES)
def test_fit_and_matrices(h, fam, ard):
    _check_fit_and_matrices(h, fam, ard)


# ---- 2. prediction ----------------------------------------------------------------------------------------------------------------
def _check_prediction(h, fam, ard):
    r = _ref(fam, ard)
    lml, _, _ = _fit(h, fam, ard)
    mu, var = h.predict(True)
    _err("mean", mu, r.mu, TOL)
    _err("var / var_ref (with noise)", var / r.var, np.ones_like(r.var), TOL)
    mu0, var0 = h.predict(False)
    _err("mean (noiseless call)", mu0, r.mu, TOL)
    _err("var (noiseless)", var0, r.var0, TOL, VAR)
    (lml1, _, _), mu1, var1 = h.fit_predict(True)
    assert lml1 == lml and np.array_equal(mu1, mu) and np.array_equal(var1, var)    # bitwise, as include/gphip.h promises
    mu2, cov = h.predict_full_cov(True)
    _err("full_cov mean", mu2, r.mu, TOL)
    _err("full_cov", cov, r.cov, TOL)
    dm, dv = h.predict_grad()
    _err("dmdx", dm, r.dmdx, TOL)
    _err("dvdx", dv, r.dvdx, TOL)
    _err("dmdx row 0 (on a training point)", dm[0], r.dmdx[0], TOL, np.max(np.abs(r.dmdx)))
    _err("dvdx row 0 (on a training point)", dv[0], r.dvdx[0], TOL, np.max(np.abs(r.dvdx)))
    dm_only = h.predict_grad(mean_only=True)
    _err("dmdx alone", dm_only, r.dmdx, TOL)


@pytest.mark.parametrize("fam,ard", CASES)
def test_prediction(h, fam, ard):
    _check_prediction(h, fam, ard)


def test_prediction_two_outputs(h):
    """P = 2 (Exponential, ARD): means and mean gradients per output, one variance."""
    fam, ard = "Exponential", True
    X, _, Xs, Y2 = _problem()
    gp = O.OracleGP(X, Y2, KF.make(fam, D, VAR, _ls(ard), ard, direct=True), NOISE)
    _fit(h, fam, ard, Y=Y2)
    _err("lml (P = 2)", h.fit_state()[0], gp.log_likelihood(), 1e-8)
    mu, var = h.predict(True)
    mu0, var0 = gp.predict(Xs)
    assert mu.shape == (M, 2)
    _err("mean (P = 2)", mu, mu0, TOL)
    _err("var / var_ref (P = 2)", var / var0, np.ones_like(var0), TOL)
    dm, dv = h.predict_grad()
    dm0, dv0 = gp.predictive_gradients(Xs)
    _err("dmdx (P = 2)", dm, dm0, TOL)
    _err("dvdx (P = 2)", dv, dv0, TOL)
    g = h.lml_grad(D)
    _grad_err("lml_grad (P = 2)", g, gp.gradients())


# ---- 3. acquisitions ----------------------------------------------------------------------------------------------------------------
def _same_row_or_tie(what, idx, want, ref, atol):
    print("%-34s device row %d, oracle row %d, score gap %.3e" % (what, idx, want, abs(ref[idx] - ref[want])))
    assert idx == want or abs(ref[idx] - ref[want]) <= 2 * atol, (what, idx, want)


@pytest.mark.parametrize("fam,ard", CASES)
def test_acquisitions(h, fam, ard):
    r = _ref(fam, ard)
    _fit(h, fam, ard)
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
            idxs, vals = h.acq_topk(t, par, r.fmin, sense, 5)
            order = np.argsort(ref[:, 0] if sense < 0 else -ref[:, 0], kind="stable")[:5]
            assert len(set(idxs.tolist())) == 5
            for j in range(5):
                _same_row_or_tie("%s topk %+d #%d" % (name, sense, j), int(idxs[j]), int(order[j]), ref[:, 0], atol)
                assert abs(vals[j] - ref[idxs[j], 0]) <= atol


@pytest.mark.parametrize("transform", [0, 1], ids=["log", "softplus"])
@pytest.mark.parametrize("fam,ard", CASES)
def test_local_penalisation(h, fam, ard, transform):
    """gp_acq_lp / gp_acq_lp_grad / gp_acq_lp_argbest over EI with nb = 2 batch points, both transforms, one excluded row."""
    _, _, Xs, _ = _problem()
    r = _ref(fam, ard)
    _fit(h, fam, ard)
    t, par, name = ACQS[0]
    tname = "softplus" if transform else "none"
    ref = O.lp_penalized_acquisition(r.neg[name], Xs, r.Xb, r.r0, r.s0, tname)
    dref = O.lp_d_acquisition(r.neg[name], r.dneg[name], Xs, r.Xb, r.r0, r.s0, tname)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(dref))
    atol = TOL * float(np.max(np.abs(ref)))
    _err("lp value", h.acq_lp(t, par, r.fmin, transform, r.Xb, r.r0, r.s0), ref, TOL)
    v, dv = h.acq_lp_grad(t, par, r.fmin, transform, r.Xb, r.r0, r.s0)
    _err("lp value (gradient call)", v, ref, TOL)
    _err("lp gradient", dv, dref, TOL)
    for sense, pick in ((-1, np.argmin), (+1, np.argmax)):
        first = int(pick(ref))
        idx, val = h.acq_lp_argbest(t, par, r.fmin, transform, sense, r.Xb, r.r0, r.s0)
        _same_row_or_tie("lp argbest %+d" % sense, idx, first, ref, atol)
        masked = np.ma.array(ref, mask=False)
        masked.mask[first] = True
        idx2, val2 = h.acq_lp_argbest(t, par, r.fmin, transform, sense, r.Xb, r.r0, r.s0, exclude=[first])
        assert idx2 != first
        _same_row_or_tie("lp argbest %+d, one row excluded" % sense, idx2, int(pick(masked)), ref, atol)
        assert abs(val2 - ref[idx2]) <= atol


# ---- 4. one-location calls --------------------------------------------------------------------------------------------------------
def _rows_bundle(h, x, r, via):
    """(mean, var, dmdx, dvdx, EI, dEI, LP(EI), dLP(EI)) of the rows x: through gp_*_rows, or through the batched entry points
    on the resident candidates (rows 0 .. len(x) - 1 of what gp_set_candidates holds)."""
    t, par, _ = ACQS[0]
    lp = (0, r.Xb, r.r0, r.s0)
    k = x.shape[0]
    if via == "rows":
        mu, var, dm, dv = h.predict_rows(x, True, grad=True)
        a, da = h.acq_rows(x, t, par, r.fmin, grad=True)
        v, dvl = h.acq_rows(x, t, par, r.fmin, grad=True, lp=lp)
        v_only = h.acq_rows(x, t, par, r.fmin, lp=lp)
        a_only = h.acq_rows(x, t, par, r.fmin)
        # value call against gradient call (|w|^2 summed per row or per row block), as tests/test_gpu_rows.py holds them
        assert np.max(np.abs(a_only - a)) <= 1e-8 * np.max(np.abs(a)) and np.max(np.abs(v_only - v)) <= 1e-6 * np.max(np.abs(v))
    else:
        mu, var = h.predict(True)
        dm, dv = h.predict_grad()
        a, da = h.acq_grad(t, par, r.fmin)
        v, dvl = h.acq_lp_grad(t, par, r.fmin, 0, r.Xb, r.r0, r.s0)
    return [np.asarray(q)[:k] for q in (mu, var, dm[:, :, 0], dv, a, da, v, dvl)]


ROWS_NAMES = ("mean", "var", "dmdx", "dvdx", "EI", "dEI", "LP(EI)", "dLP(EI)")


@pytest.mark.parametrize("fam,ard", CASES)
def test_one_location_calls(h, fam, ard):
    """gp_predict_rows / gp_acq_rows (lp = 0 and 1, with gradients) for M = 1, 3 and 6 on the fused route (one pass up to four
    locations, two for six; a single-output model of N <= 4096 always has the inverse factor), the same six rows as six resident
    candidates (M <= small_m: the matrix-vector route of smallm.hip with cross_k_rows_kernel) and as the first rows of the 130
    resident candidates (the tile route), and M = 9 through gp_*_rows, which takes the batched entry points inside.  Row 0 is ON a
    training point.  The routes agree to 1e-9 of each quantity's largest entry and each agrees with the oracle at 1e-6."""
    _, _, Xs, _ = _problem()
    r = _ref(fam, ard)
    _fit(h, fam, ard)
    x6 = np.array(Xs[:6])
    tile = _rows_bundle(h, x6, r, "batched")                  # 130 resident candidates
    h.set_candidates(x6)
    small = _rows_bundle(h, x6, r, "batched")                 # 6 resident candidates
    s0 = h.rows_stats()
    fused = {m: _rows_bundle(h, np.array(Xs[:m]), r, "rows") for m in (1, 3, 6)}
    s1 = h.rows_stats()
    assert s1["fused"] - s0["fused"] == 3 * 5 and s1["fallback"] == s0["fallback"]
    nine = _rows_bundle(h, np.array(Xs[:9]), r, "rows")
    s2 = h.rows_stats()
    assert s2["fallback"] - s1["fallback"] == 5 and s2["fused"] == s1["fused"]
    # the oracle: GPModel.predict_withGradients and the acquisitions over it, restated
    m0, sd0, dm0, ds0 = r.gm.predict_withGradients(x6)
    f0, df0 = O.acq_EI_withGradients(r.gm, x6, 0.01, r.fmin)
    oracle = [m0, sd0 ** 2, dm0, ds0 * 2 * sd0, -f0, -df0,
              O.lp_penalized_acquisition(-f0, x6, r.Xb, r.r0, r.s0, "none"),
              O.lp_d_acquisition(-f0, -df0, x6, r.Xb, r.r0, r.s0, "none")]
    for q, name in enumerate(ROWS_NAMES):
        scale = float(np.max(np.abs(tile[q])))
        _err("small-M vs tile: " + name, small[q], tile[q], 1e-9, scale)
        _err("rows M = 9 vs tile: " + name, nine[q][:6], tile[q], 1e-9, scale)
        for m in (1, 3, 6):
            _err("fused M = %d vs tile: %s" % (m, name), fused[m][q], tile[q][:m], 1e-9, scale)
        oscale = float(np.max(np.abs(oracle[q])))
        for label, got in (("tile", tile), ("small-M", small), ("fused M = 6", fused[6]), ("fused M = 1", fused[1])):
            k = got[q].shape[0]
            _err("%s vs oracle: %s" % (label, name), got[q], oracle[q][:k], TOL, oscale)
    # the mean's gradient alone (one pass over the training points), on and off the training point
    _err("mean_grad_rows", h.mean_grad_rows(x6)[:, :, 0], dm0, TOL)


# ---- 5. r = 0 in the hyper-parameter gradients ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,ard", CASES)
def test_duplicated_training_rows(h, fam, ard):
    """Rows 100..119 equal rows 0..19: twenty off-diagonal pairs at r = 0 exactly in lml_grad_tile_kernel.  Finite, and equal to
    the oracle on direct-difference distances (the Gram trick's r ~ 1e-8 at a duplicate is the oracle's noise; the Exponential is
    not differentiable there)."""
    X, Y, _, _ = _problem()
    X2 = np.array(X)
    X2[100:120] = X2[0:20]
    gp = O.OracleGP(X2, Y, KF.make(fam, D, VAR, _ls(ard), ard, direct=True), NOISE)
    ref = gp.gradients()
    assert np.all(np.isfinite(np.r_[ref[0], ref[1], ref[2]]))
    (lml, logdet, jit) = _fit(h, fam, ard, X=X2)
    assert jit == 0.0
    _err("lml (duplicates)", lml, gp.log_likelihood(), 1e-8)
    g = h.lml_grad(_ls(ard).size)
    assert np.all(np.isfinite(np.r_[g[0], g[1], g[2]]))
    _grad_err("lml_grad (duplicates)", g, ref)
    (lml2, _, _), g2 = h.fit_grad(_ls(ard).size)
    assert np.all(np.isfinite(np.r_[lml2, g2[0], g2[1], g2[2]]))
    _grad_err("fit_grad (duplicates)", g2, ref)
    # a candidate on a duplicated pair: two training points at r = 0
    h.set_candidates(X2[[3, 103, 150]])
    dm, dv = h.predict_grad()
    dm0, dv0 = gp.predictive_gradients(X2[[3, 103, 150]])
    _err("dmdx (duplicates)", dm, dm0, TOL)
    _err("dvdx (duplicates)", dv, dv0, TOL, VAR / float(np.min(_ls(ard))))


# ---- 6. batch ---------------------------------------------------------------------------------------------------------------------
def _close(a, b, rtol=1e-12):
    """tests/test_gpu_fit_grad_batch.py's criterion between the batch and the single call: lml, log det and jitter within rtol
    relative; the gradient entries within rtol of the member's largest one."""
    head = np.all(np.abs(a[:3] - b[:3]) <= rtol * np.abs(b[:3]))
    return bool(head and np.max(np.abs(a[3:] - b[3:])) <= rtol * np.max(np.abs(b[3:])))


@pytest.mark.parametrize("fam,ard", CASES)
def test_fit_grad_batch_members_equal_the_single_call(h, fam, ard):
    X, Y, _, _ = _problem()
    h.set_data(X, Y)
    nls = D if ard else 1
    var = np.array([1.3, 0.4, 2.5])
    ls = np.array([_ls(ard), _ls(ard) * 2.2, _ls(ard) * 0.6])
    noise = np.array([1e-2, 3e-2, 2e-3])
    h.set_params(KID[fam], int(ard), var[0], ls[0], noise[0])
    (lml, logdet, jit), (dv, dl, dn), status = h.fit_grad_batch(var, ls, noise)
    assert not status.any()
    for m in range(3):
        h.set_params(KID[fam], int(ard), var[m], ls[m], noise[m])
        (l1, d1, j1), (dv1, dl1, dn1) = h.fit_grad(nls)
        got, ref = np.r_[lml[m], logdet[m], jit[m], dv[m], dl[m], dn[m]], np.r_[l1, d1, j1, dv1, dl1, dn1]
        assert np.all(np.isfinite(got)) and got[2] == ref[2]
        print("member %d: max |batch - single| = %.3e" % (m, float(np.max(np.abs(got - ref)))))
        assert _close(got, ref), (m, got, ref)
        gp = O.OracleGP(X, Y, KF.make(fam, D, var[m], ls[m], ard), noise[m])
        _err("member %d lml" % m, lml[m], gp.log_likelihood(), 1e-8)
        _grad_err("member %d" % m, (dv[m], dl[m], dn[m]), gp.gradients())


@pytest.mark.parametrize("fam,ard", CASES)
def test_parallel_restarts_end_where_the_serial_restarts_end(fam, ard):
    """optimize_restarts(3, parallel=True, max_iters=20) at N = 60 against the serial run from the same seed, under the criterion of
    tests/test_restarts_lockstep.py: the same objective values and optimiser vectors per restart, the same final parameters and
    LML, the same random draws -- bitwise (below one panel the batch members run the single call's arithmetic)."""
    X, Y, _, _ = _problem()
    cls = gpo.kern.Matern32 if fam == "Mat32" else gpo.kern.Exponential

    def model():
        m = gpo.models.GPRegression(X[:60], Y[:60], cls(D, variance=1.0, ARD=ard), noise_var=0.05)
        m.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
        return m

    ms, mp = model(), model()
    np.random.seed(1234)
    runs_s = ms.optimize_restarts(3, verbose=False, max_iters=20)
    state_s = np.random.get_state()
    np.random.seed(1234)
    runs_p = mp.optimize_restarts(3, verbose=False, max_iters=20, parallel=True)
    state_p = np.random.get_state()
    assert state_s[0] == state_p[0] and np.array_equal(state_s[1], state_p[1]) and state_s[2:] == state_p[2:]
    assert len(runs_s) == len(runs_p) == 3
    for (fs, xs), (fp, xp) in zip(runs_s, runs_p):
        print("restart: serial %.12f parallel %.12f" % (fs, fp))
        assert np.isfinite(fs) and fs == fp and np.array_equal(xs, xp)
    assert np.array_equal(ms.optimizer_array, mp.optimizer_array)
    assert ms.log_likelihood() == mp.log_likelihood()
    ms.close()
    mp.close()


# ---- 7. host layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Matern32", "Exponential"])
def test_gpregression_checkgrad_and_methods(cls):
    X, Y, Xs, _ = _problem()
    fam = "Mat32" if cls == "Matern32" else "Exponential"
    ls = _ls(True)
    m = gpo.models.GPRegression(X, Y, getattr(gpo.kern, cls)(D, VAR, ls, ARD=True), noise_var=NOISE)
    np.random.seed(0)
    assert m.checkgrad()
    gp = O.OracleGP(X, Y, KF.make(fam, D, VAR, ls, True, direct=True), NOISE)
    _err("log_likelihood", m.log_likelihood(), gp.log_likelihood(), 1e-8)
    mu, var = m.predict(Xs)
    mu0, var0 = gp.predict(Xs)
    _err("predict mean", mu, mu0, TOL)
    _err("predict var", var / var0, np.ones_like(var0), TOL)
    _, v0 = m.predict_noiseless(Xs)
    _err("predict_noiseless var", v0, gp.predict_noiseless(Xs)[1], TOL, VAR)
    q, q0 = m.predict_quantiles(Xs), gp.predict_quantiles(Xs)
    for a, b in zip(q, q0):
        _err("predict_quantiles", a, b, TOL)
    dm, dv = m.predictive_gradients(Xs)
    dm0, dv0 = gp.predictive_gradients(Xs)
    _err("predictive_gradients mean", dm, dm0, TOL)
    _err("predictive_gradients var", dv, dv0, TOL)
    _err("posterior_covariance_between_points", m.posterior_covariance_between_points(Xs[:7], Xs[7:20]),
         gp.posterior_covariance_between_points(Xs[:7], Xs[7:20]), TOL, VAR)
    s = m.posterior_samples_f(Xs[:20], size=4)
    assert s.shape[0] == 20 and np.all(np.isfinite(s))
    m.optimize(max_iters=15)
    assert np.isfinite(m.log_likelihood()) and m.log_likelihood() >= gp.log_likelihood() - 1e-6
    m.close()


class _AllContinuous(object):
    """A design space of three continuous variables, as kern.gower_config reads one."""

    def get_continuous_dims(self):
        return [0, 1, 2]

    def get_discrete_dims(self):
        return []

    def lengthscales(self):
        return [1.0, 1.0, 1.0]


def test_aliases_are_the_same_device_kernel():
    X, _, Xs, _ = _problem()
    # kern.K evaluates on one scratch context per device: a Gower set-up left there by another kernel must not reach a family
    # the device refuses it for
    gpo.kern.Matern52(D, Gower=True, space=_AllContinuous()).K(X)
    assert np.array_equal(gpo.kern.OU(D).K(X), gpo.kern.Exponential(D).K(X))
    assert np.array_equal(gpo.kern.ExpQuad(D).K(X), gpo.kern.RBF(D).K(X))
    assert np.array_equal(gpo.kern.OU(D, 1.3, _ls(True), ARD=True).K(X, Xs), gpo.kern.Exponential(D, 1.3, _ls(True), ARD=True).K(X, Xs))
    k = gpo.kern.Matern32(D, VAR, _ls(False))
    kd = KF.make("Mat32", D, VAR, _ls(False), False, direct=True, extended=True)
    _err("kern.Matern32.K", k.K(X), kd.K(X).astype(np.float64), 1e-13, VAR)
    assert np.array_equal(k.Kdiag(X), np.full(N, VAR))


def test_gpmodel_and_acquisition_classes():
    """GPModel(kernel=kern.Matern32(3)).updateModel, then predict_withGradients and the acquisition classes against the oracle model
    at the fitted parameters."""
    X, Y, Xs, _ = _problem()
    np.random.seed(11)
    gm = gpo.GPModel(kernel=gpo.kern.Matern32(D), max_iters=30, optimize_restarts=2, verbose=False)
    gm.updateModel(X, Y, None, None)
    k = gm.model.kern
    v, ls, noise = float(k.variance), np.array(k.lengthscale.values), float(gm.model.likelihood.variance)
    print("fitted: variance %.4f lengthscale %s noise %.5f" % (v, ls, noise))
    gm0 = O.OracleGPModel(O.OracleGP(X, Y, KF.make("Mat32", D, v, ls, False, direct=True), noise))
    x = np.array(Xs[:20])
    m, s, dm, ds = gm.predict_withGradients(x)
    m0, s0, dm0, ds0 = gm0.predict_withGradients(x)
    _err("GPModel mean", m, m0, TOL)
    _err("GPModel sd", s / s0, np.ones_like(s0), TOL)
    _err("GPModel dmdx", dm, dm0, TOL)
    _err("GPModel dvdx", ds * 2 * s, ds0 * 2 * s0, TOL)
    f0 = gm0.get_fmin()
    _err("GPModel fmin", gm.get_fmin(), f0, TOL, max(1.0, abs(f0)))
    pairs = ((gpo.AcquisitionEI(gm), -O.acq_EI(gm0, Xs, 0.01, f0)), (gpo.AcquisitionLCB(gm), -O.acq_LCB(gm0, Xs, 2.0)),
             (gpo.AcquisitionMPI(gm), -O.acq_MPI(gm0, Xs, 0.01, f0)))
    for acq, ref in pairs:
        name = type(acq).__name__
        atol = TOL * float(np.max(np.abs(ref)))
        _err(name, acq.acquisition_function(Xs), ref, TOL)
        i, val = acq.argbest(Xs, -1)
        _same_row_or_tie(name + " argbest", i, int(np.argmin(ref)), ref[:, 0], atol)
        idx, vals = acq.topk(Xs, 5, -1)
        order = np.argsort(ref[:, 0], kind="stable")[:5]
        for j in range(5):
            _same_row_or_tie("%s topk #%d" % (name, j), int(idx[j]), int(order[j]), ref[:, 0], atol)
    gm.model.close()


def test_bayesian_optimization_by_kernel_name():
    X, Y, _, _ = _problem()
    np.random.seed(3)
    dom = [{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 3}]
    bo = gpo.methods.BayesianOptimization(f=None, domain=dom, X=X[:40], Y=Y[:40], kernel='Matern32', acquisition_type='EI',
                                          optimize_restarts=1, max_iters=30)
    x = bo.suggest_next_locations()
    assert x.shape == (1, 3) and np.all(np.isfinite(x)) and (x >= 0).all() and (x <= 1).all()
    assert type(bo.model.model.kern) is gpo.kern.Matern32
    bo.model.model.close()
    with pytest.raises(ValueError):
        gpo.methods.BayesianOptimization(f=None, domain=dom, X=X[:40], Y=Y[:40], kernel='Matern12')


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    X, Y, _, _ = _problem()
    hd = _lib.Handle(0)
    try:
        hd.set_data(X, Y)
        for bad in (4, -1, 17):
            with pytest.raises(ValueError, match="unknown kernel"):
                hd.set_params(bad, 0, VAR, [0.5], NOISE)
        assert hd.lib.gp_set_params(hd.h, 4, 0, VAR, _lib.dptr(np.array([0.5])), NOISE) == _lib.GP_ERR_ARG
        disc, rng = np.array([0, 0, 1]), np.array([1.0, 1.0, 1.0])
        for kid in (_lib.GP_KERNEL_MATERN32, _lib.GP_KERNEL_EXPONENTIAL):
            # gp_set_params first, gp_set_gower second
            hd.set_gower()
            hd.set_params(kid, 0, VAR, [0.5], NOISE)
            with pytest.raises(ValueError) as e:
                hd.set_gower(disc, rng)
            assert "gp_set_gower" in str(e.value) and "gp_set_params" in str(e.value)
            hd.fit()                                           # the refused call changed nothing: a Euclidean model of that family
            # gp_set_gower first, gp_set_params second
            hd.set_params(_lib.GP_KERNEL_MATERN52, 0, VAR, [0.5], NOISE)
            hd.set_gower(disc, rng)
            with pytest.raises(ValueError) as e:
                hd.set_params(kid, 0, VAR, [0.5], NOISE)
            assert "gp_set_gower" in str(e.value) and "gp_set_params" in str(e.value)
            # still usable with kernel 1, Gower on: the same numbers as a fresh context gives
            lml = hd.fit()[0]
            h2 = _lib.Handle(0)
            h2.set_data(X, Y)
            h2.set_params(_lib.GP_KERNEL_MATERN52, 0, VAR, [0.5], NOISE)
            h2.set_gower(disc, rng)
            assert h2.fit()[0] == lml
            h2.close()
    finally:
        hd.close()


# ---- 9. emulated arithmetic -----------------------------------------------------------------------------------------------------------
def test_emulated_fp64_matern32():
    """(1) and (2) for Matern-3/2 iso with the bulk contractions on the int8 matrix cores (option emulate_fp64 = 1): the same
    tolerances."""
    hd = _lib.Handle(0)
    try:
        hd.set_option("emulate_fp64", 1)
        _check_fit_and_matrices(hd, "Mat32", False)
        _check_prediction(hd, "Mat32", False)
    finally:
        hd.close()
