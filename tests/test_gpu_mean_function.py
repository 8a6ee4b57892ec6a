"""GPU: the affine mean function m(x) = x^T A + b (gp_mean_set / gp_mean_info / gp_mean_grad) through fit, posterior and scoring,
against the exact GP with a mean in long double (tests/_mean_truth.py; tests/test_mean_truth_host.py holds it to the pinned oracle).

Cases (``_mean_truth.TABLE``): N 1, 127, 128, 129, 255, 256, 257 (tile edges; either side of the 256-row chunk of gp_mean_grad);
D 1, 3, 64; P 1, 3, 16; A alone, b alone, both; the four families, ARD and not; a Gower model in a test of its own.

Bound against the truth, the convention of tests/test_gpu_ensemble_sizes.py:  err <= max(MULT x e64, FLOOR_N x scale), e64 the
float64 oracle's own error against the same truth (capped at 1e-9 x scale on the CPU), scale the largest truth entry, MULT = 64,
FLOOR_N = 1e-13 max(1, Npad / 384) -- both taken from tests/_ens_truth.py.  Every figure is printed before it is asserted (lines
TRUTH, in that module's format; tools/mean_errors.py collects them into profiles/mean_errors.txt).  Rows against table: the bounds
of tests/test_gpu_rows.py at noise 1e-2.  "The same bits" is ``np.array_equal``.
"""
import ctypes

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

import _family_shapes as FS
import _mean_truth as MT

pytestmark = pytest.mark.gpu

ACQ = {"EI": _lib.GP_ACQ_EI, "LCB": _lib.GP_ACQ_LCB, "MPI": _lib.GP_ACQ_MPI}
ALL = [c.id for c in MT.TABLE]


def truth(what, dev, oracle, true, N):
    """One quantity against the long-double truth under the rule of the module docstring."""
    true = np.asarray(true, dtype=MT.T)
    e64, scale = MT.e64_of(oracle, true)
    err = float(np.max(np.abs(np.asarray(dev, dtype=MT.T).reshape(true.shape) - true)))
    floor = MT.floor_n(N) * scale
    bound = max(MT.MULT * e64, floor)
    print("TRUTH %-44s scale %.3e  device %.3e  oracle %.3e  ratio %7.2f  bound %.3e  floor %.3e"
          % (what, scale, err, e64, err / max(e64, 1e-300), bound, floor))
    return err <= bound, what


def failed(res):
    return [w for ok, w in res if not ok]


def handle(cid, mean=True):
    p = MT.problem(cid)
    c = p.case
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(p.X, p.Y)
    h.set_params(FS.KERNEL_ID[c.fam], int(c.ard), MT.VAR, p.ls, MT.NOISE)
    if mean:
        h.mean_set(p.A, p.b)
    return h, p


# ---- fit, LML, alpha, the hyper-gradients, dA and db -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ALL)
def test_fit_and_gradients_against_the_truth(cid):
    h, p = handle(cid)
    c, tr, orc, res = p.case, MT.truth(cid), MT.oracle64(cid), []
    assert h.mean_info() == ("A" in c.parts, "b" in c.parts)
    nls = c.D if c.ard else 1
    (lml, logdet, jit), (dv, dl, dn) = h.fit_grad(nls)
    alpha, (dA, db) = h.alpha(), h.mean_grad()
    assert jit == 0.0
    for what, dev, f in (("lml", lml, "lml"), ("logdet", logdet, "logdet"), ("alpha", alpha, "alpha"), ("dvariance", dv, "dvar"),
                         ("dlengthscale", dl, "dls"), ("dnoise", dn, "dnoise"), ("dA", dA, "dA"), ("db", db, "db")):
        res.append(truth("%s: %s" % (cid, what), dev, getattr(orc, f), getattr(tr, f), c.N))
    # the same bits on a second call, and from the separate entries (gp_fit, gp_lml_grad run unchanged on the residuals)
    dA2, db2 = h.mean_grad()
    assert np.array_equal(dA, dA2) and np.array_equal(db, db2)
    h.mean_set(p.A, p.b)       # the residuals are rebuilt: the same inputs give the same bits
    assert h.fit()[0] == lml and np.array_equal(h.alpha(), alpha)
    dv2, dl2, dn2 = h.lml_grad(nls)
    assert (dv2, dn2) == (dv, dn) and np.array_equal(dl2, dl)
    assert all(np.array_equal(a, b) for a, b in zip(h.mean_grad(), (dA, db)))
    h.close()
    assert not failed(res), failed(res)


# ---- tables: one chunk, two tiles, three chunks of 128 -----------------------------------------------------------------------------
@pytest.mark.parametrize("M", MT.TABLE_MS)
@pytest.mark.parametrize("cid", ALL)
def test_tables_against_the_truth(cid, M):
    h, p = handle(cid)
    c, res = p.case, []
    if M == 300:
        h.set_option("mc_max", 128)
    tab = MT.table(cid, M)
    mu_t, v0_t, v1_t, dm_t, dv_t = MT.truth_table(cid, M)
    mu_o, v0_o, v1_o, dm_o, dv_o = MT.oracle64_table(cid, M)
    h.set_candidates(tab)
    (lml, _, _), mu_fp, var_fp = h.fit_predict(True)       # one call: fit and table
    mu, var = h.predict(True)
    assert np.array_equal(mu, mu_fp) and np.array_equal(var, var_fp)
    _, var0 = h.predict(False)
    dm, dv = h.predict_grad()
    dm_only = h.predict_grad(mean_only=True)
    name = "%s table %d " % (cid, M)
    res.append(truth(name + "mean", mu, mu_o, mu_t, c.N))
    res.append(truth(name + "var", var, v1_o, v1_t, c.N))
    res.append(truth(name + "var (no noise)", var0, v0_o, v0_t, c.N))
    res.append(truth(name + "dmdx", dm, dm_o, dm_t, c.N))
    res.append(truth(name + "dmdx (alone)", dm_only, dm_o, dm_t, c.N))
    res.append(truth(name + "dvdx", dv, dv_o, dv_t, c.N))
    if M == 9:      # the full-covariance entry serves the same mean
        mu_fc, _ = h.predict_full_cov(True)
        res.append(truth(name + "mean (full cov)", mu_fc, mu_o, mu_t, c.N))
    h.close()
    assert not failed(res), failed(res)


# ---- rows: M = 1 .. 8 against the truth and against the table ---------------------------------------------------------------------------
def _fused(M, D):
    return min(M, 4) * D <= 128


@pytest.mark.parametrize("cid", MT.SINGLE)
def test_rows_against_the_truth_and_the_table(cid):
    h, p = handle(cid)
    c, tr, orc, res = p.case, MT.truth(cid), MT.oracle64(cid), []
    h.fit()
    x = MT.points(cid)
    ls_min = float(np.min(p.ls))
    cancel, vscale = np.abs(h.alpha()).sum() * MT.VAR / ls_min, MT.VAR / ls_min
    for M in range(1, 9):
        before, passes = h.rows_stats(), h.rows_pass_stats()
        mu, var, dm, dv = h.predict_rows(x[:M], True, grad=True)
        mu_v, var_v = h.predict_rows(x[:M], True)
        _, var0 = h.predict_rows(x[:M], False)
        dm_only = h.mean_grad_rows(x[:M])
        after, passes2 = h.rows_stats(), h.rows_pass_stats()
        if _fused(M, c.D):
            assert after["fused"] - before["fused"] == 4 and after["fallback"] == before["fallback"]
            wide = M > 4
            assert (passes2["wide"] - passes["wide"] > 0) == wide and (passes2["narrow"] - passes["narrow"] > 0) == (not wide)
        else:
            assert after["fallback"] - before["fallback"] == 4
        name = "%s rows %d " % (cid, M)
        res.append(truth(name + "mean", mu, orc.mu[:M], tr.mu[:M], c.N))
        res.append(truth(name + "mean (value call)", mu_v, orc.mu[:M], tr.mu[:M], c.N))
        res.append(truth(name + "var", var, orc.var[1][:M], tr.var[1][:M], c.N))
        res.append(truth(name + "var (value call)", var_v, orc.var[1][:M], tr.var[1][:M], c.N))
        res.append(truth(name + "var (no noise)", var0, orc.var[0][:M], tr.var[0][:M], c.N))
        res.append(truth(name + "dmdx", dm, orc.dm[:M], tr.dm[:M], c.N))
        res.append(truth(name + "dmdx (alone)", dm_only, orc.dm[:M], tr.dm[:M], c.N))
        res.append(truth(name + "dvdx", dv, orc.dv[:M], tr.dv[:M], c.N))
        # against the table: the bounds of tests/test_gpu_rows.py (noise >= 1e-4: rel = 1e-9)
        h.set_candidates(x[:M])
        mu_b, var_b = h.predict(True)
        dm_b, dv_b = h.predict_grad()
        rel = 1e-9
        assert np.max(np.abs(mu - mu_b)) <= rel * np.max(np.abs(mu_b))
        assert np.max(np.abs(dm - dm_b)) <= rel * np.max(np.abs(dm_b)) + 1e-13 * cancel
        assert np.max(np.abs(dv - dv_b)) <= max(rel, 1e-8) * np.max(np.abs(dv_b)) + 1e-12 * vscale
        assert np.max(np.abs(var - var_b) / np.abs(var_b)) <= rel
    h.close()
    assert not failed(res), failed(res)


def _rows_of(h, x, fmin):
    mu, var, dm, dv = h.predict_rows(x, True, grad=True)
    a, da = h.acq_rows(x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    return mu, var, dm, dv, a, da, h.mean_grad_rows(x), h.predict_rows(x, False)[0]


def _same_bits_in_every_slot(h, x, widths):
    """Location x[0] alone, then in every slot of calls of the given widths with the other locations as company."""
    fmin = h.fmin()
    alone = _rows_of(h, x[:1], fmin)
    for M in widths:
        for slot in range(M):
            order = list(range(1, M))
            order.insert(slot, 0)
            got = _rows_of(h, x[order], fmin)
            for a, g in zip(alone, got):
                assert np.array_equal(a[0], g[slot]), (M, slot)


@pytest.mark.parametrize("cid,widths", [("d", (2, 4, 5, 8)), ("g", (2,)), ("f", (3, 7))])
def test_a_location_keeps_its_bits_in_every_slot_and_company(cid, widths):
    """Narrow passes (M <= 4), wide ones (5 .. 8) and D = 64, where two locations share a pass."""
    h, p = handle(cid)
    h.fit()
    before = h.rows_stats()
    _same_bits_in_every_slot(h, MT.points(cid), widths)
    assert h.rows_stats()["fallback"] == before["fallback"]
    h.close()


# ---- a Gower model: m never enters K ------------------------------------------------------------------------------------------------
def test_gower_model_with_a_mean():
    """A Gower handle with a resident mean against the same handle without one, fitted to residuals formed on the host, plus m(x*)
    and A added on the host.  The two differ in how the residuals are rounded (fma chain against NumPy's dot: 2 eps (|y| + sum
    |x A| + |b|) per target) and in the last addition; through Ky^-1 that is at most eps cond(Ky) of the scale, cond(Ky) <=
    (N variance + noise) / noise = 1.7e4 here: 4 eps cond = 1.5e-11 of each quantity's scale.  Slots and company keep their bits."""
    p = MT.problem("d")
    N, D = p.X.shape
    rng = np.random.default_rng(77)
    X = p.X.copy()
    X[:, 2] = rng.integers(0, 4, N)                       # a discrete variable
    disc, ranges = np.array([0, 0, 1]), np.array([1.0, 1.0, 1.0])
    x = MT.points("d").copy()
    x[:, 2] = rng.integers(0, 4, 8)
    x[0] = X[5]
    mX = X @ p.A + p.b
    hs = []
    for Y, mean in ((p.Y, True), (p.Y - mX, False)):
        h = _lib.Handle(0)
        h.set_option("emulate_fp64", 0)
        h.set_data(X, Y)
        h.set_params(FS.KERNEL_ID["Mat52"], 1, MT.VAR, np.array([0.5, 0.8, 1.0]), MT.NOISE)
        h.set_gower(disc, ranges)
        if mean:
            h.mean_set(p.A, p.b)
        hs.append(h)
    hm, h0 = hs
    lml, lml0 = hm.fit()[0], h0.fit()[0]
    tol = 4 * np.finfo(float).eps * (N * MT.VAR + MT.NOISE) / MT.NOISE
    print("GOWER lml %.12f %.12f tol %.2e" % (lml, lml0, tol))
    assert abs(lml - lml0) <= tol * abs(lml0)
    assert np.max(np.abs(hm.alpha() - h0.alpha())) <= tol * np.max(np.abs(h0.alpha()))
    assert abs(hm.fmin() - _train_min(h0, X, mX)) <= tol * 10.0
    for M in (1, 3, 8):
        mu, var, dm, dv = hm.predict_rows(x[:M], True, grad=True)
        mu0, var0, dm0, dv0 = h0.predict_rows(x[:M], True, grad=True)
        assert np.max(np.abs(mu - (mu0 + x[:M] @ p.A + p.b))) <= tol * max(np.max(np.abs(mu)), 1.0)
        assert np.max(np.abs(dm - (dm0 + p.A[None]))) <= tol * max(np.max(np.abs(dm)), 1.0)
        assert np.array_equal(var, var0) and np.array_equal(dv, dv0)      # the variance never sees the targets
    hm.set_candidates(x)
    h0.set_candidates(x)
    assert np.max(np.abs(hm.predict(True)[0] - (h0.predict(True)[0] + x @ p.A + p.b))) <= tol * 10.0
    _same_bits_in_every_slot(hm, x, (2, 4, 6))
    hm.close()
    h0.close()


def _train_min(h0, X, mX):
    h0.set_candidates(X)
    return float((h0.predict(False)[0] + mX).min())


# ---- clearing the mean ------------------------------------------------------------------------------------------------------------------
def test_a_cleared_mean_leaves_the_bits_of_a_context_that_never_had_one():
    h, p = handle("d")
    h.fit()
    h.predict_rows(MT.points("d")[:3], True, grad=True)
    h.mean_set(None, None)
    assert h.mean_info() == (False, False)
    never, _ = handle("d", mean=False)
    x, tab = MT.points("d"), MT.table("d", 9)
    out = []
    for hd in (h, never):
        lml = hd.fit()
        hd.set_candidates(tab)
        out.append((np.array(lml), hd.alpha(), *hd.predict(True), *hd.predict_grad(), *hd.predict_rows(x[:3], True, grad=True),
                    hd.mean_grad_rows(x[:2]), np.array(hd.fmin())))
        hd.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- scores -----------------------------------------------------------------------------------------------------------------------------
def _score_refs(cid, rec_t, rec_o, sl):
    """{name: (truth's rule values, gradients, the oracle's values, gradients)} over the posterior records' rows ``sl``."""
    tr, orc = MT.truth(cid), MT.oracle64(cid)
    f_t, f_o = float(tr.train_mean.min()), float(orc.train_mean.min())
    out = {}
    for name in MT.RULES:
        out[name] = (MT.scores(name, rec_t[0][sl, 0], rec_t[2][sl], rec_t[3][sl, :, 0], rec_t[4][sl], f_t)
                     + MT.scores(name, rec_o[0][sl, 0], rec_o[2][sl], rec_o[3][sl, :, 0], rec_o[4][sl], f_o))
    return out


@pytest.mark.parametrize("cid", ["b", "d"])
def test_scores_on_table_and_rows(cid):
    h, p = handle(cid)
    c, tr, orc, res = p.case, MT.truth(cid), MT.oracle64(cid), []
    h.fit()
    fmin = h.fmin()
    res.append(truth("%s: fmin" % cid, fmin, orc.train_mean.min(), tr.train_mean.min(), c.N))
    M = 130
    tab = MT.table(cid, M)[:, :]
    inside = np.all((tab > -0.1) & (tab < 1.1), axis=1)          # (EI of the far point underflows: nothing to compare there)
    rec_t, rec_o = MT.truth_table(cid, M), MT.oracle64_table(cid, M)
    refs = _score_refs(cid, rec_t, rec_o, slice(None))
    h.set_candidates(tab)
    for name, t in ACQ.items():
        par = MT.RULES[name][1]
        a, da = h.acq_grad(t, par, fmin)
        a_only = h.acq(t, par, fmin)
        assert np.array_equal(a, a_only)
        v_t, g_t, v_o, g_o = refs[name]
        res.append(truth("%s table %s value" % (cid, name), a[inside, 0], v_o[inside], v_t[inside], c.N))
        res.append(truth("%s table %s gradient" % (cid, name), da[inside], g_o[inside], g_t[inside], c.N))
        for k in (1, 4, 7):
            r, dr = h.acq_rows(tab[:k], t, par, fmin, grad=True)
            res.append(truth("%s rows %d %s value" % (cid, k, name), r[:, 0], v_o[:k], v_t[:k], c.N))
            res.append(truth("%s rows %d %s gradient" % (cid, k, name), dr, g_o[:k], g_t[:k], c.N))
    # the penalised entries (EI, log transform, a batch of three): table and rows
    Xb, r0, s0 = tab[20:23], np.array([0.05, 0.2, 0.01]), np.array([0.03, 0.1, 0.02])
    v_t, g_t, v_o, g_o = refs["EI"]
    lp_t = O.lp_penalized_acquisition(v_t[:, None], tab, Xb, r0, s0, "none")
    lp_o = O.lp_penalized_acquisition(v_o[:, None], tab, Xb, r0, s0, "none")
    dlp_t = O.lp_d_acquisition(v_t[:, None], g_t, tab, Xb, r0, s0, "none")
    dlp_o = O.lp_d_acquisition(v_o[:, None], g_o, tab, Xb, r0, s0, "none")
    ok = inside & np.isfinite(lp_t) & (np.arange(M) < 20)        # away from the batch's own rows (their penalty is -inf)
    v, dv = h.acq_lp_grad(_lib.GP_ACQ_EI, 0.01, fmin, 0, Xb=Xb, r_x0=r0, s_x0=s0)
    res.append(truth("%s table lp EI value" % cid, np.ravel(v)[ok], lp_o[ok], lp_t[ok], c.N))
    res.append(truth("%s table lp EI gradient" % cid, dv[ok], dlp_o[ok], dlp_t[ok], c.N))
    v, dv = h.acq_rows(tab[:6], _lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=(0, Xb, r0, s0))
    res.append(truth("%s rows 6 lp EI value" % cid, np.ravel(v), lp_o[:6], lp_t[:6], c.N))
    res.append(truth("%s rows 6 lp EI gradient" % cid, dv, dlp_o[:6], dlp_t[:6], c.N))
    # GP_ACQ_PER_COST: the cost divides after the rule, the mean enters before it
    rng = np.random.default_rng(5)
    Xc, ac = rng.uniform(0, 1, (40, c.D)), rng.standard_normal(40)
    h.cost_set(Xc, ac, 0, 0, 1.0, np.array([0.6]), 0.1, 0.5)
    logc, dlogc = h.cost_rows(tab, grad=True)
    cost = np.exp(logc)
    a, da = h.acq_grad(_lib.GP_ACQ_EI | _lib.GP_ACQ_PER_COST, 0.01, fmin)
    res.append(truth("%s table EI per cost value" % cid, a[inside, 0], (v_o / cost)[inside], (v_t / cost)[inside], c.N))
    res.append(truth("%s table EI per cost gradient" % cid, da[inside], ((g_o - v_o[:, None] * dlogc) / cost[:, None])[inside],
                     ((g_t - v_t[:, None] * dlogc) / cost[:, None])[inside], c.N))
    r, dr = h.acq_rows(tab[:5], _lib.GP_ACQ_EI | _lib.GP_ACQ_PER_COST, 0.01, fmin, grad=True)
    res.append(truth("%s rows 5 EI per cost value" % cid, r[:, 0], (v_o / cost)[:5], (v_t / cost)[:5], c.N))
    h.close()
    assert not failed(res), failed(res)


def test_argbest_and_topk_are_exact_with_ties_to_the_lowest_index():
    h, p = handle("d")
    h.fit()
    fmin = h.fmin()
    tab = MT.table("d", 130)
    h.set_candidates(tab)
    first = h.acq(_lib.GP_ACQ_LCB, 2.0, fmin)[:, 0]
    best = int(np.argmin(first))
    tied = np.vstack([tab, tab[best], tab[3], tab[best]])        # rows 130 and 132 tie with the winner, row 131 with row 3
    h.set_candidates(tied)
    for name, t in ACQ.items():
        par = MT.RULES[name][1]
        vals = h.acq(t, par, fmin)[:, 0]
        assert vals[130] == vals[best] == vals[132] and vals[131] == vals[3]
        for sense in (-1, 1):
            key = vals if sense < 0 else -vals
            i, v = h.acq_argbest(t, par, fmin, sense)
            assert i == int(np.argmin(key)) and v == vals[i]
            idx, tv = h.acq_topk(t, par, fmin, sense, 6)
            want = np.argsort(key, kind="stable")[:6]
            assert np.array_equal(idx, want) and np.array_equal(tv, vals[want])
    i, _ = h.acq_argbest(_lib.GP_ACQ_LCB, 2.0, fmin, -1)
    assert i == best                                              # the lowest index among the three tied winners
    h.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------
def test_the_mean_survives_params_and_same_shape_data_and_another_shape_drops_it():
    h, p = handle("d")
    c = p.case
    lml = h.fit()[0]
    h.set_params(FS.KERNEL_ID[c.fam], int(c.ard), MT.VAR, p.ls, MT.NOISE)
    assert h.mean_info() == (True, True) and h.fit()[0] == lml
    Y2 = p.Y[::-1].copy()
    h.set_data(p.X, Y2)                                          # same D and P: the mean stays, the residuals are rebuilt
    h.set_params(FS.KERNEL_ID[c.fam], int(c.ard), MT.VAR, p.ls, MT.NOISE)
    assert h.mean_info() == (True, True)
    gp = MT.MeanGP(c.fam, c.ard, MT.VAR, p.ls, MT.NOISE, p.X, Y2, p.A, p.b, MT.F64)
    assert abs(h.fit()[0] - float(gp.lml)) <= 1e-9 * abs(float(gp.lml))
    h.set_data(p.X[:, :2].copy(), p.Y)                          # another D drops it
    assert h.mean_info() == (False, False)
    h.set_data(p.X, p.Y)
    h.mean_set(p.A, p.b)
    h.set_data(p.X, np.hstack([p.Y, p.Y]))                       # another P drops it
    assert h.mean_info() == (False, False)
    h.close()


def test_argument_and_state_errors():
    h = _lib.Handle(0)
    assert h.lib.gp_mean_set(h.h, None, None) == _lib.GP_ERR_STATE                      # needs gp_set_data
    p = MT.problem("d")
    h.set_data(p.X, p.Y)
    h.set_params(2, 0, MT.VAR, p.ls, MT.NOISE)
    dA, db = np.empty((3, 1)), np.empty(1)
    assert h.lib.gp_mean_grad(h.h, _lib.dptr(dA), _lib.dptr(db)) == _lib.GP_ERR_STATE   # needs a fit
    bad = p.A.copy()
    bad[1, 0] = np.nan
    with pytest.raises(ValueError):
        h.mean_set(bad, p.b)
    with pytest.raises(ValueError):
        h.mean_set(p.A, np.array([np.inf]))
    assert h.mean_info() == (False, False)
    h.set_output_warp(np.array([[1.0, 0.5, 0.1]]), 1.0)
    assert h.lib.gp_mean_set(h.h, _lib.dptr(p.A), _lib.dptr(p.b)) == _lib.GP_ERR_STATE  # refused while a warp is on
    assert b"warp" in h.lib.gp_last_error()
    h.set_output_warp(None)
    h.mean_set(p.A, p.b)
    h.fit()
    assert h.lib.gp_mean_grad(h.h, None, None) == 0                                     # either output may be NULL
    h.close()


def test_refused_entries_name_the_mean_function_and_leave_the_context_usable():
    h, p = handle("d")
    lml = h.fit()[0]
    x = MT.points("d")
    h.set_candidates(x)
    mu = h.predict(True)[0]
    nls = 1
    one, ls1 = np.array([1.0]), np.array([[0.5]])
    h.Mz, h.sparse_M = 8, 8        # (what the refused sparse_set_inducing / sparse_set_candidates would have recorded on the wrapper)
    calls = [
        lambda: h.set_output_warp(np.array([[1.0, 0.5, 0.1]]), 1.0), lambda: h.warp_grad(1),
        lambda: h.fit_grad_warp(np.array([[1.0, 0.5, 0.1]]), 1.0, nls), lambda: h.predict_warped(),
        lambda: h.sparse_set_inducing(p.X[:8]), lambda: h.sparse_fit(), lambda: h.sparse_fit_grad(nls),
        lambda: h.sparse_fit_grad_batch(p.X[None, :8], one, ls1, one), lambda: h.sparse_posterior(),
        lambda: h.sparse_predict(x), lambda: h.sparse_fmin(), lambda: h.sparse_set_candidates(x),
        lambda: h.sparse_acq(_lib.GP_ACQ_EI, 0.01, 0.0), lambda: h.sparse_acq_argbest(_lib.GP_ACQ_EI, 0.01, 0.0, -1),
        lambda: h.sparse_acq_topk(_lib.GP_ACQ_EI, 0.01, 0.0, -1, 2), lambda: h.sparse_predict_rows(x[:2]),
        lambda: h.sparse_acq_rows(x[:2], _lib.GP_ACQ_EI, 0.01, 0.0),
        lambda: h.ens_fit(one, ls1, one), lambda: h.ens_predict_rows(x[:2]), lambda: h.ens_acq_rows(x[:2], _lib.GP_ACQ_EI, 0.01),
        lambda: h.ens_acq(_lib.GP_ACQ_EI, 0.01), lambda: h.ens_acq_argbest(_lib.GP_ACQ_EI, 0.01, -1),
        lambda: h.es_set_representers(x[:4]), lambda: h.es_pmin(np.zeros(4), np.eye(4)),
        lambda: h.es_set_belief(np.zeros(4), np.zeros((4, 1)), np.zeros((4, 4)), np.zeros((4, 4, 4)), np.zeros((4, 2))),
        lambda: h.es_acq(), lambda: h.es_acq_rows(x[:2]), lambda: h.es_acq_argbest(-1),
        lambda: h.append(x[:1], np.vstack([p.Y, [[0.0]]])),
        lambda: h.fit_grad_batch(one, ls1, one), lambda: h.fit_grad_x_batch(p.X[None], one, ls1, one),
        lambda: h.fit_grad_warp_batch(np.array([[[1.0, 0.5, 0.1]]]), one, one, ls1, one),
        lambda: h.lml_grad_x(), lambda: h.fit_grad_x(nls),
        lambda: h.set_candidates_kumar(x, np.ones(3, dtype=np.int32), np.ones(3), np.ones(3), np.zeros(3), np.ones(3)),
        lambda: h.comm_allgather_best(0.0, 0, 1), lambda: h.comm_allgather_topk(np.zeros(1), np.zeros(1, dtype=np.int64), 1),
        lambda: h.comm_bcast_fit(0),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "mean function" in str(e.value) and "(%d)" % _lib.GP_ERR_STATE in str(e.value), (k, str(e.value))
    assert h.fit()[0] == lml
    h.set_candidates(x)
    assert np.array_equal(h.predict(True)[0], mu)
    h.close()


def test_group_entries_refuse_a_member_with_a_mean():
    p, x = MT.problem("d"), MT.points("d")
    grp = _lib.Group([0])
    try:
        grp.set_data(p.X, p.Y)
        grp.set_params(FS.KERNEL_ID[p.case.fam], int(p.case.ard), MT.VAR, p.ls, MT.NOISE)
        grp.fit()
        member = ctypes.c_void_p()
        assert grp.lib.gp_group_member(grp.h, 0, ctypes.byref(member)) == 0
        assert grp.lib.gp_mean_set(member, _lib.dptr(p.A), _lib.dptr(p.b)) == 0
        for call in (lambda: grp.fit(), lambda: grp.fmin(), lambda: grp.set_data(p.X, p.Y), lambda: grp.set_candidates(x[:4]),
                     lambda: grp.acq_argbest(_lib.GP_ACQ_EI, 0.01, 0.0, -1)):
            with pytest.raises(RuntimeError, match=r"\(-3\).*mean function"):
                call()
        assert grp.lib.gp_mean_set(member, None, None) == 0
        grp.fit()
    finally:
        grp.close()


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def _planted(N=40, seed=4):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, 2))
    Y = (3.0 * X[:, :1] - 2.0 * X[:, 1:] + 1.0) + 0.3 * np.exp(-((X - 0.5) ** 2).sum(1, keepdims=True) / 0.02) + 0.02 * rng.standard_normal((N, 1))
    return X, Y


def _mean_model(X, Y, seed=11):
    np.random.seed(seed)
    mean = gpo.mappings.Additive(gpo.mappings.Linear(2, 1), gpo.mappings.Constant(2, 1, 0.0))
    return gpo.models.GPRegression(X, Y, gpo.kern.RBF(2, 1.0, 0.2), noise_var=1e-2, mean_function=mean)


def test_checkgrad_with_additive_linear_constant():
    X, Y = _planted()
    m = _mean_model(X, Y)
    np.random.seed(0)
    assert m.checkgrad()
    assert m.checkgrad(verbose=True)
    m.close()


def test_optimize_beats_the_zero_mean_model_and_extrapolates_along_the_trend():
    X, Y = _planted()
    m = _mean_model(X, Y)
    z = gpo.models.GPRegression(X, Y, gpo.kern.RBF(2, 1.0, 0.2), noise_var=1e-2)
    for mod in (m, z):
        mod.optimize(max_iters=200)
    print("MODEL lml with mean %.6f  zero-mean %.6f" % (m.log_likelihood(), z.log_likelihood()))
    assert m.log_likelihood() > z.log_likelihood()
    # three lengthscales outside the data, the posterior is the trend (k* ~ variance exp(-9 / 2) of its weight in the box at
    # most); the zero-mean model has fallen back towards 0 there
    ls = float(m.kern.lengthscale.values[0])
    x = np.array([[1.0 + 3.0 * ls, 0.5]])
    A, b = gpo.mappings.affine_parts(m.mean_function)
    trend = (x @ A + b).item()
    hyper = (float(m.kern.variance), m.kern.lengthscale.values.copy(), float(m.likelihood.variance))
    gp, gp64 = (MT.MeanGP("rbf", False, *hyper, X, Y, A, b, lin) for lin in (MT.LD, MT.F64))
    mu_t, mu_64 = gp.at(x)[0][0, 0], gp64.at(x)[0][0, 0]
    mu = float(m.predict_noiseless(x)[0][0, 0])
    print("MODEL outside: device %.12f truth %.12f trend %.6f zero-mean %.6f" % (mu, float(mu_t), trend, float(z.predict(x)[0][0, 0])))
    ok, what = truth("model: mean 3 lengthscales outside", mu, mu_64, mu_t, 40)
    assert ok, what
    zls = float(z.kern.lengthscale.values[0])
    far = np.array([[1.0 + 6.0 * max(ls, zls), 0.5]])
    far_trend = (far @ A + b).item()
    assert abs(float(z.predict(far)[0][0, 0])) < 0.05 * abs(far_trend) and abs(float(m.predict(far)[0][0, 0]) - far_trend) < 1e-3
    dm, _ = m.predictive_gradients(far)
    assert np.max(np.abs(dm[0, :, 0] - A[:, 0])) < 1e-3          # the stated deviation: the gradients include A
    m.close()
    z.close()


def test_bayesian_optimization_with_a_mean_function_takes_the_device_routes():
    X, Y = _planted(12)
    np.random.seed(5)
    mean = gpo.mappings.Additive(gpo.mappings.Linear(2, 1), gpo.mappings.Constant(2, 1, 0.0))
    domain = [{"name": "x0", "type": "continuous", "domain": (0.0, 1.0)}, {"name": "x1", "type": "continuous", "domain": (0.0, 1.0)}]
    bo = gpo.methods.BayesianOptimization(f=None, domain=domain, X=X, Y=Y, acquisition_type="EI", mean_function=mean, max_iters=20,
                                          optimize_restarts=1)
    x = np.atleast_2d(bo.suggest_next_locations())
    assert x.shape == (1, 2) and np.all(x >= 0.0) and np.all(x <= 1.0)
    gp = bo.model.model
    assert gp.mean_function is mean and gp._h.mean_info() == (True, True)
    stats = gp._h.rows_stats()
    print("BO rows stats", stats)
    assert stats["fused"] >= 1
