"""GPU: max-value entropy search -- the rule GP_ACQ_MES through every scoring entry of the exact model, the samples behind it
(gp_mes_set / gp_mes_info), the sampler's reductions (gp_mes_logsurv, gp_mes_bracket; csrc/mes.hip, csrc/api_mes.hip) and the
classes on top (max_value.MinValueSampler, AcquisitionMES, BayesianOptimization(acquisition_type='MES')).

The truth is tests/_mes_truth.py (long double).  Two kinds of comparison:
* rule arithmetic: the truth fed with the handle's OWN gp_predict / gp_predict_grad outputs, held to the rounding-error bound the
  truth derives operation by operation;
* end to end: the truth fed with the CPU oracle's posterior, held to that bound plus the posterior tolerance of
  tests/test_gpu_rows.py (mean 1e-6 max(1, |m|), sd 1e-6 sd + 1e-12, dmdx 1e-6 max(|dmdx|_max, 1e-3), dvdx 1e-6 variance)
  propagated through the rule per case and location (_mes_truth.propagate).
Every figure is printed before it is asserted (tools/mes_errors.py collects them into profiles/mes_errors.txt).
"""
import collections
import ctypes
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import bayesian_optimization as bo
from gaussian_process_optimization_amd import max_value
from gaussian_process_optimization_amd.acquisitions import _RULES
from oracle import cpu_ref as O

import _mes_truth as MT
import _kernel_families as KF

pytestmark = pytest.mark.gpu

T, U = MT.T, 2.0 ** -53
MES = _lib.GP_ACQ_MES
YM, YS = MT.Y_MEAN, MT.Y_STD
KID = {"Mat52": _lib.GP_KERNEL_MATERN52, "Exponential": _lib.GP_KERNEL_EXPONENTIAL}
CASE_IDS = [c.id for c in MT.TABLE]


def _handle(p):
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(p.X, p.Y)
    h.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, MT.NOISE)
    h.fit()
    return h


Setup = collections.namedtuple("Setup", "p h gp post dev latent_tab")


@functools.lru_cache(maxsize=None)
def setup(cid):
    """The handle of a case, its oracle, the oracle's posterior (noise included, with gradients) and the handle's own at the nine
    rows, and the oracle's LATENT posterior over the table: computed once, shared, read-only."""
    p = MT.problem(cid)
    h = _handle(p)
    gp = O.OracleGP(p.X, p.Y, KF.make(p.case.fam, p.case.D, p.variance, p.ls_arg, p.case.ard, direct=True), MT.NOISE)
    m, v = gp.predict(p.Xs)
    dm, dv = gp.predictive_gradients(p.Xs)
    post = (m[:, 0], v[:, 0], dm[:, :, 0], dv)
    h.set_candidates(p.Xs)
    mean, var = h.predict(True)
    gm, gv = h.predict_grad()
    dev = (mean[:, 0].copy(), var[:, 0].copy(), gm[:, :, 0].copy(), gv.copy())
    lm, lv = gp.predict(p.Xtab, include_likelihood=False)
    latent = (lm[:, 0], lv[:, 0])
    for a in post + dev + latent:
        a.setflags(write=False)
    return Setup(p, h, gp, post, dev, latent)


def _unnormalised(mean, var):
    return mean * YS + YM, np.sqrt(np.maximum(var * (YS * YS), 1e-10))


def _ystar(s, target):
    return MT.ystar_for(s.p.case.id, target, *_unnormalised(*s.dev[:2]))


def _posterior_tolerance(s, post):
    mean, var, dm, dv = post
    sd = np.sqrt(np.maximum(var, 0.0))
    return (1e-6 * np.maximum(1.0, np.abs(mean)), 1e-6 * sd + 1e-12,
            np.full(dm.shape, 1e-6 * max(np.abs(dm).max(), 1e-3)), np.full(dv.shape, 1e-6 * s.p.variance))


def _ratio(err, bound):
    return float(np.max(np.asarray(err, dtype=T) / np.asarray(bound, dtype=T)))


def _table(s, X):
    s.h.set_candidates(X)
    return s.h


# ---- 1. rule arithmetic, 2. end to end -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", MT.G_TARGETS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_table_scores_against_the_truth(cid, target):
    s = setup(cid)
    p = s.p
    ystar = _ystar(s, target)
    h = _table(s, p.Xs)
    h.mes_set(ystar)
    assert h.mes_info() == p.case.K
    a = h.acq(MES, 0.0, 0.0, YM, YS)
    a2, da = h.acq_grad(MES, 123.0, -7.0, YM, YS)            # par and fmin are ignored
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(da))
    assert np.array_equal(a, a2)
    f = MT.score(*s.dev, ystar, YM, YS)
    r1 = _ratio(np.abs(a[:, 0] + f.alpha), f.bound_alpha)
    r2 = _ratio(np.abs(da + f.dalpha), f.bound_dalpha)
    g = MT.score(*s.post, ystar, YM, YS)
    tl, td = MT.propagate(g, YS, *_posterior_tolerance(s, s.post))
    r3 = _ratio(np.abs(a[:, 0] + g.alpha), tl + g.bound_alpha)
    r4 = _ratio(np.abs(da + g.dalpha), td + g.bound_dalpha)
    print("MES table case %s g*=%+.0f g[0,0]=%+.3f alpha[0]=%.6e | rule: value %.3f gradient %.3f of the bound | "
          "oracle: value %.3g gradient %.3g of the tolerance" % (cid, target, float(f.g[0, 0]), -a[0, 0], r1, r2, r3, r4))
    assert abs(float(f.g[0, 0]) - target) <= 1e-9 * max(1.0, abs(target))
    assert max(r1, r2, r3, r4) <= 1.0


# ---- 3. rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_rows_routes_bits_and_the_table(cid):
    s = setup(cid)
    p, h = s.p, s.h
    ystar = _ystar(s, 0.0)
    h.mes_set(ystar)
    h.set_candidates(p.Xs)
    tab, dtab = h.acq_grad(MES, 0.0, 0.0, YM, YS)
    alone = [h.acq_rows(p.Xs[i:i + 1], MES, 0.0, 0.0, YM, YS, grad=True) for i in range(MT.M_ROWS)]
    alone_v = [h.acq_rows(p.Xs[i:i + 1], MES, 0.0, 0.0, YM, YS) for i in range(MT.M_ROWS)]
    worst = 0.0
    for M, kind in ((1, "narrow"), (3, "narrow"), (4, "narrow"), (5, "wide"), (8, "wide"), (9, "fallback")):
        for grad in (False, True):
            before = dict(h.rows_pass_stats(), **h.rows_stats())
            out = h.acq_rows(p.Xs[:M], MES, 0.0, 0.0, YM, YS, grad=grad)
            after = dict(h.rows_pass_stats(), **h.rows_stats())
            assert tuple(after[k] - before[k] for k in ("narrow", "wide", "fallback")) == {"narrow": (1, 0, 0), "wide": (0, 1, 0), "fallback": (0, 0, 1)}[kind], (M, kind)
            v, dv = out if grad else (out, None)
            if kind != "fallback":
                # a location's results: the same bits alone, in any slot and in either kind of pass
                for i in range(M):
                    ref = alone[i] if grad else (alone_v[i], None)
                    assert v[i, 0] == ref[0][0, 0], (M, i)
                    if grad:
                        assert np.array_equal(dv[i], ref[1][0]), (M, i)
                rev = h.acq_rows(p.Xs[:M][::-1].copy(), MES, 0.0, 0.0, YM, YS, grad=grad)
                rv = rev[0] if grad else rev
                assert np.array_equal(rv[::-1], v)
            else:
                assert np.array_equal(v, tab[:M]) and (not grad or np.array_equal(dv, dtab[:M]))     # the table entries themselves
            # fused against table route: the tolerance tests/test_gpu_rows.py holds the two routes to
            worst = max(worst, np.max(np.abs(v - tab[:M])) / (1e-8 * np.max(np.abs(tab[:M]))))
            if grad:
                worst = max(worst, np.max(np.abs(dv - dtab[:M])) / (1e-7 * np.max(np.abs(dtab[:M]))))
    print("MES rows case %s: fused against table, worst %.3g of the routes' tolerance" % (cid, worst))
    assert worst <= 1.0


def test_rows_with_a_mean_function_and_the_penaliser():
    """The MES instances of the finishing kernel that also carry the mean function, and the penaliser behind the rule: against the
    table entries within the routes' tolerance."""
    s = setup("b")
    p = s.p
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(p.X, p.Y)
    h.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, MT.NOISE)
    h.mean_set(np.linspace(0.2, -0.3, p.case.D)[:, None], np.array([0.1]))
    h.fit()
    h.mes_set(_ystar(s, 0.0))
    Xb, r0, s0 = p.Xs[:2] + 0.01, np.array([0.05, 0.2]), np.array([0.03, 0.1])
    h.set_candidates(p.Xs[:5])
    tab, dtab = h.acq_grad(MES, 0.0, 0.0, YM, YS)
    lpt, dlpt = h.acq_lp_grad(MES, 0.0, 0.0, 0, Xb, r0, s0, YM, YS)
    for M in (1, 4, 5):
        v, dv = h.acq_rows(p.Xs[:M], MES, 0.0, 0.0, YM, YS, grad=True)
        assert np.max(np.abs(v - tab[:M])) <= 1e-8 * np.max(np.abs(tab)) and np.max(np.abs(dv - dtab[:M])) <= 1e-7 * np.max(np.abs(dtab))
        lv, dlv = h.acq_rows(p.Xs[:M], MES, 0.0, 0.0, YM, YS, grad=True, lp=(0, Xb, r0, s0))
        assert np.max(np.abs(lv - lpt[:M])) <= 1e-8 * np.max(np.abs(lpt)) and np.max(np.abs(dlv - dlpt[:M])) <= 1e-7 * np.max(np.abs(dlpt))
    h.close()


# ---- 4. selection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["b", "c"])
def test_selection_is_numpy_over_the_scores(cid):
    s = setup(cid)
    p, h = s.p, s.h
    h.mes_set(_ystar(s, 3.0))
    X = np.vstack([p.Xtab[:300], p.Xtab[:40], p.Xtab[100:103]])          # duplicated rows: ties resolve to the lowest index
    h.set_candidates(X)
    v = h.acq(MES, 0.0, 0.0, YM, YS)[:, 0]
    assert np.array_equal(v[300:340], v[:40])
    for sense in (-1, 1):
        i, val = h.acq_argbest(MES, 0.0, 0.0, sense, YM, YS)
        want = int(np.argmin(v) if sense < 0 else np.argmax(v))
        assert i == want and val == v[want]
        idx, vals = h.acq_topk(MES, 0.0, 0.0, sense, 7, YM, YS)
        order = np.argsort(v if sense < 0 else -v, kind="stable")[:7]
        assert list(idx) == list(order) and np.array_equal(np.asarray(vals), v[order])
    dup = np.vstack([p.Xtab[5:6]] * 6)
    h.set_candidates(dup)
    assert h.acq_argbest(MES, 0.0, 0.0, -1, YM, YS)[0] == 0
    assert list(h.acq_topk(MES, 0.0, 0.0, -1, 3, YM, YS)[0]) == [0, 1, 2]


def _lp_truth(neg, dneg, X, Xb, r0, s0):
    """lp_value / lp_value_grad (csrc/acq_math.h, transform 'none') in long double on the given base scores, with the rounding
    bound of the device's evaluation: log within 8 u, the penaliser's z = (|x - xb| - r) / s good to dz = u ((D + 6) |x - xb| + 2
    |z| s) / s, log Phi(z) moving by lambda dz and evaluated within ev (tests/_mes_truth._ev); the gradient's scale 1 / a within 2 u
    and each penaliser term phi / (s Phi |x - xb|) within (48 + 2 z^2) u + (|z| + lambda) dz relative; one u per addition."""
    a = -np.asarray(neg, dtype=np.float64).astype(T)
    D, nb = X.shape[1], Xb.shape[0]
    val = -np.log(a + T(1e-50))
    bound = 9 * U * np.abs(val) + 2 * U
    gap = X.astype(T)[:, None, :] - Xb.astype(T)[None, :, :]
    nm = np.sqrt((gap * gap).sum(-1))
    z = (nm - r0.astype(T)) / s0.astype(T)
    t = MT.log_ndtr(z)
    lam = np.exp(-z * z / 2 - MT.HALF_LOG_2PI - t)
    dz = U * ((D + 6) * nm + 2 * np.abs(z) * s0.astype(T)) / s0.astype(T)
    val = val - t.sum(1)
    bound = bound + (lam * dz + MT._ev(z, t, lam)).sum(1) + (nb + 1) * U * (np.abs(val) + np.abs(t).sum(1))
    term = lam / (s0.astype(T) * nm)
    pen = term.sum(1)
    grad = (1 / a)[:, None] * np.asarray(dneg, dtype=np.float64).astype(T) - pen[:, None]
    dterm = term * ((48 + 2 * z * z) * U + (np.abs(z) + lam) * dz)
    gbound = (np.abs((1 / a)[:, None] * dneg) * 4 * U + dterm.sum(1)[:, None] + (nb + 2) * U * (np.abs(grad) + pen[:, None]))
    return val, grad, bound * (1 + T(1e-3)), gbound * (1 + T(1e-3))


@pytest.mark.parametrize("cid", ["b", "f"])
def test_penalised_and_per_cost_scores_are_the_documented_maps_of_the_base(cid):
    s = setup(cid)
    p, h = s.p, s.h
    h.mes_set(_ystar(s, 0.0))
    X = p.Xtab[:257]
    h.set_candidates(X)
    base, dbase = h.acq_grad(MES, 0.0, 0.0, YM, YS)
    Xb, r0, s0 = X[:2] + 0.01, np.array([0.05, 0.2]), np.array([0.03, 0.1])
    lp = h.acq_lp(MES, 0.0, 0.0, 0, Xb, r0, s0, YM, YS)
    lp2, dlp = h.acq_lp_grad(MES, 0.0, 0.0, 0, Xb, r0, s0, YM, YS)
    assert np.array_equal(lp, lp2)
    val, grad, bv, bg = _lp_truth(base[:, 0], dbase, X, Xb, r0, s0)
    r1, r2 = _ratio(np.abs(lp - val), bv), _ratio(np.abs(dlp - grad), bg)
    excl = [int(np.argmin(lp)), 3]
    j, lval = h.acq_lp_argbest(MES, 0.0, 0.0, 0, -1, Xb, r0, s0, exclude=excl, y_mean=YM, y_std=YS)
    masked = np.where(np.isin(np.arange(lp.size), excl), np.inf, lp)
    assert j == int(np.argmin(masked)) and lval == masked[j]
    # GP_ACQ_PER_COST: neg <- neg / c, dneg <- (dneg - neg dlogc) / c with c = exp(logc) of gp_cost_rows (include/gphip.h)
    rng = np.random.default_rng(5)
    Xc = rng.uniform(0, 1, (40, p.case.D))
    h.cost_set(Xc, 0.3 * rng.standard_normal(40), KID[p.case.fam], int(p.case.ard), 0.8, p.ls_arg, 0.1, 0.7)
    try:
        logc, dlogc = h.cost_rows(X, grad=True)
        per = h.acq(MES | _lib.GP_ACQ_PER_COST, 0.0, 0.0, YM, YS)
        per2, dper = h.acq_grad(MES | _lib.GP_ACQ_PER_COST, 0.0, 0.0, YM, YS)
        h.set_candidates(X)
        assert np.array_equal(h.acq(MES, 0.0, 0.0, YM, YS), base)           # the flag leaves the unflagged scores alone
        c = np.exp(logc.astype(T))
        want, dwant = base[:, 0].astype(T) / c, (dbase.astype(T) - base.astype(T) * dlogc.astype(T)) / c[:, None]
        # exp within 8 u carrying |logc| u of its argument, a division; the gradient: a product, a difference, a division
        r3 = max(_ratio(np.abs(per[:, 0] - want), (10 + np.abs(logc)) * U * np.abs(want) + 1e-300),
                 _ratio(np.abs(per2[:, 0] - want), (10 + np.abs(logc)) * U * np.abs(want) + 1e-300))
        mag = (np.abs(dbase) + np.abs(base * dlogc)) / c[:, None]
        r4 = _ratio(np.abs(dper - dwant), ((12 + np.abs(logc)) * U)[:, None] * mag + 1e-300)
        rows = h.acq_rows(X[:5], MES | _lib.GP_ACQ_PER_COST, 0.0, 0.0, YM, YS)
        assert np.max(np.abs(rows - per[:5])) <= 1e-8 * np.max(np.abs(per[:5]))
    finally:
        h.cost_set(None, None, 0, 0, 1.0, None)
    print("MES maps case %s: penalised value %.3f gradient %.3f, per-cost value %.3f gradient %.3f of the bound" % (cid, r1, r2, r3, r4))
    assert max(r1, r2, r3, r4) <= 1.0


# ---- 5. the sampler's reductions, 6. the cache ---------------------------------------------------------------------------------------
LOGSURV_M = (1, 63, 64, 65, 255, 256, 257, 1000)            # MES_CHUNK = 256: one either side of it, and several chunks


@pytest.mark.parametrize("cid", ["a", "e"])
def test_logsurv_against_the_truth_and_its_bits(cid):
    s = setup(cid)
    p, h = s.p, s.h
    worst = 0.0
    for M in LOGSURV_M:
        h.set_candidates(p.Xtab[:M])
        for noise in (False, True):
            mean, var = h.predict(noise)
            m, sd = _unnormalised(mean[:, 0], var[:, 0])
            lo, hi = h.mes_bracket(8.0, include_noise=noise, y_mean=YM, y_std=YS)
            assert lo == np.min(m - 8.0 * sd) and hi == np.min(m + 8.0 * sd)          # NumPy on gp_predict's output, bit for bit
            y64 = np.linspace(lo, hi, 66)[1:-1]
            o64 = h.mes_logsurv(y64, include_noise=noise, y_mean=YM, y_std=YS)
            assert np.array_equal(o64, h.mes_logsurv(y64, include_noise=noise, y_mean=YM, y_std=YS))       # two calls
            for G in (1, 7):
                pick = np.random.default_rng(G + M).permutation(64)[:G]
                assert np.array_equal(h.mes_logsurv(y64[pick], include_noise=noise, y_mean=YM, y_std=YS), o64[pick])   # any G, any place
            t = MT.logsurv(mean[:, 0], var[:, 0], YM, YS, y64)
            worst = max(worst, _ratio(np.abs(o64 - t.value), t.bound))
            ends = h.mes_logsurv([lo, hi], include_noise=noise, y_mean=YM, y_std=YS)
            assert ends[0] > -1e-12 and ends[1] < np.log(1e-15)          # S rounds to 1 at the lower end, is below 1e-15 at the upper
    print("MES logsurv case %s: worst error %.3f of the bound over M = %s" % (cid, worst, LOGSURV_M))
    assert worst <= 1.0


def test_a_latent_logsurv_leaves_the_noisy_cache_alone():
    s = setup("d")
    p, h = s.p, s.h
    h.mes_set(_ystar(s, 0.0))
    h.set_candidates(p.Xtab[:300])
    fmin = h.fmin()
    ei = h.acq(_lib.GP_ACQ_EI, 0.01, fmin, YM, YS)
    mes = h.acq(MES, 0.0, 0.0, YM, YS)
    mean, var = h.predict(True)
    lat = h.predict(False)[1]
    assert np.all(lat < var)
    for call in (lambda: h.mes_logsurv([0.0], include_noise=False, y_mean=YM, y_std=YS),
                 lambda: h.mes_bracket(8.0, include_noise=False, y_mean=YM, y_std=YS)):
        h.acq(_lib.GP_ACQ_EI, 0.01, fmin, YM, YS)          # the cache holds the noisy posterior
        call()                                             # ... now the latent one
        assert np.array_equal(h.acq(_lib.GP_ACQ_EI, 0.01, fmin, YM, YS), ei)
        call()
        assert np.array_equal(h.acq(MES, 0.0, 0.0, YM, YS), mes)
        call()
        i, v = h.acq_argbest(_lib.GP_ACQ_EI, 0.01, fmin, -1, YM, YS)
        assert i == int(np.argmin(ei[:, 0])) and v == ei[i, 0]
        call()
        m2, v2 = h.predict(True)
        assert np.array_equal(m2, mean) and np.array_equal(v2, var)


# ---- 7. the sampler ------------------------------------------------------------------------------------------------------------------
def _gpmodel(p):
    """A GPModel at the case's fixed hyper-parameters."""
    kern = {"Mat52": gpo.kern.Matern52, "Exponential": gpo.kern.Exponential}[p.case.fam](p.case.D, p.variance, p.ls_arg, ARD=p.case.ard)
    gm = gpo.GPModel(kernel=kern, noise_var=MT.NOISE, max_iters=0, verbose=False)
    gm.updateModel(p.X, p.Y, None, None)
    return gm


class _TableSpace(object):
    """A design space whose uniform draws are the head of the case's table."""

    def __init__(self, p, n):
        self.p, self.n = p, n

    def samples_uniform(self, n):
        assert n == self.n
        return self.p.Xtab[:n]

    def get_bounds(self):
        return [(0.0, 1.0)] * self.p.case.D

    def has_constraints(self):
        return False

    def indicator_constraints(self, x):
        return np.ones((np.atleast_2d(x).shape[0], 1))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_sampler_brackets_hold_the_truths_quantiles(cid):
    s = setup(cid)
    p = s.p
    gm = _gpmodel(p)
    n = 400
    smp = max_value.MinValueSampler(gm, _TableSpace(p, n), num_samples=p.case.K, grid_size=n, seed=11)
    ystar = smp.sample()
    assert smp.last_on_device
    fmin = gm.get_fmin()
    assert ystar.shape == (p.case.K,) and np.all(ystar <= fmin)
    table = np.vstack([p.Xtab[:n], p.X])
    lm, lv = s.gp.predict(table, include_likelihood=False)
    lm, lv = lm[:, 0], np.maximum(lv[:, 0], 0.0)
    d_mean, d_sd = 1e-6 * np.maximum(1.0, np.abs(lm)), 1e-6 * np.sqrt(lv) + 1e-12
    worst = 0.0
    for q in MT.QUANTILES:
        lo, hi = smp.last_brackets[q]
        yq = MT.quantile(lm, lv, 0.0, 1.0, q)
        t = MT.logsurv(lm, lv, 0.0, 1.0, [float(yq)])
        tol = MT.propagate_logsurv(lm, lv, 0.0, 1.0, [float(yq)], d_mean, d_sd)
        widen = float((t.bound[0] + tol[0]) / abs(t.slope[0]))
        assert hi - lo <= max_value.REL_WIDTH * (smp.last_first[1] - smp.last_first[0])
        miss = max(lo - widen - float(yq), float(yq) - hi - widen)
        worst = max(worst, miss / widen + 1.0)
        print("MES sampler case %s q=%.2f: bracket [%.12g, %.12g], truth %.12g, widening %.3g, outside by %.3g"
              % (cid, q, lo, hi, float(yq), widen, max(miss, 0.0)))
        assert miss <= 0.0
    quant = {q: 0.5 * sum(smp.last_brackets[q]) for q in MT.QUANTILES}
    a, b = MT.gumbel_fit(quant[0.25], quant[0.5], quant[0.75])
    assert np.array_equal(ystar, MT.gumbel_samples(a, b, p.case.K, 11, fmin))
    gm.model.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_handle_usable():
    s = setup("d")
    p, h = s.p, s.h
    lib, ARG, STATE = h.lib, _lib.GP_ERR_ARG, _lib.GP_ERR_STATE
    ystar = _ystar(s, 0.0)
    h.set_candidates(p.Xtab[:64])
    h.mes_set(ystar)
    ref = h.acq(MES, 0.0, 0.0, YM, YS)
    fmin = h.fmin()
    ei = h.acq(_lib.GP_ACQ_EI, 0.01, fmin, YM, YS)
    out, dout = np.empty((64, 1)), np.empty((64, p.case.D))
    idx, val = ctypes.c_int64(), ctypes.c_double()
    # no resident samples
    h.mes_set(None)
    assert h.mes_info() == 0
    assert lib.gp_acq(h.h, MES, 0.0, 0.0, YM, YS, _lib.dptr(out)) == STATE
    assert lib.gp_acq_grad(h.h, MES, 0.0, 0.0, YM, YS, _lib.dptr(out), _lib.dptr(dout)) == STATE
    assert lib.gp_acq_argbest(h.h, MES, 0.0, 0.0, YM, YS, -1, ctypes.byref(idx), ctypes.byref(val)) == STATE
    with pytest.raises(RuntimeError):
        h.acq_rows(p.Xs[:3], MES, 0.0, 0.0, YM, YS)
    with pytest.raises(RuntimeError):
        h.acq_lp(MES, 0.0, 0.0, 0, y_mean=YM, y_std=YS)
    # K = 65, a NaN sample, a null pointer with K > 0: the resident samples stay
    h.mes_set(ystar)
    big = np.zeros(_lib.GP_MES_MAX_K + 1)
    assert lib.gp_mes_set(h.h, _lib.dptr(big), big.size) == ARG
    assert lib.gp_mes_set(h.h, _lib.dptr(big), -1) == ARG
    assert lib.gp_mes_set(h.h, None, 3) == ARG
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError):
            h.mes_set(np.array([0.1, bad, 0.2]))
    assert h.mes_info() == p.case.K
    assert np.array_equal(h.acq(MES, 0.0, 0.0, YM, YS), ref)
    # GP_ACQ_TIMES_FEAS with the rule, on the entries that know the flag and on those that do not
    for t in (MES | _lib.GP_ACQ_TIMES_FEAS, MES | _lib.GP_ACQ_TIMES_FEAS | _lib.GP_ACQ_PER_COST):
        with pytest.raises(ValueError):
            h.acq(t, 0.0, 0.0, YM, YS)
        with pytest.raises(ValueError):
            h.acq_grad(t, 0.0, 0.0, YM, YS)
        with pytest.raises(ValueError):
            h.acq_rows(p.Xs[:3], t, 0.0, 0.0, YM, YS)
    with pytest.raises(ValueError):
        h.acq(MES | _lib.GP_ACQ_PER_COST, 0.0, 0.0, YM, YS)          # no cost surface
    # the sampler's entries: G out of range, a trial value that is not finite, a bad normaliser or nsig
    y = np.zeros(_lib.GP_MES_MAX_G + 1)
    o = np.empty(y.size)
    for G in (0, _lib.GP_MES_MAX_G + 1):
        assert lib.gp_mes_logsurv(h.h, 0, YM, YS, _lib.dptr(y), G, _lib.dptr(o)) == ARG
    with pytest.raises(ValueError):
        h.mes_logsurv([0.0, np.nan], y_mean=YM, y_std=YS)
    with pytest.raises(ValueError):
        h.mes_logsurv([0.0], y_mean=YM, y_std=0.0)
    with pytest.raises(ValueError):
        h.mes_bracket(-1.0, y_mean=YM, y_std=YS)
    with pytest.raises(ValueError):
        h.mes_bracket(np.nan, y_mean=YM, y_std=YS)
    # P = 2
    two = _lib.Handle(0)
    two.set_data(p.X, np.hstack([p.Y, -p.Y]))
    two.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, MT.NOISE)
    two.fit()
    two.set_candidates(p.Xtab[:64])
    two.mes_set(ystar)
    with pytest.raises(ValueError):
        two.acq(MES, 0.0, 0.0, YM, YS)
    with pytest.raises(ValueError):
        two.mes_logsurv([0.0], y_mean=YM, y_std=YS)
    with pytest.raises(ValueError):
        two.mes_bracket(8.0, y_mean=YM, y_std=YS)
    two.close()
    unfit = _lib.Handle(0)
    unfit.set_data(p.X, p.Y)
    unfit.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, MT.NOISE)
    unfit.mes_set(ystar)                                   # valid before a fit: the samples are the caller's numbers
    with pytest.raises(RuntimeError):
        unfit.mes_logsurv([0.0])
    unfit.close()
    # a refused call changed nothing, and the samples survive a refit and new data
    assert np.array_equal(h.acq(MES, 0.0, 0.0, YM, YS), ref)
    assert np.array_equal(h.acq(_lib.GP_ACQ_EI, 0.01, fmin, YM, YS), ei)
    h.set_data(p.X, p.Y)
    h.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, MT.NOISE)
    h.fit()
    h.set_candidates(p.Xtab[:64])
    assert h.mes_info() == p.case.K
    assert np.array_equal(h.acq(MES, 0.0, 0.0, YM, YS), ref)


def test_the_other_entries_refuse_the_rule():
    """gp_acq_rows_feas, the sparse, ensemble and group entries build specs that do not know GP_ACQ_MES: an unknown acquisition,
    and they score as before afterwards."""
    s = setup("d")
    p, h = s.p, s.h
    ystar = _ystar(s, 0.0)
    h.mes_set(ystar)
    con = _handle(p)
    pack = _lib.FeasPack([con], np.array([0.0]), np.array([0.0]), np.array([1.0]))
    with pytest.raises(ValueError):
        h.acq_rows_feas(pack, p.Xs[:3], MES, 0.0, 0.0, YM, YS)
    assert h.acq_rows_feas(pack, p.Xs[:3], _lib.GP_ACQ_EI, 0.01, h.fmin(), YM, YS).shape == (3, 1)
    con.mes_set(ystar)                                     # (a handle of its own for the sparse fit and the ensemble)
    con.sparse_set_inducing(p.X[:20])
    con.sparse_fit()
    con.sparse_set_candidates(p.Xtab[:64])
    with pytest.raises(ValueError):
        con.sparse_acq(MES, 0.0, 0.0, YM, YS)
    assert con.sparse_acq(_lib.GP_ACQ_LCB, 2.0, 0.0, YM, YS).shape == (64, 1)
    con.ens_fit(np.array([1.0, 1.3]), np.tile(p.ls_arg, (2, 1)), np.array([1e-2, 2e-2]))
    con.set_candidates(p.Xtab[:64])
    with pytest.raises(ValueError):
        con.ens_acq(MES, 0.0)
    assert con.ens_acq(_lib.GP_ACQ_LCB, 2.0).shape == (64, 1)
    con.close()


def test_the_replica_group_refuses_the_rule():
    s = setup("d")
    p = s.p
    grp = _lib.Group([0])
    grp.set_data(p.X, p.Y)
    grp.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, MT.NOISE)
    grp.fit()
    grp.set_candidates(p.Xtab[:64])
    for call in (lambda: grp.acq_argbest(MES, 0.0, 0.0, -1, YM, YS), lambda: grp.acq_lp_argbest(MES, 0.0, 0.0, 0, -1, y_mean=YM, y_std=YS),
                 lambda: grp.acq_topk(MES, 0.0, 0.0, -1, 3, YM, YS)):
        with pytest.raises(ValueError):
            call()
    assert 0 <= grp.acq_argbest(_lib.GP_ACQ_LCB, 2.0, 0.0, -1, YM, YS)[0] < 64
    grp.close()


# ---- 9. the classes ------------------------------------------------------------------------------------------------------------------
def test_acquisition_mes_is_the_host_rule_over_the_oracle():
    s = setup("b")
    p = s.p
    gm = _gpmodel(p)
    space = _TableSpace(p, 300)
    acq = gpo.AcquisitionMES(gm, space, num_samples=10, grid_size=300, seed=3)
    assert acq._device_ok() and acq.analytical_gradient_acq
    rule = _RULES["MES"]
    om = O.OracleGPModel(s.gp)
    for X in (p.Xs[:1], p.Xs[:5], p.Xtab[:40]):
        v, dv = acq.acquisition_function_withGradients(X)
        v0 = acq.acquisition_function(X)
        ystar = acq.ystar
        assert acq.draws == 1 and gm.model._h.mes_info() == 10 and np.all(ystar <= gm.get_fmin())
        mu, sd, dmu, dsd = om.predict_withGradients(X)
        want, dwant = rule.gradient(ystar, 0.0, mu, sd, dmu, dsd)
        f = MT.score(mu[:, 0], sd[:, 0] ** 2, dmu, 2 * sd * dsd, ystar, 0.0, 1.0)
        post = (mu[:, 0], sd[:, 0] ** 2, dmu, 2 * sd * dsd)
        tl, td = MT.propagate(f, 1.0, *_posterior_tolerance(s, post))
        # the end-to-end tolerance (bound + propagated) against the long-double truth over the oracle's posterior
        r1 = _ratio(np.abs(v[:, 0] + f.alpha), tl + f.bound_alpha)
        r2 = _ratio(np.abs(dv + f.dalpha), td + f.bound_dalpha)
        # ... and the host rule in double over the same posterior within ITS rounding of that truth (the same bound: the same operations)
        r3 = max(_ratio(np.abs(want[:, 0] - f.alpha), f.bound_alpha), _ratio(np.abs(dwant - f.dalpha), f.bound_dalpha))
        print("MES class M=%d: value %.3g gradient %.3g of the end-to-end tolerance; host rule %.3g of the bound" % (X.shape[0], r1, r2, r3))
        assert max(r1, r2, r3) <= 1.0
        assert np.max(np.abs(v0 - v)) <= 1e-8 * np.max(np.abs(v))
    i, val = acq.argbest(p.Xtab[:40])
    v = acq.acquisition_function(p.Xtab[:40])[:, 0]
    assert i == int(np.argmin(v)) and val == v[i]
    idx, vals = acq.topk(p.Xtab[:40], 4)
    assert list(idx) == list(np.argsort(v, kind="stable")[:4])
    # new data: the samples are redrawn, once
    gm.updateModel(np.vstack([p.X, p.Xtab[500:501]]), np.vstack([p.Y, [[0.2]]]), None, None)
    acq.acquisition_function(p.Xs[:2])
    acq.acquisition_function(p.Xs[:2])
    assert acq.draws == 2
    gm.model.close()


def _quadratic(x):
    x = np.atleast_2d(x)
    return ((x - np.array([0.3, 0.6])) ** 2).sum(1)[:, None]


DOMAIN = [{'name': 'x%d' % d, 'type': 'continuous', 'domain': (0.0, 1.0)} for d in range(2)]


@pytest.mark.parametrize("config", ["sequential", "local_penalization", "parallel_anchors"])
def test_bayesian_optimization_runs_with_mes(config):
    kw = dict(acquisition_type='MES', num_min_samples=8, mes_grid_size=500, sampler_seed=5, max_iters=0, noise_var=1e-4,
              kernel='Matern52', initial_design_numdata=6)
    if config == "local_penalization":
        kw.update(evaluator_type='local_penalization', batch_size=3)
    if config == "parallel_anchors":
        kw.update(parallel_anchors=True)
    np.random.seed(4)
    opt = gpo.BayesianOptimization(_quadratic, DOMAIN, **kw)
    scored = opt.acquisition.acq if isinstance(opt.acquisition, gpo.AcquisitionLP) else opt.acquisition
    assert isinstance(scored, gpo.AcquisitionMES)
    n0 = opt.X.shape[0]
    opt.run_optimization(max_iter=3, verbosity=False)
    assert scored._device_ok() and scored.sampler.last_on_device
    new = opt.X[n0:]
    assert new.shape[0] >= 3 and np.all(new >= 0.0) and np.all(new <= 1.0)
    v = scored.acquisition_function(new)
    assert np.all(np.isfinite(v)) and np.all(v <= 0.0)
    assert scored.draws >= 3 and np.all(scored.ystar <= opt.model.get_fmin())


def test_lockstep_returns_the_serial_optimum_with_mes():
    X, Y, Xs = O.synthetic_problem(200, 3, 8, seed=31)
    gm = gpo.GPModel(kernel=gpo.kern.RBF(3, 1.1, O.default_lengthscale(3, False)), noise_var=1e-2, max_iters=0, verbose=False)
    gm.updateModel(X, Y, None, None)
    space = gpo.Design_space([{'name': 'x%d' % d, 'type': 'continuous', 'domain': (0.0, 1.0)} for d in range(3)])
    got = []
    for parallel in (False, True):
        acq = gpo.AcquisitionMES(gm, space, bo.AcquisitionOptimizer(space, parallel=parallel), num_samples=10, grid_size=500, seed=9)
        assert acq.analytical_gradient_acq
        np.random.seed(17)
        got.append(acq.optimize())
    (xs, fs), (xp, fp) = got
    assert xs.shape == (1, 3) and np.array_equal(xs, xp) and fs == fp
    gm.model.close()
