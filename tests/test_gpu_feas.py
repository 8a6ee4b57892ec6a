"""GPU: black-box constraints -- the probability of feasibility of K constraint GPs and the product it puts behind EI / MPI
(gp_feas_table, gp_feas_rows, gp_acq_rows_feas, gp_fmin_rows, GP_ACQ_TIMES_FEAS / GP_ACQ_POF; csrc/feas.hip, csrc/api_feas.hip).

The truth is tests/_feas_truth.py (long double).  Two kinds of comparison:
* fold arithmetic: the truth fed with the constraint handles' OWN gp_predict_rows outputs, held to the rounding-error bound the
  truth derives operation by operation;
* end to end: the truth fed with the CPU oracle's posterior, held to that bound plus the posterior tolerance of
  tests/test_gpu_rows.py (mean 1e-6 max(1, |m|), sd 1e-6 sd + 1e-12, dmdx 1e-6 max(|dmdx|_max, 1e-3), dvdx 1e-6 variance)
  propagated through lambda(z) (|dm| + |z| |ds|) / s per case and location (_feas_truth.propagate).
Every figure is printed before it is asserted (tools/feas_errors.py collects them into profiles/feas_errors.txt).
"""
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd.bayesian_optimization import InvalidConfigError
from oracle import cpu_ref as O

import _feas_truth as FT
import _kernel_families as KF

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FEAS = _lib.GP_ACQ_TIMES_FEAS
KID = {"Mat52": _lib.GP_KERNEL_MATERN52, "Exponential": _lib.GP_KERNEL_EXPONENTIAL}
CASE_IDS = [c.id for c in FT.TABLE]


def _handle(X, Y, p, noise):
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(X, Y)
    h.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, noise)
    h.fit()
    return h


def _oracle(X, Y, p, noise):
    return O.OracleGP(X, Y, KF.make(p.case.fam, p.case.D, p.variance, p.ls_arg, p.case.ard, direct=True), noise)


def _oracle_post(gp, Xs):
    """normalised mean, var (noise included) [M] and their gradients [M, D] of one oracle model"""
    m, v = gp.predict(Xs)
    dm, dv = gp.predictive_gradients(Xs)
    return m[:, 0], v[:, 0], dm[:, :, 0], dv


Setup = FT.collections.namedtuple("Setup", "p h cons gp ocons post post_tab")


@functools.lru_cache(maxsize=None)
def setup(cid):
    """The handles of a case (scored model and K constraint models), their oracles, and the oracle's posterior of the constraints
    at the rows' locations and at the table: computed once, shared, read-only."""
    p = FT.problem(cid)
    h = _handle(p.X, p.Y, p, 1e-2)
    cons = [_handle(p.Xc[k], p.C[k], p, p.noise[k]) for k in range(p.case.K)]
    gp = _oracle(p.X, p.Y, p, 1e-2)
    ocons = [_oracle(p.Xc[k], p.C[k], p, p.noise[k]) for k in range(p.case.K)]
    post = tuple(np.stack(a) for a in zip(*[_oracle_post(o, p.Xs) for o in ocons]))
    post_tab = tuple(np.stack(a) for a in zip(*[_oracle_post(o, p.Xtab) for o in ocons]))
    for a in post + post_tab:
        a.setflags(write=False)
    return Setup(p, h, cons, gp, ocons, post, post_tab)


def _bounds(s, target, post=None):
    mean, var = (post or s.post)[:2]
    m = mean * s.p.c_std[:, None] + s.p.c_mean[:, None]
    sd = np.sqrt(np.maximum(var * s.p.c_std[:, None] ** 2, 1e-10))
    return FT.bounds_for(s.p.case.id, target, m, sd)


def _pack(s, bounds):
    return _lib.FeasPack(s.cons, bounds, s.p.c_mean, s.p.c_std)


def _device_post(s, Xs, grad):
    """the constraint handles' own gp_predict_rows outputs, in the groups of eight gp_feas_rows makes"""
    out = []
    for h in s.cons:
        parts = [h.predict_rows(Xs[i:i + 8], include_noise=True, grad=grad) for i in range(0, Xs.shape[0], 8)]
        cols = [np.concatenate([q[j] for q in parts]) for j in range(4 if grad else 2)]
        out.append((cols[0][:, 0], cols[1][:, 0]) + ((cols[2][:, :, 0], cols[3]) if grad else ()))
    return tuple(np.stack(a) for a in zip(*out))


def _posterior_tolerance(s, post):
    mean, var, dm, dv = post
    sd = np.sqrt(np.maximum(var, 0.0))
    return (1e-6 * np.maximum(1.0, np.abs(mean)), 1e-6 * sd + 1e-12,
            np.broadcast_to(1e-6 * np.maximum(np.abs(dm).max(axis=(1, 2)), 1e-3)[:, None, None], dm.shape),
            np.full(dv.shape, 1e-6 * s.p.variance))


def _ratio(err, bound):
    return float(np.max(np.asarray(err, dtype=FT.T) / np.asarray(bound, dtype=FT.T)))


# ---- 1. fold arithmetic, 2. end to end -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", FT.Z_TARGETS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_feas_rows_against_the_truth(cid, target):
    s = setup(cid)
    p, Xs = s.p, s.p.Xs
    b = _bounds(s, target)
    pack = _pack(s, b)
    logF, dlogF = pack.rows(Xs, grad=True)
    logF_v = pack.rows(Xs)
    assert np.all(np.isfinite(logF)) and np.all(np.isfinite(dlogF)) and np.all(np.isfinite(logF_v))
    # fold arithmetic: the handles' own posterior in, the derived rounding bound
    f = FT.fold(*_device_post(s, Xs, True), p.c_mean, p.c_std, b)
    fv = FT.fold(*_device_post(s, Xs, False), None, None, p.c_mean, p.c_std, b)
    r1 = _ratio(np.abs(logF - f.logF), f.bound_logF)
    r2 = _ratio(np.abs(dlogF - f.dlogF), f.bound_dlogF)
    r3 = _ratio(np.abs(logF_v - fv.logF), fv.bound_logF)
    # end to end: the oracle's posterior in, the posterior tolerance propagated on top
    g = FT.fold(*s.post, p.c_mean, p.c_std, b)
    d_mean, d_sd, d_dm, d_dv = _posterior_tolerance(s, s.post)
    tl, td = FT.propagate(g, p.c_std, d_mean, d_sd, d_dm, d_dv, s.post[2], s.post[3])
    r4 = _ratio(np.abs(logF - g.logF), tl + g.bound_logF)
    r5 = _ratio(np.abs(dlogF - g.dlogF), td + g.bound_dlogF)
    zhit = float(f.z[0, 0])
    print("FEAS rows case %s z*=%+.0f z[0,0]=%+.3f logF[0]=%.6e | fold: logF %.3f dlogF %.3f values-only %.3f of the bound | "
          "oracle: logF %.3g dlogF %.3g of the tolerance" % (cid, target, zhit, logF[0], r1, r2, r3, r4, r5))
    assert abs(zhit - target) <= 0.5 + 0.02 * abs(target), zhit      # the placement did what the case is there for
    assert r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0
    assert r4 <= 1.0 and r5 <= 1.0
    if target == -45.0:
        assert np.isfinite(logF[0]) and logF[0] < -1000.0 and np.exp(logF[0]) == 0.0 and np.all(np.isfinite(dlogF[0]))
    if p.case.clip:
        assert float(f.s[0, 0]) == pytest.approx(1e-5, rel=1e-12)     # location 0 of constraint 0 took the variance clip


# ---- 3. tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_feas_table_against_rows_and_across_chunks(cid):
    s = setup(cid)
    p = s.p
    b = _bounds(s, -2.0, s.post_tab)
    pack = _pack(s, b)
    s.h.set_candidates(p.Xtab)
    assert s.h.feas_info() == (0, 0)
    s.h.feas_table(pack)
    assert s.h.feas_info() == (p.case.K, p.case.Mtab)
    tab = s.h.feas_get_table()
    rows = pack.rows(p.Xtab)
    # the rows-versus-table tolerance of tests/test_gpu_rows.py: 1e-9 on a well-conditioned model, 2e-6 at cond(Ky) ~ 1e8
    g = FT.fold(*s.post_tab, p.c_mean, p.c_std, b)
    rel = np.array([1e-9 if n >= 1e-4 else 2e-6 for n in p.noise])[:, None]
    mean, var = s.post_tab[:2]
    tl, _ = FT.propagate(g, p.c_std, rel * np.maximum(1.0, np.abs(mean)), rel * np.sqrt(var) + 1e-12)
    r = _ratio(np.abs(tab - rows), tl + 2 * g.bound_logF)
    print("FEAS table case %s M=%d: table against rows %.3g of the tolerance" % (cid, p.case.Mtab, r))
    assert r <= 1.0
    if p.case.Mtab > 256:
        for c in s.cons:
            c.set_option("mc_max", 128)
        try:
            s.h.feas_table(pack)
            assert np.array_equal(s.h.feas_get_table(), tab)      # three chunks: the same bits
        finally:
            for c in s.cons:
                c.set_option("mc_max", 16384)
    s.h.set_candidates(p.Xtab)
    assert s.h.feas_info() == (0, 0)                               # dropped with the table it belonged to


# ---- 4. scores, 5. selection -----------------------------------------------------------------------------------------------------
def _exp_tol(v, n):
    """n roundings (exp at 4 ulp = 8 u counted as 8) relative to v, and the spacing of the subnormals where F underflows"""
    return n * U * np.abs(v) + 1e-322


@pytest.mark.parametrize("cid", ["b", "c", "e"])
def test_flagged_scores_are_the_product(cid):
    s = setup(cid)
    p, h = s.p, s.h
    b = _bounds(s, 0.5, s.post_tab)
    h.set_candidates(p.Xtab)
    fmin = h.fmin()
    plain = {t: h.acq(t, 0.01, fmin).copy() for t in (_lib.GP_ACQ_EI, _lib.GP_ACQ_MPI)}
    Xb, r0, s0 = p.Xtab[:2] + 0.01, np.array([0.05, 0.2]), np.array([0.03, 0.1])
    lp_plain = {nb: h.acq_lp(_lib.GP_ACQ_EI, 0.01, fmin, 0, Xb[:nb] if nb else None, r0[:nb] if nb else None, s0[:nb] if nb else None)
                for nb in (0, 2)}
    h.feas_table(_pack(s, b))
    F = np.exp(h.feas_get_table())[:, None]
    worst = 0.0
    for t in plain:
        assert np.array_equal(h.acq(t, 0.01, fmin), plain[t])      # a resident cache changes nothing for an unflagged call
        fl = h.acq(t | FEAS, 0.01, fmin)
        worst = max(worst, _ratio(np.abs(fl - plain[t] * F), _exp_tol(plain[t] * F, 10)))
    pof = h.acq(_lib.GP_ACQ_POF | FEAS, 0.0, 0.0)
    worst = max(worst, _ratio(np.abs(pof + F), _exp_tol(F, 9)))
    ei_f = h.acq(_lib.GP_ACQ_EI | FEAS, 0.01, fmin)
    for nb in (0, 2):
        fl = h.acq_lp(_lib.GP_ACQ_EI | FEAS, 0.01, fmin, 0, Xb[:nb] if nb else None, r0[:nb] if nb else None, s0[:nb] if nb else None)
        # the penaliser's terms are the same on both sides: the flagged value differs by the transform's argument alone
        la, lb = np.log(-ei_f[:, 0] + 1e-50), np.log(-plain[_lib.GP_ACQ_EI][:, 0] + 1e-50)
        want = lp_plain[nb] - (la - lb)
        tol = (16 + 2 * nb) * U * (np.abs(fl) + np.abs(lp_plain[nb]) + np.abs(la) + np.abs(lb)) + 20 * U
        worst = max(worst, _ratio(np.abs(fl - want), tol))
    # with the cost as well: the product first, then the quotient
    kc = s.cons[0]
    h.cost_set(p.Xc[0], kc.alpha(), KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg)
    try:
        per = h.acq(_lib.GP_ACQ_EI | _lib.GP_ACQ_PER_COST, 0.01, fmin)
        both = h.acq(_lib.GP_ACQ_EI | _lib.GP_ACQ_PER_COST | FEAS, 0.01, fmin)
        worst = max(worst, _ratio(np.abs(both - per * F), _exp_tol(per * F, 14)))
    finally:
        h.cost_set(None, None, 0, 0, 1.0, None)
    print("FEAS scores case %s: worst error %.3f of the bound" % (cid, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("underflow", [False, True])
def test_flagged_selection_is_numpy_over_the_flagged_vector(underflow):
    s = setup("e")
    p, h = s.p, s.h
    mean, var = s.post_tab[:2]
    m = mean * p.c_std[:, None] + p.c_mean[:, None]
    sd = np.sqrt(np.maximum(var * p.c_std[:, None] ** 2, 1e-10))
    b = (m - 60.0 * sd).min(axis=1) if underflow else _bounds(s, 0.0, s.post_tab)
    h.set_candidates(p.Xtab)
    fmin = h.fmin()
    h.feas_table(_pack(s, b))
    t = _lib.GP_ACQ_EI | FEAS
    v = h.acq(t, 0.01, fmin)[:, 0]
    if underflow:
        assert np.all(v == 0.0)                                    # zeros of either sign tie: the lowest index wins
    i, val = h.acq_argbest(t, 0.01, fmin, -1)
    assert i == int(np.argmin(v)) and val == v[i]
    idx, vals = h.acq_topk(t, 0.01, fmin, -1, 5)
    order = np.argsort(v, kind="stable")[:5]
    assert list(idx) == list(order) and np.array_equal(np.asarray(vals), v[order])
    lpv = h.acq_lp(t, 0.01, fmin, 0)
    excl = [int(np.argmin(lpv)), 3]
    j, lval = h.acq_lp_argbest(t, 0.01, fmin, 0, -1, exclude=excl)
    masked = np.where(np.isin(np.arange(lpv.size), excl), np.inf, np.ravel(lpv))
    assert j == int(np.argmin(masked)) and lval == masked[j]


# ---- 6. rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["a", "b", "c", "f"])
@pytest.mark.parametrize("rule", ["EI", "MPI"])
def test_acq_rows_feas_against_the_truth(cid, rule):
    s = setup(cid)
    p, h, Xs = s.p, s.h, s.p.Xs
    b = _bounds(s, 0.0)
    pack = _pack(s, b)
    t = {"EI": _lib.GP_ACQ_EI, "MPI": _lib.GP_ACQ_MPI}[rule]
    fmin = h.fmin()
    a, da = h.acq_rows_feas(pack, Xs, t | FEAS, 0.01, fmin, grad=True)
    a2, da2 = h.acq_rows_feas(pack, Xs, t, 0.01, fmin, grad=True)
    assert np.array_equal(a, a2) and np.array_equal(da, da2)       # repeatable, and the flag is implied
    gm = O.OracleGPModel(s.gp)
    f0, df0 = (O.acq_EI_withGradients if rule == "EI" else O.acq_MPI_withGradients)(gm, Xs, 0.01)
    g = FT.fold(*s.post, p.c_mean, p.c_std, b)
    tl, td = FT.propagate(g, p.c_std, *_posterior_tolerance(s, s.post), s.post[2], s.post[3])
    tl, td = tl + g.bound_logF, td + g.bound_dlogF
    F = np.exp(g.logF)
    want = -(f0[:, 0] * F)
    dwant = -(df0 * F[:, None] + (f0[:, 0] * F)[:, None] * g.dlogF)
    # the acquisition's own tolerance of tests/test_gpu_rows.py (1e-5 of its largest value / gradient), times F, plus F's share
    ta = 1e-5 * np.abs(f0).max() * F + np.abs(want) * tl
    tda = (1e-5 * np.abs(df0).max() * F)[:, None] + np.abs(df0) * (F * tl)[:, None] + np.abs(want)[:, None] * (tl[:, None] * np.abs(g.dlogF) + td)
    r1, r2 = _ratio(np.abs(a[:, 0] - want), ta + 1e-300), _ratio(np.abs(da - dwant), tda + 1e-300)
    print("FEAS acq rows case %s %s: value %.3g gradient %.3g of the tolerance" % (cid, rule, r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0
    # the probability of feasibility alone
    pf, dpf = h.acq_rows_feas(pack, Xs, _lib.GP_ACQ_POF | FEAS, 0.0, 0.0, grad=True)
    lf, dlf = pack.rows(Xs, grad=True)
    assert np.all(np.abs(pf[:, 0] + np.exp(lf)) <= 10 * U * np.exp(lf) + 1e-322)
    assert np.all(np.abs(dpf + (np.exp(lf)[:, None] * dlf)) <= 12 * U * np.abs(np.exp(lf)[:, None] * dlf) + 1e-322)


@pytest.mark.parametrize("cid", ["b", "f"])
def test_a_location_does_not_depend_on_its_company(cid):
    s = setup(cid)
    p, h = s.p, s.h
    pack = _pack(s, _bounds(s, -1.0))
    fmin = h.fmin()
    rng = np.random.default_rng(5)
    x = p.Xs[:1]
    one = h.acq_rows_feas(pack, x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    lone = pack.rows(x, grad=True)
    for M, slot in ((4, 2), (5, 4), (8, 6)):
        Xs = rng.uniform(0, 1, (M, p.case.D))
        Xs[slot] = x[0]
        a, da = h.acq_rows_feas(pack, Xs, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
        assert np.array_equal(a[slot], one[0][0]) and np.array_equal(da[slot], one[1][0]), (M, slot)
        lf, dlf = pack.rows(Xs, grad=True)
        assert lf[slot] == lone[0][0] and np.array_equal(dlf[slot], lone[1][0]), (M, slot)


def test_acq_rows_feas_central_differences():
    s = setup("b")
    p, h = s.p, s.h
    pack = _pack(s, _bounds(s, -1.0))
    fmin = h.fmin()
    x = p.Xs[1:2]
    a, da = h.acq_rows_feas(pack, x, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
    eps = 1e-6
    for d in range(p.case.D):
        e = np.zeros((1, p.case.D))
        e[0, d] = eps
        num = (h.acq_rows_feas(pack, x + e, _lib.GP_ACQ_EI, 0.01, fmin) - h.acq_rows_feas(pack, x - e, _lib.GP_ACQ_EI, 0.01, fmin)) / (2 * eps)
        # central differences: truncation eps^2 |f'''| / 6 and cancellation u |f| / eps, both far below 1e-5 of the gradient's scale
        assert abs(num.item() - da[0, d]) <= 1e-5 * max(np.abs(da).max(), abs(a.item())), (d, num, da[0, d])


# ---- 7. gp_fmin_rows ---------------------------------------------------------------------------------------------------------------
def test_fmin_rows():
    s = setup("b")
    h, N = s.h, FT.N_SCORED
    assert h.fmin_rows(np.arange(N)) == h.fmin()
    rows = np.array([5, 17, 3, 199, 64])
    # gp_fmin's quantity from the oracle: the training mean K alpha = y - (noise + 1e-8) alpha
    mu = s.gp.predict(s.p.X, include_likelihood=False)[0][:, 0]
    assert abs(h.fmin_rows(rows) - mu[rows].min()) <= 1e-6 * max(1.0, abs(mu[rows].min()))
    assert h.fmin_rows(rows) >= h.fmin()
    for bad in ([], [N], [-1]):
        with pytest.raises(ValueError):
            h.fmin_rows(np.array(bad, dtype=np.int64))
    assert h.fmin_rows(np.arange(N)) == h.fmin()


# ---- 8. state and refusals ---------------------------------------------------------------------------------------------------------
def test_state_and_refusals():
    s = setup("d")
    p, h = s.p, s.h
    b = _bounds(s, 0.0, s.post_tab)
    pack = _pack(s, b)
    h.set_candidates(p.Xtab)
    fmin = h.fmin()
    t = _lib.GP_ACQ_EI | FEAS
    with pytest.raises(ValueError):
        h.acq(t, 0.01, fmin)                                       # no cache yet
    with pytest.raises(ValueError):
        h.acq(_lib.GP_ACQ_POF, 0.0, 0.0)                           # the rule without the flag
    h.feas_table(pack)
    ref = h.acq(t, 0.01, fmin).copy()
    with pytest.raises(ValueError):
        h.acq(_lib.GP_ACQ_LCB | FEAS, 2.0, fmin)
    with pytest.raises(ValueError):
        h.acq_rows_feas(pack, p.Xs, _lib.GP_ACQ_LCB, 2.0, fmin)
    with pytest.raises(ValueError):
        h.acq(_lib.GP_ACQ_POF, 0.0, 0.0)
    # every entry that was not taught the flag keeps refusing it, and the rule
    for tt in (t, _lib.GP_ACQ_POF, _lib.GP_ACQ_POF | FEAS):
        with pytest.raises(ValueError):
            h.acq_grad(tt, 0.01, fmin)
        with pytest.raises(ValueError):
            h.acq_lp_grad(tt, 0.01, fmin, 0)
        with pytest.raises(ValueError):
            h.acq_rows(p.Xs, tt, 0.01, fmin)
    # ... and so do the sparse model's and the ensemble's entries (a handle of its own: the shared one stays an exact model)
    o = _handle(p.X, p.Y, p, 1e-2)
    o.set_candidates(p.Xtab)
    o.feas_table(pack)
    o.sparse_set_inducing(p.X[:16])
    o.sparse_fit()
    o.sparse_set_candidates(p.Xtab)
    o.ens_fit(np.array([p.variance]), p.ls_arg[None, :], np.array([1e-2]))
    for tt in (t, _lib.GP_ACQ_POF, _lib.GP_ACQ_POF | FEAS):
        with pytest.raises(ValueError):
            o.sparse_acq(tt, 0.01, fmin)
        with pytest.raises(ValueError):
            o.sparse_acq_argbest(tt, 0.01, fmin, -1)
        with pytest.raises(ValueError):
            o.sparse_acq_rows(p.Xs, tt, 0.01, fmin)
        with pytest.raises(ValueError):
            o.ens_acq(tt, 0.01)
        with pytest.raises(ValueError):
            o.ens_acq_rows(p.Xs, tt, 0.01)
        with pytest.raises(ValueError):
            o.sparse_acq_topk(tt, 0.01, fmin, -1, 3)
        with pytest.raises(ValueError):
            o.ens_acq_argbest(tt, 0.01, -1)
    assert o.acq(t, 0.01, o.fmin()).shape == (p.case.Mtab, 1)         # the context is usable afterwards
    with pytest.raises(ValueError):                                   # a handle with a sparse fit / an ensemble is no constraint model
        h.feas_table(_lib.FeasPack([o], b, p.c_mean, p.c_std))
    o.close()
    # state: gp_feas_table needs data and resident candidates on the scored handle (not its fit)
    bare = _lib.Handle(0)
    with pytest.raises(RuntimeError):
        bare.feas_table(pack)
    bare.set_data(p.X, p.Y)
    with pytest.raises(RuntimeError):
        bare.feas_table(pack)
    bare.set_candidates(p.Xtab)
    bare.feas_table(pack)                                              # no gp_fit on `bare`: the cache does not depend on it
    assert np.array_equal(bare.feas_get_table(), h.feas_get_table())
    bare.close()
    # arguments: P != 1, an output warp, non-finite bound / c_mean, M < 1, K outside 1 .. GP_FEAS_MAX at the C boundary
    two = _lib.Handle(0)
    two.set_data(p.Xc[0], np.hstack([p.C[0], -p.C[0]]))
    two.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, 1e-3)
    two.fit()
    warped = _lib.Handle(0)
    warped.set_data(p.Xc[0], p.C[0])
    warped.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, 1e-3)
    warped.set_output_warp(np.array([[0.5, 1.0, 0.0]]))
    warped.fit()
    for bad in (two, warped):
        with pytest.raises(ValueError):
            h.feas_table(_lib.FeasPack([bad], b, p.c_mean, p.c_std))
        with pytest.raises(ValueError):
            _lib.FeasPack([bad], b, p.c_mean, p.c_std).rows(p.Xs)
        bad.close()
    for bb, cm in ((np.array([np.inf]), p.c_mean), (np.array([np.nan]), p.c_mean), (b, np.array([np.inf]))):
        with pytest.raises(ValueError):
            h.feas_table(_lib.FeasPack(s.cons, bb, cm, p.c_std))
        with pytest.raises(ValueError):
            h.acq_rows_feas(_lib.FeasPack(s.cons, bb, cm, p.c_std), p.Xs, _lib.GP_ACQ_EI, 0.01, fmin)
    with pytest.raises(ValueError):
        pack.rows(np.empty((0, p.case.D)))
    with pytest.raises(ValueError):
        h.acq_rows_feas(pack, np.empty((0, p.case.D)), _lib.GP_ACQ_EI, 0.01, fmin)
    out = np.empty(1)
    for K in (-1, _lib.GP_FEAS_MAX + 1):
        assert h.lib.gp_feas_table(h.h, *((pack.cons, K) + pack.args[2:])) == _lib.GP_ERR_ARG
    for K in (-1, 0, _lib.GP_FEAS_MAX + 1):
        assert h.lib.gp_feas_rows(*((pack.cons, K) + pack.args[2:] + (p.Xs.ctypes.data, 1, out.ctypes.data, None))) == _lib.GP_ERR_ARG
        assert h.lib.gp_acq_rows_feas(*((h.h, pack.cons, K) + pack.args[2:] + (p.Xs.ctypes.data, 1, _lib.GP_ACQ_EI, 0.01, fmin, 0.0, 1.0,
                                                                             out.ctypes.data, None))) == _lib.GP_ERR_ARG
    # constraint handles that will not do
    other = _lib.Handle(0)                                        # another width
    other.set_data(np.random.default_rng(3).uniform(0, 1, (50, p.case.D + 1)), p.Y[:50])
    other.set_params(_lib.GP_KERNEL_MATERN52, 0, 1.0, np.array([0.5]), 1e-2)
    other.fit()
    for bad in ([h], [s.cons[0], s.cons[0]], [other]):
        with pytest.raises(ValueError):
            h.feas_table(_lib.FeasPack(bad, b[:1].repeat(len(bad)), np.zeros(len(bad)), np.ones(len(bad))))
    with pytest.raises(ValueError):
        h.feas_table(_lib.FeasPack(s.cons, b, p.c_mean, -p.c_std))
    unfit = _lib.Handle(0)
    unfit.set_data(p.Xc[0], p.C[0])
    unfit.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, 1e-3)
    with pytest.raises(RuntimeError):
        h.feas_table(_lib.FeasPack([unfit], b, p.c_mean, p.c_std))
    with pytest.raises(RuntimeError):
        _lib.Handle(0).feas_get_table()
    # a refused call changed nothing, and the context is usable
    assert h.feas_info() == (p.case.K, p.case.Mtab)
    assert np.array_equal(h.acq(t, 0.01, fmin), ref)
    # the cache is a snapshot: a constraint handle refitted or closed afterwards leaves the flagged calls valid
    c2 = _handle(p.Xc[0], p.C[0], p, p.noise[0])
    h.feas_table(_lib.FeasPack([c2], b, p.c_mean, p.c_std))
    assert np.array_equal(h.acq(t, 0.01, fmin), ref)
    c2.set_params(KID[p.case.fam], int(p.case.ard), 0.5 * p.variance, p.ls_arg, 1e-1)
    c2.fit()
    assert np.array_equal(h.acq(t, 0.01, fmin), ref)
    c2.close()
    assert np.array_equal(h.acq(t, 0.01, fmin), ref)
    # dropped by gp_set_candidates and by K = 0
    h.feas_table(None)
    assert h.feas_info() == (0, 0)
    h.feas_table(pack)
    h.set_candidates(p.Xtab[:5])
    with pytest.raises(ValueError):
        h.acq(t, 0.01, fmin)
    assert h.acq(_lib.GP_ACQ_EI, 0.01, fmin).shape == (5, 1)
    # the constraint handle's resident table is the scored handle's after gp_feas_table
    h.feas_table(pack)
    assert s.cons[0].M == 5


def test_the_replica_group_refuses_the_flag():
    """gp_group_acq_argbest / _lp_argbest / _topk build their own spec: neither GP_ACQ_TIMES_FEAS nor GP_ACQ_POF is understood, and
    the group scores as before afterwards."""
    s = setup("d")
    p, h = s.p, s.h
    h.set_candidates(p.Xtab)
    fmin = h.fmin()
    t = _lib.GP_ACQ_EI | FEAS
    grp = _lib.Group([0])
    grp.set_data(p.X, p.Y)
    grp.set_params(KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg, 1e-2)
    grp.fit()
    grp.set_candidates(p.Xtab)
    for tt in (t, _lib.GP_ACQ_POF, _lib.GP_ACQ_POF | FEAS):
        with pytest.raises(ValueError):
            grp.acq_argbest(tt, 0.01, fmin, -1)
        with pytest.raises(ValueError):
            grp.acq_lp_argbest(tt, 0.01, fmin, 0, -1)
        with pytest.raises(ValueError):
            grp.acq_topk(tt, 0.01, fmin, -1, 3)
    assert grp.acq_argbest(_lib.GP_ACQ_EI, 0.01, fmin, -1)[0] == h.acq_argbest(_lib.GP_ACQ_EI, 0.01, fmin, -1)[0]
    grp.close()


# ---- 9. model level ----------------------------------------------------------------------------------------------------------------
def _disc():
    """A 2-D problem whose feasible region is the disc of radius 0.3 around the centre of the unit square; N = 30."""
    rng = np.random.default_rng(77)
    X = rng.uniform(0, 1, (30, 2))
    X[0] = (0.5, 0.5)

    def f(x):
        x = np.atleast_2d(x)
        return (np.sin(3 * x[:, 0]) + (x[:, 1] - 0.3) ** 2)[:, None]

    def c(x):
        x = np.atleast_2d(x)
        return (((x - 0.5) ** 2).sum(1) - 0.09)[:, None]
    return X, f, c


@pytest.mark.parametrize("cls", [gpo.AcquisitionEI, gpo.AcquisitionMPI])
def test_acquisition_with_feasibility_equals_the_host_formula(cls):
    X, f, c = _disc()
    Y, C = f(X), c(X)
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, 1.0, 0.4), noise_var=1e-3, max_iters=0, verbose=False)
    gm.updateModel(X, (Y - Y.mean()) / Y.std(), None, None)
    fm = gpo.FeasibilityModel(1, 0.0, noise_var=1e-3, max_iters=0, verbose=False)
    fm.update(X, C)
    ok = fm.feasible(C)
    assert 0 < ok.sum() < 30 and np.array_equal(fm.feasible_rows, np.flatnonzero(ok))
    acq = cls(gm, jitter=0.01, feasibility=fm)
    assert acq._acq_id == acq._rule.device_id | FEAS and acq._route() is not None
    rng = np.random.default_rng(8)

    def host(x):
        fmin = gm.predict(X[ok], with_noise=False)[0].min()
        val, dval = acq._rule.gradient(0.01, fmin, *gm.predict_withGradients(x))
        logF, dlogF = fm.log_probability_withGradients(x, host=True)
        F = np.exp(logF)[:, None]
        return -(val * F), -F * (dval + val * dlogF)

    # the north-star tolerance of the posterior routes (1e-6 of the largest entry): the incumbent comes from two routes
    # (y - d alpha on the device, K alpha here), everything else agrees to rounding
    for M in (1, 5, 20):
        x = rng.uniform(0.1, 0.9, (M, 2))
        a, da = acq.acquisition_function_withGradients(x)
        want, dwant = host(x)
        assert np.max(np.abs(a - want)) <= 1e-6 * np.abs(want).max(), (M, a, want)
        assert np.max(np.abs(da - dwant)) <= 1e-6 * np.abs(dwant).max(), (M, da, dwant)
        v = acq.acquisition_function(x)
        assert np.max(np.abs(v - want)) <= 1e-6 * np.abs(want).max()
    tab = rng.uniform(0, 1, (200, 2))
    v = acq.acquisition_function(tab)
    assert np.max(np.abs(v - host(tab)[0])) <= 1e-6 * np.abs(v).max()
    i, val = acq.argbest(tab, -1)
    assert i == int(np.argmin(v)) and val == v[i, 0]
    lp = gpo.AcquisitionLP(gm, acquisition=acq)
    lv = lp.acquisition_function(tab)
    assert np.max(np.abs(lv + np.log(-v[:, 0] + 1e-50))) <= 1e-9 * np.abs(lv).max()
    j, _ = lp.argbest(tab, +1, exclude=(int(np.argmax(lv)),))
    masked = lv.copy()
    masked[int(np.argmax(lv))] = -np.inf
    assert j == int(np.argmax(masked))
    with pytest.raises(NotImplementedError):
        lp.acquisition_function_withGradients(tab[:2])
    # while no observation is feasible the rule is the probability of feasibility alone
    none = gpo.FeasibilityModel(1, -10.0, noise_var=1e-3, max_iters=0, verbose=False)
    none.update(X, C)
    pof = cls(gm, jitter=0.01, feasibility=none)
    assert pof._acq_id == _lib.GP_ACQ_POF | FEAS
    x = rng.uniform(0.1, 0.9, (3, 2))
    a, da = pof.acquisition_function_withGradients(x)
    logF, dlogF = none.log_probability_withGradients(x, host=True)
    assert np.max(np.abs(a[:, 0] + np.exp(logF))) <= 1e-9 * np.exp(logF).max() + 1e-300
    assert np.max(np.abs(da + np.exp(logF)[:, None] * dlogF)) <= 1e-9 * np.abs(np.exp(logF)[:, None] * dlogF).max() + 1e-300


@pytest.mark.parametrize("evaluator,batch", [("sequential", 1), ("random", 2), ("thompson_sampling", 2)])
def test_bayesian_optimization_with_a_constraint_function(evaluator, batch):
    X, f, c = _disc()
    np.random.seed(3)
    bo = gpo.BayesianOptimization(f, domain=[{"name": "x", "type": "continuous", "domain": (0, 1), "dimensionality": 2}], X=X[:8],
                                  constraint_function=c, evaluator_type=evaluator, batch_size=batch, max_iters=0,
                                  exact_feval=True)
    x_opt, fx_opt = bo.run_optimization(max_iter=3)
    assert bo.X.shape[0] == 8 + 3 * batch and bo.C.shape == (bo.X.shape[0], 1) and bo.feasibility.generation >= 3
    assert c(x_opt)[0, 0] <= 0.0                                   # the reported optimum is feasible
    ok = bo.feasibility.feasible(bo.C)
    assert fx_opt == bo.Y[ok, 0].min()


def test_bayesian_optimization_refuses_local_penalization_with_constraints():
    X, f, c = _disc()
    with pytest.raises(InvalidConfigError):
        gpo.BayesianOptimization(f, domain=[{"name": "x", "type": "continuous", "domain": (0, 1), "dimensionality": 2}], X=X[:8],
                                 constraint_function=c, evaluator_type="local_penalization", batch_size=2)


# ---- the substitution fallback: handles that cannot take the fused route ----------------------------------------------------------------
def _route_tolerance(s, post, b):
    """Two float64 routes to one posterior (fused rows over L^-1 against the table posterior over L): 1e-9 of each other on these
    well-conditioned models (tests/test_gpu_rows.py; 1e-8 for d var / dx), propagated through the fold"""
    mean, var, dm, dv = post
    g = FT.fold(*post, s.p.c_mean, s.p.c_std, b)
    d_dm = np.broadcast_to(1e-9 * np.maximum(np.abs(dm).max(axis=(1, 2)), 1e-3)[:, None, None], dm.shape)
    tl, td = FT.propagate(g, s.p.c_std, 1e-9 * np.maximum(1.0, np.abs(mean)), 1e-9 * np.sqrt(var) + 1e-12, d_dm,
                          np.full(dv.shape, 1e-8 * s.p.variance), dm, dv)
    return g, np.asarray(tl + 2 * g.bound_logF, float), np.asarray(td + 2 * g.bound_dlogF, float)


@pytest.mark.parametrize("cid", ["c", "f"])
def test_handles_on_the_fallback_route_agree_with_the_fused_route(cid):
    """small_m = 0 takes a handle off the fused route: its results are folded from its table buffers.  The scored handle alone,
    one constraint alone, every handle -- log F, the flagged rows (with the cost as well, and the probability alone), values and
    gradients, against all handles fused."""
    s = setup(cid)
    p, h, Xs = s.p, s.h, s.p.Xs
    b = _bounds(s, -1.0)
    pack = _pack(s, b)
    fmin = h.fmin()
    h.cost_set(p.Xc[0], s.cons[0].alpha(), KID[p.case.fam], int(p.case.ard), p.variance, p.ls_arg)
    types = (_lib.GP_ACQ_EI, _lib.GP_ACQ_MPI | _lib.GP_ACQ_PER_COST, _lib.GP_ACQ_POF | FEAS)

    def everything():
        return [pack.rows(Xs, grad=True), (pack.rows(Xs),)] + [h.acq_rows_feas(pack, Xs, t, 0.01, fmin, grad=True) for t in types] + \
               [(h.acq_rows_feas(pack, Xs, t, 0.01, fmin),) for t in types]

    g, tl, td = _route_tolerance(s, s.post, b)
    try:
        ref = everything()
        before = [o.rows_stats()["fallback"] for o in [h] + s.cons]
        worst = 0.0
        for off in ([h], [s.cons[-1]], [h] + s.cons):
            for o in off:
                o.set_option("small_m", 0)
            got = everything()
            for o in off:
                o.set_option("small_m", 8)
            for n, (r, q) in enumerate(zip(ref, got)):
                is_logF = n < 2                                        # the first two entries are log F itself, the rest scores
                a, a0 = q[0].reshape(len(Xs)), r[0].reshape(len(Xs))
                worst = max(worst, _ratio(np.abs(a - a0), (tl if is_logF else np.abs(a0) * (1e-8 + tl)) + 1e-300))
                if len(q) > 1:
                    da, da0 = q[1], r[1]
                    tg = td if is_logF else (1e-7 * np.abs(da0).max() + np.abs(da0) * tl[:, None] +
                                             np.abs(a0)[:, None] * (tl[:, None] * np.abs(np.asarray(g.dlogF, float)) + td))
                    worst = max(worst, _ratio(np.abs(da - da0), tg + 1e-300))
        after = [o.rows_stats()["fallback"] for o in [h] + s.cons]
        assert all(x > y for x, y in zip(after, before))               # every handle did take the fallback
        print("FEAS fallback case %s: worst difference to the fused route %.3g of the tolerance" % (cid, worst))
        assert worst <= 1.0
        assert np.array_equal(everything()[2][0], ref[2][0])           # back on the fused route: the same bits as before
    finally:
        for o in [h] + s.cons:
            o.set_option("small_m", 8)
        h.cost_set(None, None, 0, 0, 1.0, None)


def test_a_rows_call_on_the_fallback_route_does_not_strand_the_table_cache():
    """A rows call that takes the substitution fallback makes its locations the scored handle's resident table inside the library
    and drops the cache of gp_feas_table with the old one; the next call on the same table object stages and caches it again."""
    X, f, c = _disc()
    Y, C = f(X), c(X)
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, 1.0, 0.4), noise_var=1e-3, max_iters=0, verbose=False)
    gm.updateModel(X, (Y - Y.mean()) / Y.std(), None, None)
    fm = gpo.FeasibilityModel(1, 0.0, noise_var=1e-3, max_iters=0, verbose=False)
    fm.update(X, C)
    acq = gpo.AcquisitionEI(gm, jitter=0.01, feasibility=fm)
    tab = np.random.default_rng(4).uniform(0, 1, (50, 2))
    v = acq.acquisition_function(tab)
    hd = gm.model._h
    assert hd.feas_info() == (1, 50)
    for option in ("small_m", None):                                  # the scored handle on the fallback, then a plain rows call
        if option:
            hd.set_option(option, 0)
        try:
            a, da = acq.acquisition_function_withGradients(tab[:2])
            if option:
                assert hd.feas_info() == (0, 0) and hd.feas_key is not None     # dropped in the library, the Python key stands
        finally:
            hd.set_option("small_m", 8)
        i, val = acq.argbest(tab, -1)
        assert i == int(np.argmin(v)) and val == v[i, 0] and hd.feas_info() == (1, 50)
        assert np.array_equal(acq.acquisition_function(tab), v)
        assert np.max(np.abs(a - v[:2])) <= 1e-8 * np.abs(v[:2]).max()
