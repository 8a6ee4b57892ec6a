"""GPU: entropy search on the device -- the EP sweeps of p_min (gp_es_pmin), the representers' posterior
(gp_es_set_representers), the scoring of candidate tables (gp_es_acq / gp_es_acq_argbest) and of a handful of locations
(gp_es_acq_rows), their state rules, and the class.

References: the reference's own ``epmgp.joint_min`` outputs recorded in tests/golden/es_epmgp.npz (made by
tests/golden/generate_es.py), the long-double statement tests/_es_truth.py, and oracle.cpu_ref for the posterior.

Tolerances.  EP: 1e-9 of each array's largest magnitude over the entries with logP > -400 (the reference's outputs move by
3e-12 under a 1e-13 perturbation of their inputs); status and sweep counts equal the truth's (the fixture keeps every chain's
last sum |d| 10 % away from the 1e-3 threshold and every z 1e-6 away from +-6).  Representers: 1e-9 of the largest entry.  Scores:
1e-9 of the largest |value| on models with noise 1e-2 -- the project's rule for posterior-derived values -- and 1e-6 on one
ill-conditioned model with noise 1e-6.  Every comparison prints its figure before it asserts.
"""
import functools
import os

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import entropy_search as E
from oracle import cpu_ref as O

import _es_truth as T
import _kernel_families as KF

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "es_epmgp.npz"))
TAGS = sorted({k.split("/")[0] for k in G.files})
KERN = {"rbf": gpo.kern.RBF, "Mat52": gpo.kern.Matern52, "Mat32": gpo.kern.Matern32, "Exponential": gpo.kern.Exponential}
DOMAIN = [{"name": "a", "type": "continuous", "domain": (0.0, 1.0)}, {"name": "b", "type": "continuous", "domain": (0.0, 2.0)},
          {"name": "c", "type": "discrete", "domain": (0, 1, 2)}]


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=float), np.asarray(ref, dtype=float)
    return float(np.max(np.abs(a - ref)) / max(np.max(np.abs(ref)), 1e-300)) if ref.size else 0.0


@functools.lru_cache(maxsize=None)
def _handle():
    return gpo._lib.Handle(0)


@functools.lru_cache(maxsize=None)
def _truth_sweeps(tag):
    return T.sweeps(G[tag + "/mu"], G[tag + "/cov"])


# ---- EP ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_pmin_matches_the_truth_and_the_reference(tag):
    mu, cov = G[tag + "/mu"], G[tag + "/cov"]
    sw = _truth_sweeps(tag)
    P, MP, logS, status, sweeps = _handle().es_pmin(mu, cov)
    print(tag, "status", np.bincount(status + 2, minlength=4), "sweeps", sweeps.min(), sweeps.max())
    assert np.array_equal(status, sw["status"])
    assert np.array_equal(sweeps, sw["sweeps"])
    logP, dMu, dSigma, dMuMu = E.joint_min(mu, cov, (P, MP, logS, status))
    ok = G[tag + "/logP"] > -400
    figs = {"logP": _rel(logP[ok], G[tag + "/logP"][ok]), "dlogPdMu": _rel(dMu[ok], G[tag + "/dlogPdMu"][ok])}
    if tag + "/dlogPdSigma" in G.files:
        figs["dlogPdSigma"] = _rel(dSigma[ok], G[tag + "/dlogPdSigma"][ok])
        figs["dlogPdMudMu"] = _rel(dMuMu[ok], G[tag + "/dlogPdMudMu"][ok])
    else:
        Q = E.quadratic_forms(dSigma, dMuMu)
        det = np.array([np.einsum("iab,a,b->i", Q, m, m) for m in G[tag + "/m"]])
        figs["det"] = _rel(det[:, ok], G[tag + "/det"][:, ok])
    print(tag, " ".join("%s %.2e" % kv for kv in figs.items()))
    assert np.array_equal(logP[~ok], G[tag + "/logP"][~ok]) or _rel(logP[~ok], G[tag + "/logP"][~ok]) < 1e-9
    for name, fig in figs.items():
        assert fig < 1e-9, name


def test_pmin_is_a_pure_function_and_bounds_its_sweeps():
    mu, cov = G["R20m1/mu"], G["R20m1/cov"]
    h = _handle()
    a, b = h.es_pmin(mu, cov), h.es_pmin(mu, cov)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    status, sweeps = h.es_pmin(mu, cov, max_sweeps=1)[3:]
    assert np.all(sweeps == 1) and set(status) <= {1, -1, 0}
    assert np.all(status[_truth_sweeps("R20m1")["sweeps"] > 1] != 0)
    one = h.es_pmin(np.array([0.3]), np.array([[1.0]]))
    assert one[3].tolist() == [0] and one[0].shape == (1, 0)
    for R in (0, 65):
        with pytest.raises(ValueError):
            h.es_pmin(np.zeros(R), np.eye(R))


# ---- models -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(fam, N, D, noise, ard=False, gower=False, seed=3):
    rng = np.random.default_rng(1000 * N + seed)
    if gower:
        D = 3
        X = np.c_[rng.uniform(0, 1, N), rng.uniform(0, 2, N), rng.integers(0, 3, N).astype(float)]
    else:
        X = rng.uniform(0, 1, (N, D))
    Y = (np.sin(3 * X.sum(1)) + 0.1 * rng.standard_normal(N))[:, None]
    ls = np.linspace(0.4, 0.9, D) if ard else np.array([0.6])
    if gower:
        ok = O.make_kernel(fam, D, 1.3, ls, ARD=ard, Gower=True, space=O.MixedSpace(DOMAIN))
        dk = KERN[fam](D, variance=1.3, lengthscale=ls, ARD=ard, Gower=True, space=gpo.Design_space(DOMAIN))
    else:
        ok = KF.make(fam, D, 1.3, ls, ard)
        dk = KERN[fam](D, variance=1.3, lengthscale=ls, ARD=ard)
    oracle = O.OracleGP(X, Y, ok, noise)
    dev = gpo.models.GPRegression(X, Y, dk, noise_var=noise)
    dev._ensure_fit()
    X.setflags(write=False)
    return oracle, dev, X


def _points(rng, n, D, gower=False):
    if gower:
        return np.c_[rng.uniform(0, 1, n), rng.uniform(0, 2, n), rng.integers(0, 3, n).astype(float)]
    return rng.uniform(0, 1, (n, D))


# ---- representers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,N,R,ard,gower", [("rbf", 5, 1, False, False), ("Mat52", 128, 2, False, False),
                                                ("Mat32", 129, 17, True, False), ("Exponential", 300, 64, False, False),
                                                ("rbf", 300, 17, True, False), ("Mat52", 5, 64, False, False),
                                                ("rbf", 129, 17, False, True)])
def test_representers_posterior(fam, N, R, ard, gower):
    oracle, dev, _ = _model(fam, N, 3, 1e-2, ard, gower)
    Xr = _points(np.random.default_rng(R), R, 3, gower)
    y_mean, y_std = 0.7, 1.9
    mu_ref, cov_ref = oracle.predict(Xr, full_cov=True)
    mu, cov = dev._h.es_set_representers(Xr, y_mean, y_std)
    figs = _rel(mu, mu_ref.ravel() * y_std + y_mean), _rel(cov, cov_ref * y_std ** 2)
    print(fam, N, R, "mu %.2e cov %.2e" % figs)
    assert max(figs) < 1e-9
    assert np.array_equal(cov, cov.T) or _rel(cov, cov.T) < 1e-12


# ---- scoring ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _belief(fam, N, R, noise, seed=3, soften=0.0):
    """Representers of a model and a belief over them: inputs of the scoring entries (the package's host algebra makes them; the
    scores are checked against tests/_es_truth.py, which takes them as given).  ``soften`` is added to the diagonal of the
    covariance the belief is computed from: at noise 1e-6 the representers' own posterior gives a belief with all its mass on one
    point, under which every candidate scores the same."""
    oracle, dev, _ = _model(fam, N, 3, noise, seed=seed)
    rng = np.random.default_rng(50 + R)
    Xr = rng.uniform(0, 1, (R, 3))
    mu, cov = oracle.predict(Xr, full_cov=True)
    cov = np.maximum(cov, 1e-10) + soften * np.eye(R)
    logP, dMu, dSigma, dMuMu = (np.zeros(1), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1, 1))) if R == 1 else \
        E.joint_min(mu.ravel(), cov)
    u = -rng.uniform(0.5, 6.0, R)
    for a in (Xr, logP, dMu, dSigma, dMuMu, u):
        a.setflags(write=False)
    return Xr, logP, u, dMu, dSigma, dMuMu


def _quantiles(S):
    from scipy.stats import norm
    return norm.ppf(np.linspace(1. / (S + 1), 1 - 1. / (S + 1), S))


def _truth_scores(oracle, Xr, Xs, rows, logP, u, dMu, dSigma, dMuMu, W, y_std):
    _, var0 = oracle.predict_noiseless(Xs[rows])
    C = oracle.posterior_covariance_between_points(Xr, Xs[rows])          # [R, rows]
    out = []
    for j in range(len(rows)):
        m = C[:, j] * y_std ** 2 / np.sqrt(max(float(var0[j, 0]) * y_std ** 2, 1e-10))
        out.append(T.score(m, logP, u, dMu, T.det_reference_style(m, dSigma, dMuMu), W))
    return np.array(out)


def _load(dev, Xr, logP, u, dMu, dSigma, dMuMu, W, y_std=1.0):
    dev._h.es_set_representers(Xr, 0.0, y_std)
    dev._h.es_set_belief(logP, u, dMu, E.quadratic_forms(dSigma, dMuMu), W)


def _candidates(rng, M, Xr):
    """Half of them uniform, half next to a representer (large innovations): the scores must differ from row to row."""
    Xs = rng.uniform(0, 1, (M, Xr.shape[1]))
    near = np.arange(M // 2, M)
    Xs[near] = np.clip(Xr[near % Xr.shape[0]] + 0.03 * rng.standard_normal((near.size, Xr.shape[1])), 0, 1)
    return Xs


def _sample_rows(M, n=24):
    return np.unique(np.r_[0, M - 1, np.linspace(0, M - 1, min(n, M)).astype(int), [r for r in (127, 128, 255, 256) if r < M]]).astype(int)


@pytest.mark.parametrize("M,N,R,S,mc_max,y_std", [(1, 5, 2, 1, None, 1.0), (7, 129, 17, 7, None, 2.5), (129, 300, 50, 100, None, 1.0),
                                                  (300, 129, 64, 100, 128, 1.0), (300, 300, 17, 7, None, 0.4), (7, 5, 1, 7, None, 1.0)])
def test_table_scores_match_the_truth(M, N, R, S, mc_max, y_std):
    oracle, dev, _ = _model("Mat52", N, 3, 1e-2)
    Xr, logP, u, dMu, dSigma, dMuMu = _belief("Mat52", N, R, 1e-2)
    W = _quantiles(S)
    Xs = _candidates(np.random.default_rng(M), M, Xr)
    _load(dev, Xr, logP, u, dMu, dSigma, dMuMu, W, y_std)
    h = dev._h
    if mc_max:
        h.set_option("mc_max", mc_max)      # three chunks of the candidate solve
    try:
        h.set_candidates(Xs)
        out = h.es_acq(y_std)
        again = h.es_acq(y_std)
    finally:
        h.set_option("mc_max", 16384)
    assert out.shape == (M, 1) and np.array_equal(out, again)
    rows = _sample_rows(M)
    ref = _truth_scores(oracle, Xr, Xs, rows, logP, u, dMu, dSigma, dMuMu, W, y_std)
    fig = float(np.max(np.abs(out[rows, 0] - ref)) / np.max(np.abs(ref)))
    print("M %d N %d R %d S %d: %.2e (largest |value| %.3g, spread %.3g)" % (M, N, R, S, fig, np.max(np.abs(ref)), np.ptp(ref)))
    assert fig < 1e-9
    assert M == 1 or R == 1 or np.ptp(ref) > 1e-3 * np.max(np.abs(ref))      # the candidates do score differently
    # a candidate's value does not depend on M or on its row: the same location alone, and in another table.  (To rounding: the
    # scoring kernel's sums are the same, but the candidate solve in front of it picks its GEMM instance by the table's size.)
    k = int(rows[len(rows) // 2])
    scale = np.max(np.abs(out))
    h.set_candidates(Xs[k:k + 1])
    assert abs(h.es_acq(y_std)[0, 0] - out[k, 0]) <= 1e-11 * scale
    h.set_candidates(np.vstack([Xs[::-1], Xs[k:k + 1]]))
    rev = h.es_acq(y_std)
    assert abs(rev[M, 0] - out[k, 0]) <= 1e-11 * scale and np.max(np.abs(rev[:M][::-1] - out)) <= 1e-11 * scale


def test_table_scores_on_an_ill_conditioned_model():
    """rbf, N = 129 in three dimensions, noise 1e-6: cond(Ky) ~ 1e8.  The posterior is tight there, so the innovations are small;
    an output scale of 100 (the normaliser's y_std) brings them to ~0.5 and the scores apart."""
    oracle, dev, _ = _model("rbf", 129, 3, 1e-6)
    Xr, logP, u, dMu, dSigma, dMuMu = _belief("rbf", 129, 17, 1e-6, soften=0.05)
    W, y_std = _quantiles(7), 100.0
    Xs = _candidates(np.random.default_rng(9), 40, Xr)
    _load(dev, Xr, logP, u, dMu, dSigma, dMuMu, W, y_std)
    dev._h.set_candidates(Xs)
    out = dev._h.es_acq(y_std)
    ref = _truth_scores(oracle, Xr, Xs, np.arange(40), logP, u, dMu, dSigma, dMuMu, W, y_std)
    fig = float(np.max(np.abs(out[:, 0] - ref)) / np.max(np.abs(ref)))
    print("noise 1e-6: %.2e (largest |value| %.3g, spread %.3g)" % (fig, np.max(np.abs(ref)), np.ptp(ref)))
    assert fig < 1e-6 and np.ptp(ref) > 1e-3 * np.max(np.abs(ref))


def test_scores_under_emulation_stay_fp64_in_the_new_kernels():
    oracle, dev, _ = _model("Mat52", 300, 3, 1e-2)
    Xr, logP, u, dMu, dSigma, dMuMu = _belief("Mat52", 300, 17, 1e-2)
    W = _quantiles(7)
    Xs = np.random.default_rng(4).uniform(0, 1, (129, 3))
    _load(dev, Xr, logP, u, dMu, dSigma, dMuMu, W)
    h = dev._h
    h.set_candidates(Xs)
    plain = h.es_acq()
    h.set_option("emulate_fp64", 1)
    try:
        h.set_candidates(Xs)
        emu = h.es_acq()
    finally:
        h.set_option("emulate_fp64", 0)
    fig = _rel(emu, plain)
    print("emulated candidate solve: %.2e" % fig)
    assert fig < 1e-9


def test_argbest_is_the_lowest_index_best_bitwise():
    oracle, dev, _ = _model("Mat52", 129, 3, 1e-2)
    Xr, logP, u, dMu, dSigma, dMuMu = _belief("Mat52", 129, 17, 1e-2)
    _load(dev, Xr, logP, u, dMu, dSigma, dMuMu, _quantiles(7))
    h = dev._h
    base = np.random.default_rng(2).uniform(0, 1, (150, 3))
    for Xs in (base, np.vstack([base, base[::-1], base])):      # the second table holds every row three times
        h.set_candidates(Xs)
        out = h.es_acq()[:, 0]
        for sense, pick in ((-1, np.argmin), (+1, np.argmax)):
            idx, val = h.es_acq_argbest(sense)
            assert idx == int(pick(out)) and val == out[idx]
    with pytest.raises(ValueError):
        h.es_acq_argbest(0)


# ---- a handful of locations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,R,gower,y_std", [(129, 3, 17, False, 1.0), (300, 3, 50, False, 2.5), (5, 3, 2, False, 1.0),
                                               (640, 20, 17, False, 1.0), (129, 3, 17, True, 1.0)])
def test_rows_match_the_table_route_and_do_not_depend_on_their_company(N, D, R, gower, y_std):
    """M = 1 .. 8 fused against the table route at 1e-9 of the largest |value|; a location alone and among eight: equal bits;
    M = 9 takes the table route.  D = 20: eight locations do not fit one wide pass (passes of four); N = 640: 128-row blocks."""
    oracle, dev, _ = _model("Mat52", N, D, 1e-2, gower=gower)
    D = 3 if gower else D
    rng = np.random.default_rng(N + R)
    Xr = _points(rng, R, D, gower)
    mu, cov = oracle.predict(Xr, full_cov=True)
    logP, dMu, dSigma, dMuMu = E.joint_min(mu.ravel(), np.maximum(cov, 1e-10))
    u, W = -rng.uniform(0.5, 6.0, R), _quantiles(7)
    _load(dev, Xr, logP, u, dMu, dSigma, dMuMu, W, y_std)
    h = dev._h
    Xs = _points(rng, 9, D, gower)
    h.set_candidates(Xs)
    table = h.es_acq(y_std)
    scale = np.max(np.abs(table))
    before = h.rows_stats()
    worst = 0.0
    for M in range(1, 9):
        rows = h.es_acq_rows(Xs[:M], y_std)
        assert rows.shape == (M, 1)
        worst = max(worst, float(np.max(np.abs(rows - table[:M]))) / scale)
    print("N %d D %d R %d rows against table: %.2e" % (N, D, R, worst))
    assert worst < 1e-9
    mid = h.rows_stats()
    assert mid["fused"] == before["fused"] + 8 and mid["fallback"] == before["fallback"]
    eight = h.es_acq_rows(Xs[:8], y_std)
    for k in (0, 3, 4, 7):
        assert h.es_acq_rows(Xs[k:k + 1], y_std)[0, 0] == eight[k, 0]
    assert np.array_equal(h.es_acq_rows(Xs[:8][::-1], y_std)[::-1], eight)
    assert np.array_equal(h.es_acq_rows(Xs[2:6], y_std), eight[2:6])
    nine = h.es_acq_rows(Xs, y_std)
    after = h.rows_stats()
    assert after["fallback"] == mid["fallback"] + 1
    assert np.max(np.abs(nine - table)) <= 1e-11 * scale


def test_rows_refuse_without_a_belief_and_after_a_refit():
    h, X, Y = _fresh()
    with pytest.raises(RuntimeError, match="gp_es_set_representers"):
        h.es_acq_rows(X[:2])
    _with_belief(h)
    assert np.all(np.isfinite(h.es_acq_rows(X[:2] + 0.01)))
    h.fit()
    with pytest.raises(RuntimeError, match="gp_es_set_representers"):
        h.es_acq_rows(X[:2])
    with pytest.raises(ValueError):
        h.es_acq_rows(np.zeros((0, 2)))


# ---- state and refusals -----------------------------------------------------------------------------------------------------
def _fresh(N=40, P=1):
    rng = np.random.default_rng(8)
    X = rng.uniform(0, 1, (N, 2))
    Y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, P))
    h = gpo._lib.Handle(0)
    h.set_data(X, Y)
    h.set_params(gpo._lib.GP_KERNEL_RBF, 0, 1.0, np.array([0.5]), 1e-2)
    h.fit()
    return h, X, Y


def _with_belief(h, R=5, S=3):
    rng = np.random.default_rng(R)
    Xr = rng.uniform(0, 1, (R, 2))
    mu, cov = h.es_set_representers(Xr)
    logP, dMu, dSigma, dMuMu = E.joint_min(mu, np.maximum(cov, 1e-10), h.es_pmin(mu, np.maximum(cov, 1e-10)))
    h.es_set_belief(logP, -np.ones(R), dMu, E.quadratic_forms(dSigma, dMuMu), _quantiles(S))
    h.set_candidates(rng.uniform(0, 1, (9, 2)))
    return Xr, (logP, -np.ones(R), dMu, E.quadratic_forms(dSigma, dMuMu), _quantiles(S))


def test_scoring_needs_representers_and_a_belief_of_their_size():
    h, X, Y = _fresh()
    h.set_candidates(X[:4])
    with pytest.raises(RuntimeError, match="gp_es_set_representers"):
        h.es_acq()
    h.es_set_representers(X[:5] + 0.01)
    with pytest.raises(RuntimeError, match="gp_es_set_belief"):
        h.es_acq()
    with pytest.raises(RuntimeError, match="gp_es_set_belief"):
        h.es_acq_argbest(-1)
    with pytest.raises(RuntimeError, match="representers are 5"):
        h.es_set_belief(np.zeros(4), np.zeros(4), np.zeros((4, 4)), np.zeros((4, 4, 4)), np.zeros(3))
    Xr, belief = _with_belief(h)
    assert np.all(np.isfinite(h.es_acq()))
    h.es_set_representers(Xr)               # new representers drop the belief
    with pytest.raises(RuntimeError, match="gp_es_set_belief"):
        h.es_acq()


def test_argument_ranges():
    h, X, Y = _fresh()
    for R in (0, 65):
        with pytest.raises(ValueError, match="R out of range"):
            h.es_set_representers(np.zeros((R, 2)))
    h.es_set_representers(X[:3] + 0.01)
    for S in (0, 1025):
        with pytest.raises(ValueError, match="S out of range"):
            h.es_set_belief(np.zeros(3), np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3, 3)), np.zeros(S))
    h2, X2, _ = _fresh(P=2)
    with pytest.raises(ValueError, match="P == 1"):
        h2.es_set_representers(X2[:3] + 0.01)


@pytest.mark.parametrize("change", ["set_data", "set_params", "set_gower", "fit", "fit_grad", "fit_predict", "append",
                                    "set_output_warp", "kernel_matrix"])
def test_whatever_changes_the_fit_drops_representers_and_belief(change):
    h, X, Y = _fresh()
    Xr, belief = _with_belief(h)
    before = h.es_acq()
    assert np.all(np.isfinite(before))
    if change == "set_data":
        h.set_data(X, Y)
    elif change == "set_params":
        h.set_params(gpo._lib.GP_KERNEL_RBF, 0, 1.0, np.array([0.5]), 1e-2)
    elif change == "set_gower":
        h.set_gower(None, None)
    elif change == "fit":
        h.fit()
    elif change == "fit_grad":
        h.fit_grad(1)
    elif change == "fit_predict":
        h.fit_predict()
    elif change == "append":
        h.append(np.array([[0.31, 0.77]]), np.vstack([Y, [[0.2]]]))
    elif change == "set_output_warp":
        h.set_output_warp(np.array([[1.0, 0.5, 0.1]]), 1.0)
        h.set_output_warp(None)
    elif change == "kernel_matrix":
        h.kernel_matrix()
    with pytest.raises(RuntimeError):        # no fit, or a fit without representers: never a score from the stale belief
        h.es_acq()
    h.fit()
    h.set_candidates(X[:9])
    with pytest.raises(RuntimeError, match="gp_es_set_representers"):
        h.es_acq()
    with pytest.raises(RuntimeError, match="gp_es_set_representers"):
        h.es_set_belief(*belief)
    Xr2, _ = _with_belief(h)
    assert np.all(np.isfinite(h.es_acq()))


def test_refused_beside_a_warp_a_sparse_fit_or_an_ensemble():
    h, X, Y = _fresh()
    h.set_output_warp(np.array([[1.0, 0.5, 0.1]]), 1.0)
    h.fit()
    with pytest.raises(RuntimeError, match="output warp"):
        h.es_set_representers(X[:3] + 0.01)
    h, X, Y = _fresh()
    _with_belief(h)
    h.sparse_set_inducing(X[:8])
    h.sparse_fit()
    with pytest.raises(RuntimeError, match="sparse"):
        h.es_acq()
    h, X, Y = _fresh()
    _with_belief(h)
    h.ens_fit(np.array([1.0, 1.2]), np.array([[0.5], [0.6]]), np.array([1e-2, 2e-2]))
    with pytest.raises(RuntimeError, match="ensemble"):
        h.es_acq()


# ---- the class --------------------------------------------------------------------------------------------------------------
class _FixedSampler(E.McmcSampler):
    def __init__(self, space, points):
        super().__init__(space)
        self.points = points

    def get_samples(self, n_samples, log_p_function, burn_in_steps=50):
        pts = self.points[:n_samples]
        return pts, np.array([float(np.ravel(log_p_function(p))[0]) for p in pts]).reshape(-1, 1)


def _gpmodel(N=30, normalizer=False):
    rng = np.random.default_rng(77)
    X = rng.uniform(0, 1, (N, 2))
    Y = np.sin(4 * X[:, :1]) + np.cos(3 * X[:, 1:]) + 0.05 * rng.standard_normal((N, 1))
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, variance=1.0, lengthscale=0.5), noise_var=1e-2, max_iters=0, verbose=False)
    gm.updateModel(X, Y, None, None)
    return gm, X, Y


def test_class_device_route_matches_its_host_twin():
    gm, X, Y = _gpmodel()
    space = gpo.Design_space([{"name": "x", "type": "continuous", "domain": (0.0, 1.0), "dimensionality": 2}])
    rng = np.random.default_rng(5)
    pts = np.vstack([rng.uniform(0, 1, (11, 2)), [[1.5, 0.5]]])        # the last one lies outside: log proposal -inf, removed
    kw = dict(num_samples=20, num_representer_points=12)
    dev = gpo.AcquisitionEntropySearch(gm, space, _FixedSampler(space, pts), **kw)
    host = gpo.AcquisitionEntropySearch(gm, space, _FixedSampler(space, pts), device=False, **kw)
    Xs = rng.uniform(0, 1, (40, 2))
    a, b = dev.acquisition_function(Xs), host.acquisition_function(Xs)
    assert dev.repr_points.shape == (11, 2) and host.repr_points.shape == (11, 2)
    fig = _rel(a, b)
    print("class, device against host route: %.2e (largest |value| %.3g)" % (fig, np.max(np.abs(b))))
    assert a.shape == (40, 1) and fig < 1e-9
    assert dev.argbest(Xs) == (int(np.argmin(a[:, 0])), float(a[:, 0].min()))
    idx, val = dev.topk(Xs, 3)
    assert idx.tolist() == np.argsort(a[:, 0], kind="stable")[:3].tolist()
    one = dev.acquisition_function(Xs[3])
    assert one.shape == (1, 1) and abs(one[0, 0] - a[3, 0]) <= 1e-9 * np.max(np.abs(a))     # (the fused rows route)
    # a changed fit renews representers and belief instead of scoring from the old ones
    seen = dev.logP.copy()
    gm.model.kern.lengthscale[:] = 0.3
    c = dev.acquisition_function(Xs)
    assert np.all(np.isfinite(c)) and not np.array_equal(seen, dev.logP)
    fig = _rel(c, host.acquisition_function(Xs))
    print("after new hyper-parameters: %.2e" % fig)
    assert fig < 1e-9


def test_bayesian_optimization_front_door():
    rng = np.random.default_rng(11)
    domain = [{"name": "x", "type": "continuous", "domain": (-1.0, 2.0)}, {"name": "y", "type": "continuous", "domain": (0.0, 1.0)}]
    X = np.c_[rng.uniform(-1, 2, 20), rng.uniform(0, 1, 20)]
    Y = (np.sin(3 * X[:, 0]) + (X[:, 1] - 0.3) ** 2)[:, None]
    bo = gpo.BayesianOptimization(f=None, domain=domain, X=X, Y=Y, acquisition_type="ES", num_representer_points=12,
                                  num_samples=20, burn_in_steps=5, sampler_seed=1, max_iters=0)
    assert isinstance(bo.acquisition, gpo.AcquisitionEntropySearch)
    x = np.atleast_2d(bo.suggest_next_locations())
    print("suggested", x)
    assert x.shape == (1, 2) and -1.0 <= x[0, 0] <= 2.0 and 0.0 <= x[0, 1] <= 1.0
