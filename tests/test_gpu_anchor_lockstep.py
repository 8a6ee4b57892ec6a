"""GPU: the acquisition optimiser's anchors refined in lockstep (AcquisitionOptimizer(parallel=True), ThompsonBatch,
LocalPenalization, BayesianOptimization(parallel_anchors=True)) against the serial loop.  Each round of L-BFGS steps is ONE
gp_acq_rows call carrying the running anchors' points; a location's value and gradient do not depend on its company
(tests/test_gpu_rows_wide.py), so every anchor walks its serial path and the winner is the serial winner, bit for bit."""
import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import bayesian_optimization as bo
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

N, D = 300, 3
DOMAIN = [{'name': 'x%d' % d, 'type': 'continuous', 'domain': (0.0, 1.0)} for d in range(D)]


@pytest.fixture(scope="module")
def problem():
    X, Y, Xs = O.synthetic_problem(N, D, 8, seed=31)
    return X, Y, Xs


def _model(X, Y, kernel=None):
    gm = gpo.GPModel(kernel=kernel or gpo.kern.RBF(X.shape[1], 1.1, O.default_lengthscale(X.shape[1], False)), noise_var=1e-2,
                     max_iters=0, verbose=False)
    gm.updateModel(X, Y, None, None)
    return gm


def _acquisition(kind, gm, space, optimizer, Xs):
    if kind == "EI":
        return gpo.AcquisitionEI(gm, space, optimizer)
    if kind == "LCB":
        return gpo.AcquisitionLCB(gm, space, optimizer)
    lp = gpo.AcquisitionLP(gm, space, optimizer, gpo.AcquisitionEI(gm, space, optimizer))
    lp.update_batches(Xs[:2], 2.5, float(gm.model.Y.min()))        # a two-point batch
    return lp


@pytest.mark.parametrize("kind", ["EI", "LCB", "LP"])
def test_lockstep_returns_the_serial_optimum(problem, kind):
    X, Y, Xs = problem
    gm = _model(X, Y)
    space = gpo.Design_space(DOMAIN)
    got = []
    for parallel in (False, True):
        acq = _acquisition(kind, gm, space, bo.AcquisitionOptimizer(space, parallel=parallel), Xs)
        assert acq.analytical_gradient_acq
        np.random.seed(17)
        got.append(acq.optimize())
    (xs, fs), (xp, fp) = got
    assert xs.shape == (1, D) and np.array_equal(xs, xp) and fs == fp
    gm.model.close()


def test_lockstep_makes_no_more_calls_than_its_longest_anchor(problem):
    """gp_acq_rows calls (gp_rows_stats): a lockstep run makes one per round, so at most as many as the longest serial anchor
    run, plus the one that scores the rounded optima; and every round with five to eight anchors running is ONE wide pass."""
    X, Y, Xs = problem
    gm = _model(X, Y)
    space = gpo.Design_space(DOMAIN)
    acq = gpo.AcquisitionEI(gm, space, bo.AcquisitionOptimizer(space, parallel=True))
    f, f_df = acq.acquisition_function, acq.acquisition_function_withGradients
    h = gm.model._h
    np.random.seed(23)
    S = space.samples_uniform(1000)
    anchors = S[np.argsort(f(S).flatten())[:5]]
    per_anchor = []
    for a in anchors:
        c0 = h.rows_stats()["fused"]
        bo._lbfgs_from_anchor(space, a, f, f_df)
        per_anchor.append(h.rows_stats()["fused"] - c0)
    c0, p0 = h.rows_stats(), h.rows_pass_stats()
    np.random.seed(23)
    acq.optimize()
    c1, p1 = h.rows_stats(), h.rows_pass_stats()
    calls = c1["fused"] - c0["fused"]
    print("gp_acq_rows calls per serial anchor", per_anchor, "in lockstep", calls)
    assert c1["fallback"] == c0["fallback"]
    assert calls <= max(per_anchor) + 1 and calls < sum(per_anchor)
    assert p1["wide"] - p0["wide"] >= 2 and (p1["wide"] - p0["wide"]) + (p1["narrow"] - p0["narrow"]) == calls      # one pass per call
    gm.model.close()


@pytest.mark.parametrize("evaluator", ["local_penalization", "thompson_sampling"])
def test_batch_evaluators_suggest_the_serial_batch(problem, evaluator):
    X, Y, Xs = problem
    got = []
    for parallel in (False, True):
        opt = gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, evaluator_type=evaluator, batch_size=3, normalize_Y=False,
                                       kernel=gpo.kern.RBF(D, 1.1, O.default_lengthscale(D, False)), noise_var=1e-2, max_iters=0,
                                       parallel_anchors=parallel)
        assert opt.acquisition_optimizer.parallel is parallel
        np.random.seed(5)
        got.append(opt.suggest_next_locations())
        opt.model.model.close()
    assert got[0].shape == (3, D) and np.array_equal(got[0], got[1])


def test_mixed_space_rounds_each_anchor(problem):
    """One discrete variable: round_optimum is applied to every anchor's optimum before the rounded points are scored."""
    dom = [{'name': 'k', 'type': 'discrete', 'domain': (0.0, 0.25, 0.5, 1.0)}] + DOMAIN[1:]
    space = gpo.Design_space(dom)
    X, Y, Xs = problem
    X = X.copy()
    X[:, 0] = np.asarray(dom[0]['domain'])[np.random.default_rng(2).integers(0, 4, N)]
    gm = _model(X, Y)
    got = []
    for parallel in (False, True):
        acq = gpo.AcquisitionEI(gm, space, bo.AcquisitionOptimizer(space, parallel=parallel))
        np.random.seed(41)
        got.append(acq.optimize())
    (xs, fs), (xp, fp) = got
    assert xs[0, 0] in dom[0]['domain'] and np.array_equal(xs, xp) and fs == fp
    gm.model.close()
