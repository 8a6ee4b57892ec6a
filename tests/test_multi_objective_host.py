"""CPU: multi_objective.py -- the Pareto front, the hypervolume, the cell decomposition, the host rule of ``AcquisitionEHVI`` over
stub models, the refusals and the bookkeeping of ``MultiObjectiveBayesianOptimization``.  Nothing needs a GPU."""
import types

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import multi_objective as MO

import _ehvi_truth as ET


def _hv_exact(P, ref):
    """Inclusion-exclusion over the points: shares nothing with the sweeps of multi_objective.hypervolume."""
    ref = np.asarray(ref, dtype=float)
    P = [p for p in np.asarray(P, dtype=float).reshape(-1, ref.size) if np.all(p < ref)]
    total = 0.0
    for mask in range(1, 1 << len(P)):
        sub = [P[i] for i in range(len(P)) if mask >> i & 1]
        total += (-1) ** (len(sub) + 1) * np.prod(ref - np.max(sub, axis=0))
    return total


class StubModel(object):
    """An objective GP with an analytic posterior: mean sin(x . w) + shift, variance 0.05 + |x|^2 / 4."""

    def __init__(self, w, shift=0.0):
        self.w, self.shift, self.model, self.device = np.asarray(w, dtype=float), shift, None, 0

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        self.model = types.SimpleNamespace(X=np.array(X_all, dtype=float), Y=np.array(Y_all, dtype=float))

    def posterior(self, x):
        x = np.atleast_2d(x)
        return np.sin(x @ self.w) + self.shift, 0.05 + 0.25 * (x ** 2).sum(1), np.cos(x @ self.w)[:, None] * self.w, 0.5 * x

    def predict_withGradients(self, x):
        mean, var, dm, dv = self.posterior(x)
        sd = np.sqrt(var)
        return mean[:, None], sd[:, None], dm, dv / (2 * sd[:, None])


def test_pareto_front_and_hypervolume_on_hand_made_fronts():
    assert gpo.multi_objective is MO and gpo.pareto_front is MO.pareto_front and gpo.hypervolume is MO.hypervolume
    Y = np.array([[0.2, 0.5], [0.5, 0.2], [0.5, 0.5], [0.2, 0.5], [0.1, 0.9], [0.6, 0.6]])
    F, rows = MO.pareto_front(Y, return_index=True)
    assert np.array_equal(F, [[0.1, 0.9], [0.2, 0.5], [0.5, 0.2]]) and np.array_equal(Y[rows], F)
    assert MO.hypervolume(Y, [1.0, 1.0]) == pytest.approx(0.9 * 0.1 + 0.8 * 0.4 + 0.5 * 0.3)
    assert MO.hypervolume(Y, [0.4, 0.8]) == pytest.approx(0.2 * 0.3)          # the other front points lie beyond this reference
    assert MO.hypervolume(np.empty((0, 2)), [1.0, 1.0]) == 0.0 and MO.pareto_front(np.empty((0, 3))).shape == (0, 3)
    Y3 = np.array([[0.0, 0.0, 0.5], [0.5, 0.5, 0.0], [0.6, 0.6, 0.6], [0.0, 0.0, 0.5]])
    assert np.array_equal(MO.pareto_front(Y3), [[0.0, 0.0, 0.5], [0.5, 0.5, 0.0]])
    assert MO.hypervolume(Y3, [1.0, 1.0, 1.0]) == pytest.approx(0.5 + 0.25 * 0.5)   # the box of point 0, and point 1's slab below it
    for bad in (np.zeros((3, 1)), np.zeros((3, 4))):
        with pytest.raises(ValueError):
            MO.pareto_front(bad)
    with pytest.raises(ValueError):
        MO.hypervolume(Y, [1.0, np.inf])


@pytest.mark.parametrize("K", [2, 3])
def test_cells_against_exact_hypervolume_differences(K):
    rng = np.random.default_rng(40 + K)
    ref = np.full(K, 0.85)
    worst, most = 0.0, 0
    for trial in range(40):
        n = int(rng.integers(0, 7))
        Y = rng.uniform(0, 1, (n, K))                   # some rows lie beyond the reference point
        if trial % 3 == 1:
            Y = np.round(Y, 1)                          # ties on every axis
        if trial % 3 == 2 and n > 1:
            Y[-1] = Y[0]                                # a duplicate
        levels, lo, hi = MO.nondominated_cells(Y, ref)
        F = MO.pareto_front(Y[np.all(Y < ref, axis=1)])
        assert lo.shape == hi.shape and lo.shape[1] == K and np.all(lo < hi) and np.all(lo >= 0)
        assert lo.shape[0] <= (len(F) + 1) * (len(F) + 2) // 2 if K == 3 else lo.shape[0] == len(F) + 1
        for k in range(K):
            assert levels[k][0] == -np.inf and levels[k][-1] == ref[k] and np.all(np.diff(levels[k]) > 0)
            assert np.array_equal(levels[k][1:-1], np.unique(F[:, k])) and np.all(hi[:, k] < levels[k].size)
        t_levels, t_lo, t_hi = ET.cells_of(Y, ref)      # the truth's own construction: the same cells
        assert all(np.array_equal(a, b) for a, b in zip(levels, t_levels)) and np.array_equal(lo, t_lo) and np.array_equal(hi, t_hi)
        base = _hv_exact(Y, ref)
        assert MO.hypervolume(Y, ref) == pytest.approx(base, abs=1e-14)
        for y in rng.uniform(-0.2, 1.1, (6, K)):
            gain = _hv_exact(np.vstack((Y, y)), ref) - base
            worst = max(worst, abs(MO.hypervolume_improvement_from_cells(y, levels, lo, hi) - gain))
        most = max(most, lo.shape[0])
    print("cells K=%d: worst difference to the exact hypervolume gain %.3g over 240 outcomes, up to %d cells" % (K, worst, most))
    assert worst <= 1e-14


def test_cells_of_an_empty_front_and_the_caps(monkeypatch):
    for K in (2, 3):
        levels, lo, hi = MO.nondominated_cells(np.empty((0, K)), np.ones(K))
        assert lo.tolist() == [[0] * K] and hi.tolist() == [[1] * K] and all(l.tolist() == [-np.inf, 1.0] for l in levels)
        levels, lo, hi = MO.nondominated_cells(np.full((2, K), 2.0), np.ones(K))     # every row beyond the reference point
        assert lo.shape == (1, K)
    t = np.linspace(0.0, 1.0, MO.MAX_FRONT_VALUES + 1)
    with pytest.raises(ValueError, match="GP_EHVI_MAX_LEVELS"):
        MO.nondominated_cells(np.stack((t, 1.0 - t), axis=1), [2.0, 2.0])
    levels, lo, hi = MO.nondominated_cells(np.stack((t[:-1], 1.0 - t[:-1]), axis=1), [2.0, 2.0])
    assert levels[0].size == _lib.GP_EHVI_MAX_LEVELS and lo.shape[0] == MO.MAX_FRONT_VALUES + 1
    # K = 3, the most cells a front within the level cap can have: every slab keeps all the points below it, (n + 1)(n + 2) / 2
    # cells -- 32640 at n = 254, within GP_EHVI_MAX_CELLS; the cell cap itself is reached only by a smaller one
    n = MO.MAX_FRONT_VALUES
    big = np.stack((t[:n], 1.0 - t[:n] ** 0.5, np.linspace(1.0, 0.0, n)), axis=1)
    levels, lo, hi = MO.nondominated_cells(big, [2.0, 2.0, 2.0])
    assert lo.shape[0] == (n + 1) * (n + 2) // 2 <= MO.MAX_CELLS and np.all(lo < hi)
    monkeypatch.setattr(MO, "MAX_CELLS", 100)
    with pytest.raises(ValueError, match="GP_EHVI_MAX_CELLS"):
        MO.nondominated_cells(big[:20], [2.0, 2.0, 2.0])
    assert MO.nondominated_cells(big[:12], [2.0, 2.0, 2.0])[1].shape[0] == 91


def _acq(K, ref, **kw):
    models = [StubModel([0.7, -0.4], 0.1), StubModel([-0.3, 0.9], -0.2), StubModel([0.5, 0.5], 0.3)][:K]
    return MO.AcquisitionEHVI(models, reference_point=ref, **kw), models


@pytest.mark.parametrize("K", [2, 3])
def test_host_rule_against_the_truth(K):
    rng = np.random.default_rng(7 + K)
    acq, models = _acq(K, np.full(K, 1.4))
    assert acq.device_pack() is None                                # foreign models: the host formulas
    Y = rng.normal(0.2, 0.6, (9, K))
    y_mean, y_std = rng.normal(0, 0.2, K), rng.uniform(0.7, 1.5, K)
    gen = acq.generation
    acq.set_front(Y, y_mean, y_std)
    assert acq.generation == gen + 1
    x = rng.uniform(0, 1, (6, 2))
    f, df = acq.acquisition_function_withGradients(x)
    assert f.shape == (6, 1) and df.shape == (6, 2) and np.array_equal(acq.acquisition_function(x), f)
    assert np.array_equal(acq.acquisition_function(x, host=True), f)
    post = [np.stack(a) for a in zip(*[m.posterior(x) for m in models])]
    levels, lo, hi = ET.cells_of(Y, acq.reference_point)
    t = ET.ehvi(*post, y_mean, y_std, levels, lo, hi)
    # float64 NumPy against the long-double truth: the bound derived for the device's float64 evaluation, with a factor for
    # NumPy's different order of the same operations
    assert np.all(np.abs(-f[:, 0] - t.value) <= 4 * t.bound_value)
    assert np.all(np.abs(-df - t.grad) <= 4 * t.bound_grad)
    assert np.all(f <= 0)
    v = f[:, 0]
    assert acq.argbest(x, -1) == (int(np.argmin(v)), v.min())
    masked = np.where(np.arange(6) == int(np.argmin(v)), np.inf, v)
    assert acq.argbest(x, -1, exclude=(int(np.argmin(v)),))[0] == int(np.argmin(masked))
    idx, val = acq.topk(x, 3, -1)
    assert list(idx) == list(np.argsort(v, kind="stable")[:3]) and np.array_equal(val, v[idx])
    # an outcome that cannot improve the front: far beyond the reference point in every objective
    far, _ = _acq(K, np.full(K, -50.0))
    assert np.all(np.abs(far.acquisition_function(x)) < 1e-300)


def test_refusals():
    K, ref = 2, np.ones(2)
    models = [StubModel([1.0, 0.0]), StubModel([0.0, 1.0])]
    with pytest.raises(NotImplementedError, match="cost"):
        MO.AcquisitionEHVI(models, reference_point=ref, cost_withGradients=lambda x: (np.ones((len(x), 1)), np.zeros_like(x)))
    with pytest.raises(NotImplementedError, match="constraints"):
        MO.AcquisitionEHVI(models, reference_point=ref, feasibility=object())
    acq = MO.AcquisitionEHVI(models, reference_point=ref)
    with pytest.raises(NotImplementedError, match="penalised"):
        gpo.AcquisitionLP(models[0], acquisition=acq)
    with pytest.raises(NotImplementedError):
        acq.argbest(np.zeros((3, 2)), devices=[0, 1])
    for bad in ([models[0]], models * 2):
        with pytest.raises(ValueError):
            MO.AcquisitionEHVI(bad, reference_point=np.ones(len(bad)))
    with pytest.raises(ValueError):
        MO.AcquisitionEHVI(models, reference_point=[1.0, np.nan])
    with pytest.raises(ValueError):
        MO.AcquisitionEHVI(models)
    dom = [{"name": "x", "type": "continuous", "domain": (0, 1), "dimensionality": 2}]
    f = lambda x: np.atleast_2d(x)
    X = np.random.default_rng(0).uniform(0, 1, (4, 2))
    for kw in (dict(cost_withGradients="evaluation_time"), dict(constraint_function=f), dict(evaluator_type="local_penalization"),
               dict(batch_size=2)):
        with pytest.raises(NotImplementedError):
            gpo.MultiObjectiveBayesianOptimization(f, dom, 2, X=X, models=models, **kw)
    for K in (1, 4):
        with pytest.raises(ValueError):
            gpo.MultiObjectiveBayesianOptimization(f, dom, K, X=X, models=models)


def test_bookkeeping_of_the_loop_over_stub_models():
    dom = [{"name": "x", "type": "continuous", "domain": (0, 1), "dimensionality": 2}]
    f = lambda x: np.stack((np.atleast_2d(x)[:, 0] ** 2, (np.atleast_2d(x)[:, 1] - 1.0) ** 2 + np.atleast_2d(x)[:, 0]), axis=1)
    X = np.random.default_rng(1).uniform(0, 1, (6, 2))
    models = [StubModel([1.0, 0.0]), StubModel([0.0, 1.0])]
    np.random.seed(0)
    bo = gpo.MultiObjectiveBayesianOptimization(f, dom, 2, X=X, models=models)
    Y = f(X)
    assert np.allclose(bo.reference_point, Y.max(0) + 0.1 * (Y.max(0) - Y.min(0)))       # the default reference point
    assert np.array_equal(bo.Y, Y) and bo.hypervolume == pytest.approx(_hv_exact(Y, bo.reference_point))
    assert np.array_equal(bo.pareto_Y, MO.pareto_front(Y)) and np.array_equal(f(bo.pareto_X), bo.pareto_Y)
    x = bo.suggest_next_locations()
    assert x.shape == (1, 2) and np.all(x >= 0) and np.all(x <= 1)
    for k, m in enumerate(models):                                  # fitted on the column standardised
        assert np.allclose(m.model.Y[:, 0], (Y[:, k] - Y[:, k].mean()) / Y[:, k].std())
    assert np.allclose(bo.acquisition.y_mean, Y.mean(0)) and np.allclose(bo.acquisition.y_std, Y.std(0))
    ref = bo.reference_point.copy()
    bo.run_optimization(max_iter=2)
    assert bo.X.shape == (8, 2) and bo.Y.shape == (8, 2) and np.array_equal(bo.reference_point, ref)    # fixed from then on
    fixed = gpo.MultiObjectiveBayesianOptimization(f, dom, 2, X=X, models=models, reference_point=[0.5, 0.9])
    inside = np.all(Y < [0.5, 0.9], axis=1)
    assert np.array_equal(fixed.pareto_Y, MO.pareto_front(Y[inside]))     # observations beyond it are left out of the front
    assert fixed.Y.shape[0] == 6                                           # ... and stay in the data
