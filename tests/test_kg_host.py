"""CPU: the host logic of ``AcquisitionKG`` and the ``BayesianOptimization(acquisition_type='KG')`` wiring over a stub handle -- the
discretisation set (reproducible from the seed, inside the domain), the rows / table split and the signs, every refusal and its
message, the staleness key after a model update -- and what the package exports."""
import types

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib, knowledge_gradient
from gaussian_process_optimization_amd.acquisitions import _host_topk, _pick
from gaussian_process_optimization_amd.bayesian_optimization import InvalidConfigError

DOMAIN = [{"name": "x", "type": "continuous", "domain": (0.0, 1.0)}, {"name": "y", "type": "continuous", "domain": (-1.0, 2.0)}]
XTRAIN = np.array([[0.9, 1.5], [0.1, -0.5], [0.5, 0.5]])


class _StubHandle(object):
    """What AcquisitionKG asks of ``_lib.Handle`` and of its ``kg`` entries: KG is a bump 1 / (1 + |x - target|^2)."""
    kg = property(lambda self: self)

    def __init__(self, target=(0.3, 0.6)):
        self.target = np.asarray(target, dtype=float)
        self.kg_key, self.points, self.sets, self.calls, self.Xs = None, None, 0, [], None

    def set_points(self, Xa, y_mean=0.0, y_std=1.0, key=None):
        self.points, self.kg_key = np.array(Xa), key
        self.sets += 1
        self.calls.append(("set", Xa.shape, y_mean, y_std))
        return np.asarray(Xa).sum(1) * y_std + y_mean

    def info(self):
        return 0 if self.points is None else self.points.shape[0]

    def _kg(self, X):
        d = np.asarray(X, dtype=float) - self.target
        return 1.0 / (1.0 + (d * d).sum(1))

    def rows(self, Xs, y_std=1.0, grad=False):
        Xs = np.asarray(Xs, dtype=float)
        self.calls.append(("rows", Xs.shape, y_std, grad))
        v = self._kg(Xs)
        out = -v[:, None]
        return (out, 2.0 * (Xs - self.target) * (v * v)[:, None]) if grad else out

    def acq(self, y_std=1.0):
        self.calls.append(("acq", self.Xs.shape, y_std))
        return self._kg(self.Xs)[:, None]

    def acq_argbest(self, sense, y_std=1.0):
        self.calls.append(("argbest", sense, y_std))
        return _pick(self._kg(self.Xs), sense)

    def acq_topk(self, sense, k, y_std=1.0):
        self.calls.append(("topk", sense, k, y_std))
        return _host_topk(self._kg(self.Xs), k, sense)


def _model(**kw):
    gm = gpo.GPModel(max_iters=0, verbose=False, **kw)
    h = _StubHandle()
    gp = types.SimpleNamespace(output_dim=1, normalizer=None, kern=types.SimpleNamespace(Gower=False), _ensure_fit=lambda: None,
                               _h=h, X=XTRAIN, _data_epoch=0, param_array=np.array([1.0, 0.5, 0.01]))
    gp._stage = lambda x, fit=True: setattr(h, "Xs", np.array(x))
    gm.model = gp
    return gm


def _acq(num_points=8, seed=4, table=200, domain=DOMAIN, **kw):
    space = gpo.Design_space(domain)
    gm = _model()
    acq = gpo.AcquisitionKG(gm, space, gpo.AcquisitionOptimizer(space), num_points=num_points, kg_table_size=table,
                            sampler_seed=seed, **kw)
    # the posterior mean's ranking on the host (the device's gp_acq_topk / _argbest of LCB at weight 0 take its place): the
    # posterior mean is the coordinate sum
    acq._mean.topk = lambda X, k, sense=-1, devices=None: _host_topk(np.asarray(X).sum(1), k, sense)
    acq._mean.argbest = lambda X, sense=-1, devices=None: _pick(np.asarray(X).sum(1), sense)
    return acq, gm


def test_exports_and_constants():
    assert "AcquisitionKG" in gpo.__all__ and "knowledge_gradient" in gpo.__all__
    assert knowledge_gradient.AcquisitionKG is gpo.AcquisitionKG and gpo.AcquisitionKG.analytical_gradient_prediction is True
    assert _lib.GP_KG_MAX_A == 256
    names = ("set_points", "info", "acq", "acq_argbest", "acq_topk", "rows")
    for name in names:
        assert callable(getattr(_lib.KgEntries, name))
    assert {"gp_kg_" + n for n in names} <= {n for n, _, _ in _lib.SIGNATURES}
    assert _lib.Handle.kg_key is None and isinstance(_lib.Handle.kg, property)


def test_the_discretisation_set_is_deterministic_and_inside_the_domain():
    a, _ = _acq(num_points=10, seed=4)
    b, _ = _acq(num_points=10, seed=4)
    c, _ = _acq(num_points=10, seed=5)
    P = a.discretisation()
    assert P.shape == (10, 2) and np.array_equal(P, b.discretisation()) and np.array_equal(P, a.discretisation())
    assert not np.array_equal(P, c.discretisation())
    assert np.all(P[:, 0] >= 0.0) and np.all(P[:, 0] <= 1.0) and np.all(P[:, 1] >= -1.0) and np.all(P[:, 1] <= 2.0)
    rs = np.random.RandomState(4)
    table = gpo.Design_space(DOMAIN).samples_uniform(200, rs)
    low = table[np.argsort(table.sum(1), kind="stable")[:3]]             # ceil(10 / 4) lowest posterior means of the table, in order
    assert np.array_equal(P[:3], low)
    assert np.array_equal(P[3], XTRAIN[1])                               # the training input with the lowest posterior mean
    assert np.array_equal(P[4:], gpo.Design_space(DOMAIN).samples_uniform(6, rs))      # uniform draws of the same stream
    one, _ = _acq(num_points=1)
    assert one.discretisation().shape == (1, 2)
    few, _ = _acq(num_points=5, table=1)                                 # a table shorter than ceil(A / 4)
    assert few.discretisation().shape == (5, 2)


def test_rows_table_split_and_signs():
    acq, gm = _acq()
    h = gm.model._h
    X = np.random.RandomState(0).uniform(0, 1, (20, 2))
    v8 = acq.acquisition_function(X[:8])
    assert v8.shape == (8, 1) and np.allclose(v8[:, 0], -h._kg(X[:8]), rtol=1e-15)
    assert h.calls[0][0] == "set" and h.calls[-1] == ("rows", (8, 2), 1.0, False)
    v20 = acq.acquisition_function(X)
    assert v20.shape == (20, 1) and np.allclose(v20[:, 0], -h._kg(X), rtol=1e-15)      # the table's +KG negated
    assert h.calls[-1] == ("acq", (20, 2), 1.0) and np.array_equal(h.Xs, X)
    f, df = acq.acquisition_function_withGradients(X)
    assert f.shape == (20, 1) and df.shape == (20, 2) and np.allclose(f, v20, rtol=1e-15)
    assert [c[1] for c in h.calls[-3:]] == [(8, 2), (8, 2), (4, 2)] and all(c[3] for c in h.calls[-3:])     # groups of eight rows
    eps = 1e-6
    num = (acq.acquisition_function(X[:1] + [eps, 0])[0, 0] - acq.acquisition_function(X[:1] - [eps, 0])[0, 0]) / (2 * eps)
    assert abs(num - df[0, 0]) < 1e-8
    want = -h._kg(X)
    assert acq.argbest(X) == (int(np.argmin(want)), float(want.min())) and h.calls[-1] == ("argbest", 1, 1.0)
    assert acq.argbest(X, sense=+1) == (int(np.argmax(want)), float(want.max()))
    idx, val = acq.topk(X, 5)
    order = np.argsort(want, kind="stable")[:5]
    assert np.array_equal(idx, order) and np.allclose(val, want[order], rtol=1e-15)
    for call in (lambda: acq.argbest(X, devices=[0, 1]), lambda: acq.topk(X, 3, devices=[0, 1])):
        with pytest.raises(NotImplementedError, match="replica groups"):
            call()


def test_normaliser_reaches_the_calls():
    acq, gm = _acq()
    gm.model.normalizer = types.SimpleNamespace(mean=np.array([1.5]), std=np.array([2.0]))
    acq.acquisition_function(np.zeros((1, 2)))
    h = gm.model._h
    assert h.calls[0] == ("set", (8, 2), 1.5, 2.0) and h.calls[-1] == ("rows", (1, 2), 2.0, False)
    assert np.allclose(acq.points_mean, acq.points.sum(1) * 2.0 + 1.5)


def test_the_staleness_key_after_a_model_update():
    acq, gm = _acq()
    h = gm.model._h
    X = np.zeros((2, 2))
    assert acq.builds == 0 and acq.uploads == 0 and h.sets == 0          # built at the first call
    acq.acquisition_function(X)
    acq.acquisition_function_withGradients(X)
    assert (acq.builds, acq.uploads, h.sets) == (1, 1, 1) and h.kg_key == (id(acq), 1) and not acq.points.flags.writeable
    first = acq.points
    gm.model._data_epoch = 1                                             # new data: the set is rebuilt and sent
    acq.acquisition_function(X)
    assert (acq.builds, acq.uploads, h.sets) == (2, 2, 2) and h.kg_key == (id(acq), 2)
    assert np.array_equal(acq.points, first)                             # (the stub's posterior mean did not move: the same set)
    gm.model.param_array = np.array([1.0, 0.7, 0.01])                    # new hyper-parameters
    acq.acquisition_function(X)
    assert (acq.builds, acq.uploads) == (3, 3)
    h.points = None                                                      # the library dropped the points with a refit of its own
    acq.acquisition_function(X)
    assert (acq.builds, acq.uploads, h.sets) == (3, 4, 4)
    h2 = _StubHandle()                                                   # the model rebuilt its handle
    gm.model._h = h2
    acq.acquisition_function(X)
    acq.acquisition_function(X)
    assert (acq.builds, acq.uploads, h2.sets) == (3, 5, 1)
    h2.kg_key = ("someone", "else")                                      # another object's points took their place
    acq.acquisition_function(X)
    assert acq.uploads == 6 and h2.kg_key == (id(acq), 3)


def test_refused_models_and_options():
    space = gpo.Design_space(DOMAIN)
    style = "the knowledge gradient scores our exact GPModel with one output"
    with pytest.raises(NotImplementedError, match=style + ".*foreign, MCMC, warped or input-warped"):
        gpo.AcquisitionKG(object(), space)
    for foreign in (gpo.GPModel_MCMC(verbose=False), gpo.WarpedGPModel(verbose=False), gpo.InputWarpedGPModel(space, verbose=False)):
        with pytest.raises(NotImplementedError, match=style):
            gpo.AcquisitionKG(foreign, space)
    with pytest.raises(NotImplementedError, match=style + ".*sparse=True"):
        gpo.AcquisitionKG(gpo.GPModel(sparse=True, verbose=False), space)
    with pytest.raises(NotImplementedError, match=style + ".*Gower"):
        gpo.AcquisitionKG(gpo.GPModel(Gower=True, space=space, verbose=False), space)
    with pytest.raises(NotImplementedError, match=style + ".*mean function"):
        gpo.AcquisitionKG(gpo.GPModel(mean_function=gpo.mappings.Linear(2, 1), verbose=False), space)
    gm = _model()
    with pytest.raises(NotImplementedError, match="no cost model"):
        gpo.AcquisitionKG(gm, space, cost_withGradients=lambda x: (np.ones((x.shape[0], 1)), np.zeros(x.shape)))
    with pytest.raises(NotImplementedError, match="no black-box constraints"):
        gpo.AcquisitionKG(gm, space, feasibility=object())
    with pytest.raises(NotImplementedError, match="no black-box constraints"):
        gpo.AcquisitionKG(gm, space)._set_feasibility(object())
    with pytest.raises(NotImplementedError, match="not penalised"):
        gpo.AcquisitionLP(gm, space, None, gpo.AcquisitionKG(gm, space))
    for bad in (0, 257):
        with pytest.raises(ValueError, match="between 1 and 256 discretisation points"):
            gpo.AcquisitionKG(gm, space, num_points=bad)
    with pytest.raises(ValueError, match="kg_table_size"):
        gpo.AcquisitionKG(gm, space, kg_table_size=0)
    acq = gpo.AcquisitionKG(gm, space)
    gm.model.output_dim = 2
    with pytest.raises(NotImplementedError, match=style + ".*2 outputs"):
        acq.acquisition_function(np.zeros((1, 2)))
    gm.model.output_dim, gm.model.kern.Gower = 1, True
    with pytest.raises(NotImplementedError, match=style + ".*Gower"):
        acq.acquisition_function(np.zeros((1, 2)))
    gm.model = None
    with pytest.raises(RuntimeError, match="updateModel first"):
        acq.acquisition_function(np.zeros((1, 2)))


def test_front_door_wiring():
    X = np.random.RandomState(1).uniform(0, 1, (6, 2))
    Y = X.sum(1)[:, None]
    kw = dict(f=None, domain=DOMAIN, X=X, Y=Y, acquisition_type="KG")
    bo = gpo.BayesianOptimization(num_kg_points=16, kg_table_size=500, sampler_seed=2, parallel_anchors=True, **kw)
    acq = bo.acquisition
    assert isinstance(acq, gpo.AcquisitionKG) and bo.evaluator is None and acq.optimizer is bo.acquisition_optimizer
    assert (acq.num_points, acq.kg_table_size, acq.sampler_seed) == (16, 500, 2) and acq.analytical_gradient_acq
    assert bo.acquisition_optimizer.lockstep(acq.acquisition_function_withGradients)          # the lockstep optimiser takes it as it is
    bo = gpo.BayesianOptimization(**kw)
    assert (bo.acquisition.num_points, bo.acquisition.kg_table_size, bo.acquisition.sampler_seed) == (64, 10000, None)
    assert gpo.BayesianOptimization(evaluator_type="sequential", batch_size=3, **kw).evaluator is None
    for ev in ("local_penalization", "thompson_sampling", "random"):
        with pytest.raises(InvalidConfigError, match="one point at a time"):
            gpo.BayesianOptimization(evaluator_type=ev, batch_size=3, **kw)
    with pytest.raises(NotImplementedError, match="KG.*no black-box constraints"):
        gpo.BayesianOptimization(constraint_function=lambda x: x[:, :1] - 0.5, C=X[:, :1] - 0.5, **kw)
    with pytest.raises(NotImplementedError, match="no cost model"):
        gpo.BayesianOptimization(cost_withGradients=lambda x: (np.ones((x.shape[0], 1)), np.zeros(x.shape)), **kw)
    with pytest.raises(NotImplementedError, match="the knowledge gradient scores our exact GPModel"):
        gpo.BayesianOptimization(model_type="input_warped_GP", **kw)
    with pytest.raises(NotImplementedError, match="the knowledge gradient scores our exact GPModel"):
        gpo.BayesianOptimization(model=gpo.GPModel(sparse=True, verbose=False), **kw)
    cfg = dict(num_kg_points=12, kg_table_size=300, sampler_seed=7)
    made = gpo.AcquisitionKG.fromConfig(_model(), gpo.Design_space(DOMAIN), None, None, cfg)
    assert (made.num_points, made.kg_table_size, made.sampler_seed) == (12, 300, 7)
