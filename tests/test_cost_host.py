"""CPU: ``CostModel`` (cost.py), the predicates that decide where a cost is divided (acquisitions.py) and the evaluation-time
bookkeeping of ``BayesianOptimization`` -- with stub models: nothing here needs a GPU."""
import types

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import acquisitions as A
from gaussian_process_optimization_amd import bayesian_optimization as B
from gaussian_process_optimization_amd import cost as C


class StubModel(object):
    """A cost GP that remembers its data: posterior mean m(x) = 0.3 + x . w, so that dm/dx = w."""
    w = np.array([0.5, -0.25])

    def __init__(self, **kw):
        self.kw, self.model, self.updates = kw, None, 0

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        self.model = types.SimpleNamespace(X=np.array(X_all, dtype=float), Y=np.array(Y_all, dtype=float))
        self.updates += 1

    def predict_withGradients(self, x):
        x = np.atleast_2d(x)
        m = 0.3 + x @ self.w[:, None]
        return m, np.ones_like(m), np.tile(self.w, (x.shape[0], 1)), np.zeros_like(x)


@pytest.fixture
def stub_cost_gp(monkeypatch):
    monkeypatch.setattr(C, "GPModel", StubModel)


def test_constant_cost_is_one_function_object():
    assert A.constant_cost_withGradients is C.constant_cost_withGradients
    assert gpo.CostModel is C.CostModel and gpo.cost is C
    cm = gpo.CostModel(None)
    assert cm.cost_withGradients is C.constant_cost_withGradients and cm.cost_type == 'Constant cost'
    price, dprice = cm.cost_withGradients(np.zeros((3, 2)))
    assert np.array_equal(price, np.ones((3, 1))) and np.array_equal(dprice, np.zeros((3, 2)))
    cm.update_cost_model(np.zeros((2, 2)), [1.0, 2.0])                      # a no-op for this kind
    assert cm.generation == 0

    def mine(x):
        return 2 * np.ones((x.shape[0], 1)), np.zeros(x.shape)
    cm = gpo.CostModel(mine)
    assert cm.cost_withGradients is mine and cm.cost_type == 'Used defined cost'
    cm.update_cost_model(np.zeros((2, 2)), [1.0, 2.0])
    assert cm.generation == 0 and not hasattr(cm, "cost_model")


def test_evaluation_time_cost_model(stub_cost_gp):
    cm = gpo.CostModel('evaluation_time', device=3)
    assert isinstance(cm.cost_model, StubModel) and cm.cost_model.kw == dict(device=3)
    assert cm.cost_type == 'evaluation_time' and cm.num_updates == 0 and cm.generation == 0
    assert cm.cost_withGradients.__self__ is cm and cm.cost_withGradients.__func__ is C.CostModel._cost_gp_withGradients
    x = np.array([[0.2, 0.4], [1.0, 0.0], [0.5, 0.5]])
    price, dprice = cm.cost_withGradients(x)                                # before the first update: the constant cost
    assert np.array_equal(price, np.ones((3, 1))) and np.array_equal(dprice, np.zeros((3, 2)))
    X1, c1 = np.array([[0.1, 0.2], [0.3, 0.4]]), [2.0, 0.5]
    cm.update_cost_model(X1, c1)
    assert cm.num_updates == 1 and cm.generation == 1
    assert np.array_equal(cm.cost_model.model.X, X1) and np.array_equal(cm.cost_model.model.Y, np.log([[2.0], [0.5]]))
    X2, c2 = np.array([[0.9, 0.8]]), [4.0]
    cm.update_cost_model(X2, c2)                                            # the data accumulate by vstack
    assert cm.num_updates == 2 and cm.generation == 2 and cm.cost_model.updates == 2
    assert np.array_equal(cm.cost_model.model.X, np.vstack((X1, X2)))
    assert np.array_equal(cm.cost_model.model.Y, np.log([[2.0], [0.5], [4.0]]))
    price, dprice = cm.cost_withGradients(x)
    m = 0.3 + x @ StubModel.w[:, None]
    assert np.array_equal(price, np.exp(m)) and np.array_equal(dprice, np.exp(m) * StubModel.w)
    assert np.array_equal(cm._cost_gp(x), np.exp(m))


# ---- the predicates -------------------------------------------------------------------------------------------------------------------
def _fitted_exact(device=0, **kw):
    """A GPModel that looks fitted without a device behind it: one output, a Euclidean kernel."""
    gm = gpo.GPModel(device=device, verbose=False, **kw)
    gm.model = types.SimpleNamespace(output_dim=1, kern=types.SimpleNamespace(_kernel_id=_lib.GP_KERNEL_MATERN52, Gower=False))
    return gm


def _device_cost_model(cost_gp=None):
    cm = gpo.CostModel('evaluation_time')
    cm.cost_model = _fitted_exact() if cost_gp is None else cost_gp
    cm.num_updates = cm.generation = 1
    return cm


class _Constrained(object):
    def has_constraints(self):
        return True

    def indicator_constraints(self, x):
        return np.ones((np.atleast_2d(x).shape[0], 1))


def test_device_cost_predicate():
    gm, cm = _fitted_exact(), _device_cost_model()
    for cls in (gpo.AcquisitionEI, gpo.AcquisitionMPI):
        acq = cls(gm, cost_withGradients=cm.cost_withGradients)
        assert A._device_cost(acq) is cm and acq._device_ok() and acq._per_cost and acq._route() is A._EXACT
        assert acq._acq_id == acq._rule.device_id | _lib.GP_ACQ_PER_COST
        assert not A._unit_cost_unconstrained(acq)                         # (the unit-cost predicate is what it was)
    unit = gpo.AcquisitionEI(gm)
    assert unit._device_ok() and not unit._per_cost and unit._acq_id == _lib.GP_ACQ_EI and A._device_cost(unit) is None
    # a user's function keeps the host rule, whatever it computes; so does a constrained space, with either cost
    wrapped = gpo.AcquisitionEI(gm, cost_withGradients=lambda x: cm.cost_withGradients(x))
    assert not wrapped._device_ok() and not wrapped._sparse_device_ok() and wrapped._route() is None and not wrapped._per_cost
    assert wrapped._acq_id == _lib.GP_ACQ_EI
    for cost in (None, cm.cost_withGradients):
        held = gpo.AcquisitionEI(gm, space=_Constrained(), cost_withGradients=cost)
        assert not held._device_ok() and held._route() is None
    # the cost model's own conditions
    unfitted = gpo.CostModel('evaluation_time')
    assert A._device_cost(gpo.AcquisitionEI(gm, cost_withGradients=unfitted.cost_withGradients)) is None
    foreign = _device_cost_model(StubModel())
    foreign.cost_model.model = object()
    sparse = _device_cost_model(_fitted_exact(sparse=True))
    gower = _device_cost_model(_fitted_exact(Gower=True, space=object()))
    elsewhere = _device_cost_model(_fitted_exact(device=1))
    two_outputs = _device_cost_model()
    two_outputs.cost_model.model.output_dim = 2
    for bad in (foreign, sparse, gower, elsewhere, two_outputs):
        acq = gpo.AcquisitionEI(gm, cost_withGradients=bad.cost_withGradients)
        assert A._device_cost(acq) is None and not acq._device_ok() and acq._route() is None and not acq._per_cost
    # the sparse route and the integrated acquisitions accept the same two costs
    sm = _fitted_exact(sparse=True, device_acquisitions=True)
    acq = gpo.AcquisitionEI(sm, cost_withGradients=cm.cost_withGradients)
    assert acq._sparse_device_ok() and acq._route() is A._SPARSE and acq._per_cost
    assert not gpo.AcquisitionEI(sm, cost_withGradients=lambda x: cm.cost_withGradients(x))._sparse_device_ok()
    mm = gpo.GPModel_MCMC()
    mm.model, mm.hmc_samples = object(), np.ones((2, 3))
    for cls in (gpo.AcquisitionEI_MCMC, gpo.AcquisitionMPI_MCMC):
        assert cls(mm, cost_withGradients=cm.cost_withGradients)._ens_ok() and cls(mm, cost_withGradients=cm.cost_withGradients)._per_cost
        assert not cls(mm, cost_withGradients=lambda x: cm.cost_withGradients(x))._ens_ok()
        assert not cls(mm, space=_Constrained(), cost_withGradients=cm.cost_withGradients)._ens_ok()


def test_lcb_and_lp_never_carry_the_flag(capsys):
    gm, cm = _fitted_exact(), _device_cost_model()
    lcb = gpo.AcquisitionLCB(gm, cost_withGradients=cm.cost_withGradients)
    assert lcb.cost_withGradients is C.constant_cost_withGradients and not lcb._per_cost and lcb._acq_id == _lib.GP_ACQ_LCB
    mm = gpo.GPModel_MCMC()
    mm.model, mm.hmc_samples = object(), np.ones((2, 3))
    lcbi = gpo.AcquisitionLCB_MCMC(mm, cost_withGradients=cm.cost_withGradients)
    assert not lcbi._per_cost and lcbi._acq_id == _lib.GP_ACQ_LCB
    base = gpo.AcquisitionEI(gm, cost_withGradients=cm.cost_withGradients)
    lp = gpo.AcquisitionLP(gm, acquisition=base)
    assert base._per_cost and lp._lp_route() is None and not lp._lp_device_ok() and not lp._lp_sparse_ok()
    assert not lp._per_cost and lp._acq_id is None
    plain = gpo.AcquisitionLP(gm, acquisition=gpo.AcquisitionEI(gm))
    assert plain._lp_route() is A._EXACT                                    # without a cost: the device, as before


# ---- BayesianOptimization under 'evaluation_time' ---------------------------------------------------------------------------------------
DOMAIN = [{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}]


class _Clock(object):
    """Every reading is later than the one before by 1, 2, 3, ... seconds."""

    def __init__(self):
        self.now, self.step = 100.0, 0

    def __call__(self):
        self.step += 1
        self.now += self.step
        return self.now


def test_bayesian_optimization_times_the_initial_design(stub_cost_gp, monkeypatch):
    clock = _Clock()
    monkeypatch.setattr(B, "_clock", clock)
    seen = []

    def f(x):
        seen.append(np.array(x))
        return np.sum(np.square(x), axis=1, keepdims=True)

    np.random.seed(1)
    bo = gpo.BayesianOptimization(f, DOMAIN, cost_withGradients='evaluation_time', initial_design_numdata=4)
    assert isinstance(bo.cost, gpo.CostModel) and bo.cost.cost_type == 'evaluation_time'
    assert bo.acquisition.cost_withGradients == bo.cost.cost_withGradients
    assert len(seen) == 4 and all(s.shape == (1, 2) for s in seen)          # one row at a time
    assert np.array_equal(np.vstack(seen), bo.X) and np.array_equal(bo.Y, np.sum(np.square(bo.X), axis=1, keepdims=True))
    # the k-th evaluation lies between readings 2k - 1 and 2k of the clock: it lasted 2k seconds
    gp = bo.cost.cost_model
    assert bo.cost.num_updates == 1 and bo.cost.generation == 1
    assert np.array_equal(gp.model.X, bo.X) and np.array_equal(gp.model.Y, np.log([[2.0], [4.0], [6.0], [8.0]]))
    # a later evaluation that is recorded goes under them
    y = bo._evaluate(np.array([[0.5, 0.5], [0.25, 0.75]]), record_cost=True)
    assert y.shape == (2, 1) and len(seen) == 6 and bo.cost.generation == 2
    assert np.array_equal(gp.model.Y[4:], np.log([[10.0], [12.0]])) and gp.model.X.shape == (6, 2)


def test_bayesian_optimization_other_costs_evaluate_as_before(stub_cost_gp):
    shapes = []

    def f(x):
        shapes.append(x.shape)
        return np.sum(x, axis=1, keepdims=True)

    def mine(x):
        return np.ones((x.shape[0], 1)), np.zeros(x.shape)

    for cost in (None, mine):
        del shapes[:]
        bo = gpo.BayesianOptimization(f, DOMAIN, cost_withGradients=cost, initial_design_numdata=3)
        assert shapes == [(3, 2)]                                           # the whole design in one call
        assert bo.acquisition.cost_withGradients is (C.constant_cost_withGradients if cost is None else mine)
        assert bo.cost.cost_withGradients is bo.acquisition.cost_withGradients


def test_bayesian_optimization_without_f_is_fed_its_costs(stub_cost_gp):
    X = np.random.RandomState(0).uniform(0, 1, (5, 2))
    bo = gpo.BayesianOptimization(None, DOMAIN, X=X, Y=np.sum(X, axis=1, keepdims=True), cost_withGradients='evaluation_time')
    assert bo.cost.num_updates == 0
    bo.cost.update_cost_model(X, [1.0, 2.0, 3.0, 4.0, 5.0])
    assert bo.cost.generation == 1 and np.array_equal(bo.cost.cost_model.model.Y[:, 0], np.log([1.0, 2.0, 3.0, 4.0, 5.0]))
