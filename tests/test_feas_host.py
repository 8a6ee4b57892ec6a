"""CPU: ``FeasibilityModel`` (feasibility.py), the acquisition classes over it (acquisitions.py) and the constraint bookkeeping of
``BayesianOptimization`` -- over stand-ins for the models and for the handle that only record their calls: nothing needs a GPU."""
import types

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import acquisitions as A
from gaussian_process_optimization_amd import bayesian_optimization as B
from gaussian_process_optimization_amd import feasibility as F

import _feas_truth as FT

FEAS = _lib.GP_ACQ_TIMES_FEAS


class StubModel(object):
    """A constraint GP with an analytic posterior: mean sin(x . w), variance 0.05 + |x|^2."""

    def __init__(self, **kw):
        self.kw, self.model, self.updates, self.device = kw, None, 0, kw.get("device", 0)
        self.w = np.array([0.7, -0.4])

    def updateModel(self, X_all, Y_all, X_new, Y_new):
        self.model = types.SimpleNamespace(X=np.array(X_all, dtype=float), Y=np.array(Y_all, dtype=float))
        self.updates += 1

    def posterior(self, x):
        x = np.atleast_2d(x)
        mean, var = np.sin(x @ self.w), 0.05 + (x ** 2).sum(1)
        return mean, var, np.cos(x @ self.w)[:, None] * self.w, 2 * x

    def predict_withGradients(self, x):
        mean, var, dm, dv = self.posterior(x)
        sd = np.sqrt(var)
        return mean[:, None], sd[:, None], dm, dv / (2 * sd[:, None])


@pytest.fixture
def stub_gps(monkeypatch):
    monkeypatch.setattr(F, "GPModel", StubModel)


X0 = np.array([[0.1, 0.2], [0.8, 0.4], [0.5, 0.5], [0.3, 0.9], [0.6, 0.1]])
C0 = np.array([[-1.0, 0.5], [0.2, -0.3], [-0.1, -2.0], [0.0, 0.0], [3.0, 1.0]])


def test_feasibility_model_on_the_host(stub_gps):
    assert gpo.FeasibilityModel is F.FeasibilityModel and gpo.feasibility is F
    fm = gpo.FeasibilityModel(2, bounds=[0.0, 0.1], device=3, max_iters=0)
    assert [m.kw for m in fm.models] == [dict(device=3, max_iters=0)] * 2 and fm.generation == 0
    with pytest.raises(RuntimeError):
        fm.log_probability(X0)
    assert np.array_equal(fm.feasible(C0), [False, False, True, True, False])
    fm.update(X0, C0)
    assert fm.generation == 1 and np.array_equal(fm.feasible_rows, [2, 3]) and fm.num_rows == 5
    assert np.allclose(fm.c_mean, C0.mean(0)) and np.allclose(fm.c_std, C0.std(0))
    for k, m in enumerate(fm.models):
        assert np.array_equal(m.model.X, X0) and np.allclose(m.model.Y[:, 0], (C0[:, k] - C0[:, k].mean()) / C0[:, k].std())
    assert fm.device_pack() is None                                # foreign models: the host formulas
    x = np.random.default_rng(0).uniform(0, 1, (6, 2))
    logF, dlogF = fm.log_probability_withGradients(x)
    post = [np.stack(a) for a in zip(*[m.posterior(x) for m in fm.models])]
    f = FT.fold(*post, fm.c_mean, fm.c_std, fm.bounds)
    # float64 NumPy against the long-double truth: a few hundred roundings of values of order one
    assert np.max(np.abs(logF - f.logF)) <= 1e-13 * np.max(np.abs(f.logF))
    assert np.max(np.abs(dlogF - f.dlogF)) <= 1e-12 * np.max(np.abs(f.dlogF))
    assert np.array_equal(fm.log_probability(x), logF)
    fm.update(X0[:4], C0[:4])
    assert fm.generation == 2 and fm.num_rows == 4
    with pytest.raises(ValueError):
        fm.update(X0, C0[:, :1])
    with pytest.raises(ValueError):
        gpo.FeasibilityModel(0)
    with pytest.raises(ValueError):
        gpo.FeasibilityModel(_lib.GP_FEAS_MAX + 1)
    with pytest.raises(NotImplementedError):
        gpo.FeasibilityModel(1, sparse=True)


# ---- the acquisition classes over a recording handle ---------------------------------------------------------------------------------
class Handle(object):
    """Records (method, what matters of its arguments) and answers by shape."""

    def __init__(self, log, D=2):
        self.log, self.D, self.M, self.h, self.lib = log, D, 0, None, None
        self.feas_key = self.cost_key = None
        self.cache = (0, 0)         # what gp_feas_info answers: the LIBRARY's cache
        self.fallback = False       # the next rows calls take the substitution fallback inside the C entry

    def set_candidates(self, Xs):
        self.M = Xs.shape[0]
        self.feas_key = None
        self.cache = (0, 0)
        self.log.append(("set_candidates", Xs.shape[0]))

    def feas_table(self, pack, key=None):
        self.log.append(("feas_table", pack.K, key))
        self.feas_key = key
        self.cache = (pack.K, self.M)

    def feas_info(self):
        return self.cache

    def _rows_call(self):
        if self.fallback:           # gp_set_candidates inside the library: the table and its cache go, the Python key does not
            self.cache = (0, 0)

    def fmin(self):
        self.log.append(("fmin",))
        return -1.0

    def fmin_rows(self, rows):
        self.log.append(("fmin_rows", tuple(int(r) for r in rows)))
        return -0.5

    def acq(self, type_, par, fmin, y_mean=0.0, y_std=1.0):
        self.log.append(("acq", type_, fmin))
        return -np.ones((self.M, 1))

    def acq_grad(self, type_, par, fmin, y_mean=0.0, y_std=1.0):
        self.log.append(("acq_grad", type_, fmin))
        return -np.ones((self.M, 1)), np.zeros((self.M, self.D))

    def acq_argbest(self, type_, par, fmin, sense, y_mean=0.0, y_std=1.0):
        self.log.append(("acq_argbest", type_, fmin, sense))
        return 1, -1.0

    def acq_topk(self, type_, par, fmin, sense, k, y_mean=0.0, y_std=1.0):
        self.log.append(("acq_topk", type_, fmin, k))
        return np.arange(k), np.zeros(k)

    def acq_lp(self, type_, par, fmin, transform, Xb=None, r_x0=None, s_x0=None, y_mean=0.0, y_std=1.0):
        self.log.append(("acq_lp", type_, fmin))
        return np.ones(self.M)

    def acq_lp_argbest(self, type_, par, fmin, transform, sense, Xb=None, r_x0=None, s_x0=None, exclude=(), y_mean=0.0, y_std=1.0):
        self.log.append(("acq_lp_argbest", type_, fmin, tuple(exclude)))
        return 2, 1.0

    def acq_rows(self, Xs, type_, par, fmin, y_mean=0.0, y_std=1.0, grad=False, lp=None):
        self.log.append(("acq_rows", Xs.shape[0], type_, fmin, grad))
        self._rows_call()
        out = -np.ones((Xs.shape[0], 1))
        return (out, np.zeros(Xs.shape)) if grad else out

    def acq_rows_feas(self, pack, Xs, type_, par, fmin, y_mean=0.0, y_std=1.0, grad=False):
        self.log.append(("acq_rows_feas", pack.K, Xs.shape[0], type_, fmin, grad))
        self._rows_call()
        out = -np.ones((Xs.shape[0], 1))
        return (out, np.zeros(Xs.shape)) if grad else out


def _gp(log, n=5):
    gp = types.SimpleNamespace(output_dim=1, normalizer=None, _dirty=False, X=np.zeros((n, 2)), _h=Handle(log),
                               kern=types.SimpleNamespace(_kernel_id=_lib.GP_KERNEL_MATERN52, Gower=False))
    gp._ensure_fit = lambda: None

    def stage(x, fit=True):
        gp._h.set_candidates(x)
        return x
    gp._stage = stage
    return gp


def _scored(log):
    gm = gpo.GPModel(verbose=False)
    gm.model = _gp(log)
    return gm


def _device_feasibility(log, K=2, bounds=0.0):
    """A FeasibilityModel whose constraint models look like fitted exact GPModels with recording handles."""
    fm = gpo.FeasibilityModel(K, bounds, max_iters=0, verbose=False)
    for m in fm.models:
        m.model = _gp(log)
    fm.generation = 1
    fm.num_rows = 5
    fm.feasible_rows = np.array([2, 3], dtype=np.int64)
    return fm


def test_keyword_flags_and_refusals():
    log = []
    gm, fm = _scored(log), _device_feasibility(log)
    for cls in (gpo.AcquisitionEI, gpo.AcquisitionMPI):
        acq = cls(gm, jitter=0.01, feasibility=fm)
        assert acq.feasibility is fm and acq._acq_id == acq._rule.device_id | FEAS and acq._route() is A._EXACT
        assert cls(gm)._acq_id == acq._rule.device_id and cls(gm).feasibility is None
        assert acq._fmin() == -0.5 and log[-1] == ("fmin_rows", (2, 3))      # the incumbent: the feasible rows alone
        fm.feasible_rows = np.empty(0, dtype=np.int64)                      # no feasible observation: the rule is POF
        assert acq._acq_id == _lib.GP_ACQ_POF | FEAS and acq._fmin() == 0.0
        fm.feasible_rows = np.array([2, 3], dtype=np.int64)
    with pytest.raises(ValueError):
        gpo.AcquisitionLCB(gm, feasibility=fm)
    assert gpo.AcquisitionLCB(gm)._acq_id == _lib.GP_ACQ_LCB
    sparse = gpo.GPModel(sparse=True, verbose=False)
    mcmc = gpo.GPModel_MCMC(verbose=False)
    warped = types.SimpleNamespace(analytical_gradient_prediction=True)
    for bad in (sparse, mcmc, warped):
        with pytest.raises(NotImplementedError):
            gpo.AcquisitionEI(bad, feasibility=fm)
    # the incumbent refuses a feasibility model that saw other rows than the scored model
    fm.num_rows = 4
    with pytest.raises(ValueError):
        gpo.AcquisitionEI(gm, feasibility=fm)._fmin()
    # constraint models on another device, or foreign ones, leave the device route
    fm = _device_feasibility(log)
    fm.models[1].device = 1
    assert gpo.AcquisitionEI(gm, feasibility=fm)._route() is None


class _Calls(list):
    """The log without the incumbent's calls (cached per fit and generation: checked by itself)."""

    def seq(self):
        return [c for c in self if c[0] != "fmin_rows"]


def test_table_resync_and_rows_calls():
    log = _Calls()
    gm, fm = _scored(log), _device_feasibility(log)
    acq = gpo.AcquisitionEI(gm, jitter=0.01, feasibility=fm)
    t = _lib.GP_ACQ_EI | FEAS
    key = (id(fm), 1)
    tab = np.random.default_rng(1).uniform(0, 1, (20, 2))
    acq.acquisition_function(tab)
    assert log == [("set_candidates", 20), ("feas_table", 2, key), ("fmin_rows", (2, 3)), ("acq", t, -0.5)]
    acq.acquisition_function(tab[:3])
    assert log.count(("fmin_rows", (2, 3))) == 1                    # the incumbent: once per fit and generation
    del log[:]
    acq.argbest(tab, -1)                                           # the same table object: neither uploaded nor cached again
    acq.topk(tab, 3, -1)
    assert log == [("acq_argbest", t, -0.5, -1), ("acq_topk", t, -0.5, 3)]
    del log[:]
    acq.acquisition_function(tab.copy())                           # another table: both again
    assert [c[0] for c in log] == ["set_candidates", "feas_table", "acq"]
    del log[:]
    fm.generation = 2                                              # refitted constraints: the cache is stale
    fm._pack = None
    tab2 = tab.copy()
    acq.acquisition_function(tab2)
    acq.acquisition_function(tab2)
    assert [c[0] for c in log] == ["set_candidates", "feas_table", "fmin_rows", "acq", "acq"]     # (a new generation: a new incumbent)
    assert log[1] == ("feas_table", 2, (id(fm), 2))
    del log[:]
    gm.model._h.set_candidates(tab2[:3])                           # somebody else's table on the handle: staged and cached again
    del log[:]
    acq.acquisition_function(tab2)
    assert [c[0] for c in log] == ["set_candidates", "feas_table", "acq"]
    del log[:]
    # a rows call that takes the substitution fallback replaces the resident table INSIDE the library and drops its cache; the
    # Python-side key still stands.  The next table call asks the library (gp_feas_info) and stages and caches again
    gm.model._h.fallback = True
    acq.acquisition_function_withGradients(tab2[:1])
    assert gm.model._h.feas_key == (id(fm), 2) and gm.model._h.feas_info() == (0, 0)
    acq.argbest(tab2, -1)
    assert [c[0] for c in log] == ["acq_rows_feas", "set_candidates", "feas_table", "acq_argbest"]
    gm.model._h.fallback = False
    acq.argbest(tab2, -1)
    assert [c[0] for c in log][4:] == ["acq_argbest"]
    del log[:]
    # one location, a lockstep group, and more rows than a group with gradients: gp_acq_rows_feas, one call each
    for M, grad in ((1, True), (8, True), (20, True), (3, False)):
        out = (acq.acquisition_function_withGradients if grad else acq.acquisition_function)(tab[:M])
        assert (out[0] if grad else out).shape == (M, 1)
    assert log == [("acq_rows_feas", 2, 1, t, -0.5, True), ("acq_rows_feas", 2, 8, t, -0.5, True),
                   ("acq_rows_feas", 2, 20, t, -0.5, True), ("acq_rows_feas", 2, 3, t, -0.5, False)]
    del log[:]
    with pytest.raises(NotImplementedError):
        acq.argbest(tab, -1, devices=[0, 1])
    # the penalised acquisition over it: tables, values and arg-best with exclusions; no gradient calls
    lp = gpo.AcquisitionLP(gm, acquisition=acq)
    del log[:]
    lp.acquisition_function(tab[:4])
    lp.argbest(tab, +1, exclude=(1, 2))
    assert [c[0] for c in log] == ["set_candidates", "feas_table", "acq_lp", "set_candidates", "feas_table", "acq_lp_argbest"]
    assert log[2] == ("acq_lp", t, -0.5) and log[-1] == ("acq_lp_argbest", t, -0.5, (1, 2))
    for call in (lp.acquisition_function_withGradients, lp.d_acquisition_function):
        with pytest.raises(NotImplementedError):
            call(tab[:2])


def test_without_a_feasibility_model_the_calls_are_todays():
    log = []
    gm = _scored(log)
    acq = gpo.AcquisitionEI(gm, jitter=0.01)
    tab = np.random.default_rng(2).uniform(0, 1, (20, 2))
    acq.acquisition_function(tab)
    acq.acquisition_function(tab)
    acq.acquisition_function_withGradients(tab)
    acq.acquisition_function_withGradients(tab[:3])
    acq.argbest(tab, -1)
    gpo.AcquisitionLP(gm, acquisition=acq).acquisition_function_withGradients(tab[:2])
    e = _lib.GP_ACQ_EI
    assert log == [("set_candidates", 20), ("fmin",), ("acq", e, -1.0), ("set_candidates", 20), ("fmin",), ("acq", e, -1.0),
                   ("set_candidates", 20), ("fmin",), ("acq_grad", e, -1.0), ("fmin",), ("acq_rows", 3, e, -1.0, True),
                   ("set_candidates", 20), ("fmin",), ("acq_argbest", e, -1.0, -1), ("fmin",), ("acq_rows", 2, e, -1.0, True)]


def test_host_rule_with_foreign_constraint_models(stub_gps):
    """Constraint models that are not ours: the product is formed on the host from log_probability."""
    log = []
    gm = _scored(log)
    fm = gpo.FeasibilityModel(1, 0.0)
    fm.update(X0, C0[:, :1])
    acq = gpo.AcquisitionEI(gm, jitter=0.01, feasibility=fm)
    assert acq._route() is None
    gm.predict = lambda x: (np.zeros((len(x), 1)), np.ones((len(x), 1)))
    gm.predict_withGradients = lambda x: (np.zeros((len(x), 1)), np.ones((len(x), 1)), np.zeros(x.shape), np.zeros(x.shape))
    x = np.array([[0.2, 0.3], [0.7, 0.1]])
    Fx = np.exp(fm.log_probability(x))[:, None]
    base = A._RULES["EI"].value(0.01, -0.5, np.zeros((2, 1)), np.ones((2, 1)))
    assert np.allclose(acq.acquisition_function(x), -base * Fx, rtol=1e-14)
    v, dv = acq.acquisition_function_withGradients(x)
    logF, dlogF = fm.log_probability_withGradients(x)
    assert np.allclose(v, -base * Fx, rtol=1e-14) and np.allclose(dv, -(base * Fx) * dlogF, rtol=1e-13)


# ---- BayesianOptimization ---------------------------------------------------------------------------------------------------------------
DOMAIN = [{"name": "x", "type": "continuous", "domain": (0, 1), "dimensionality": 2}]


def _f(x):
    return np.atleast_2d(x).sum(1)[:, None]


def _c(x):
    return (((np.atleast_2d(x) - 0.5) ** 2).sum(1) - 0.09)[:, None]


def test_bayesian_optimization_bookkeeping(stub_gps, monkeypatch):
    X = np.array([[0.5, 0.5], [0.9, 0.9], [0.1, 0.2], [0.45, 0.6]])
    bo = gpo.BayesianOptimization(_f, domain=DOMAIN, X=X, constraint_function=_c, max_iters=0)
    assert np.array_equal(bo.C, _c(X)) and bo.feasibility.num_constraints == 1 and bo.acquisition.feasibility is bo.feasibility
    assert bo._best_observation() == 0                             # the best FEASIBLE row (row 2 has the lowest objective)
    # no feasible row: the least violating one
    bo.C = bo.C + 1.0
    assert bo._best_observation() == int(np.argmin(bo.C[:, 0]))
    assert np.array_equal(bo.feasibility.violation(bo.C), bo.C[:, 0] / bo.C[:, 0].std())      # ONE definition of 'least violating'
    assert np.array_equal(bo.feasibility.violation(bo.C - 1.0) == 0.0, bo.feasibility.feasible(bo.C - 1.0))
    # the constraint values of the initial design may be given (f = None use), one bound per column
    bo = gpo.BayesianOptimization(None, domain=DOMAIN, X=X, Y=_f(X), C=np.hstack([_c(X), -_c(X)]), constraint_bounds=[0.0, 0.2])
    assert bo.C.shape == (4, 2) and np.array_equal(bo.feasibility.bounds, [0.0, 0.2])
    updates = []
    monkeypatch.setattr(bo.model, "updateModel", lambda *a: updates.append("model"))
    monkeypatch.setattr(bo.feasibility, "update", lambda X_, C_: updates.append(("feasibility", X_.shape, C_.shape)))
    bo._update_model()
    assert updates == ["model", ("feasibility", (4, 2), (4, 2))]     # refitted with the surrogate, on the same rows
    with pytest.raises(B.InvalidConfigError):
        gpo.BayesianOptimization(_f, domain=DOMAIN, X=X, constraint_function=_c, evaluator_type="local_penalization", batch_size=2)
    with pytest.raises(ValueError):
        gpo.BayesianOptimization(_f, domain=DOMAIN, X=X, constraint_function=_c, acquisition_type="LCB")
    with pytest.raises(NotImplementedError):
        gpo.BayesianOptimization(_f, domain=DOMAIN, X=X, constraint_function=_c, acquisition_type="ES")
    plain = gpo.BayesianOptimization(_f, domain=DOMAIN, X=X)
    assert plain.feasibility is None and plain.C is None and plain.acquisition.feasibility is None
    assert plain._best_observation() == int(np.argmin(plain.Y))
