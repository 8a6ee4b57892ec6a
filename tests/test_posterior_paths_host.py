"""CPU: ``PosteriorPaths``, ``AcquisitionTS``, ``ThompsonPathsBatch`` and ``AcquisitionMES(sampler=...)`` over a stand-in handle
that answers the gp_paths_* calls from tests/_paths_truth.py in NumPy double: argument checks and refusals, the redraw-on-refit
logic, the batch evaluator's wiring, and the Gumbel sampler left as it was."""
import types

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import bayesian_optimization as bo
from gaussian_process_optimization_amd import parameterization
from gaussian_process_optimization_amd import posterior_paths as PP

import _paths_truth as PT
from test_mes_host import DOMAIN, _HostModel, _data, _f

NOISE = 1e-2


class _Handle(object):
    """The paths calls of ``_lib.Handle`` in NumPy double; counts what reaches it."""

    def __init__(self, gp):
        self.gp, self.paths_key, self.draws, self.cand = gp, None, None, None
        self.set_calls, self.rows_calls, self.table_calls, self.row_paths = 0, 0, 0, []

    def paths_set(self, omega_unit, phase, w, z_eps, key=None):
        self.set_calls += 1
        self.draws, self.paths_key = (omega_unit, phase, w, z_eps), key

    def paths_info(self):
        return (0, 0) if self.draws is None else self.draws[2].shape

    def set_candidates(self, X):
        self.cand = np.array(X, dtype=float)

    def _eval(self, X, grad):
        g = self.gp
        ls = np.broadcast_to(np.ravel(g.kern.lengthscale.values), (g.input_dim,))
        t = PT.evaluate(g.fam, float(g.kern.variance), ls, PT.sigma2(NOISE), g.X, g.Y, self.draws, X, lin=PT.F64, grad=grad,
                        bounds=False)
        return t.prior + t.update, (t.dprior + t.dupdate if grad else None)

    def paths_rows(self, Xs, path, y_mean=0.0, y_std=1.0, grad=False):
        assert 1 <= Xs.shape[0] <= 8
        self.rows_calls += 1
        path = np.broadcast_to(np.asarray(path).ravel(), (Xs.shape[0],)) if np.size(path) == 1 else np.asarray(path)
        self.row_paths.append(np.array(path))
        f, df = self._eval(Xs, grad)
        idx = np.arange(Xs.shape[0])
        out = y_std * f[path, idx] + y_mean
        return (out, y_std * df[path, idx]) if grad else out

    def paths_table(self, y_mean=0.0, y_std=1.0):
        self.table_calls += 1
        return y_std * self._eval(self.cand, False)[0] + y_mean

    def paths_argbest(self, sense=-1, y_mean=0.0, y_std=1.0):
        t = self.paths_table(y_mean, y_std)
        idx = np.argmin(t, axis=1) if sense < 0 else np.argmax(t, axis=1)
        return idx, t[np.arange(t.shape[0]), idx]

    mes_logsurv = None      # (MinValueSampler._device_gp asks whether the handle has the sampler's entries)


class _GP(object):
    """What the paths ask of a ``GPRegression``, without a device."""
    _appendable = True

    def __init__(self, fam="Mat52", N=14, D=2, outputs=1, gower=False, mean_function=None):
        rng = np.random.RandomState(4)
        self.fam, self.X = fam, rng.uniform(0, 1, (N, D))
        self.Y = _f(self.X) if D == 2 else self.X.sum(1)[:, None]
        self.Y = (self.Y - self.Y.mean()) / self.Y.std()
        self.kern = types.SimpleNamespace(_kernel_id=PT.FAMILY_ID[fam], ARD=False, variance=1.1,
                                          lengthscale=types.SimpleNamespace(values=np.array([0.45])))
        self.likelihood = types.SimpleNamespace(variance=NOISE)
        self.output_dim, self.input_dim, self.num_data = outputs, D, N
        self.mean_function, self.normalizer, self._gower = mean_function, None, gower
        self._data_epoch, self._dirty, self.fits = 1, False, 0
        self._h = _Handle(self)

    def _uses_gower(self):
        return self._gower

    def _ensure_fit(self):
        self.fits += self._dirty
        self._dirty = False


class _Sparse(_GP):
    _appendable = False


def _gpmodel(gp=None):
    gm = gpo.GPModel(max_iters=0, verbose=False)
    gm.model = _GP() if gp is None else gp
    gm.updateModel = lambda *a: None           # the loop's refit: the stand-in is fitted
    gm.get_fmin = lambda: float(gm.model.Y.min())
    return gm


def test_exports_and_constants():
    assert {"AcquisitionTS", "PosteriorPaths", "posterior_paths"} <= set(gpo.__all__)
    assert (_lib.GP_PATHS_MAX_S, _lib.GP_PATHS_MAX_F, _lib.GP_PATHS_MAX_ROWS) == (64, 4096, 8)
    assert gpo.AcquisitionTS.analytical_gradient_prediction is True
    names = [s[0] for s in _lib.SIGNATURES]
    assert all(n in names for n in ("gp_paths_set", "gp_paths_info", "gp_paths_table", "gp_paths_argbest", "gp_paths_rows"))
    assert hasattr(gpo.GPRegression, "posterior_paths")


def test_models_without_paths_are_refused_before_anything_reaches_the_handle():
    for gp in (_GP(gower=True), _GP(mean_function=object()), _GP(outputs=2), _Sparse()):
        with pytest.raises(NotImplementedError):
            PP.PosteriorPaths(gp, size=2, num_features=8, seed=1)
        assert gp._h.set_calls == 0
    gp = _GP()
    for kw in ({"size": 0}, {"size": 65}, {"num_features": 0}, {"num_features": 4097}):
        with pytest.raises(ValueError):
            PP.PosteriorPaths(gp, **{"size": 2, "num_features": 8, **kw})
    assert gp._h.set_calls == 0


def test_paths_object_routes_and_staleness():
    gp = _GP()
    paths = PP.PosteriorPaths(gp, size=3, num_features=16, seed=2)
    assert (paths.size, paths.num_features) == (3, 16) and gp._h.set_calls == 1
    Xq = np.random.RandomState(1).uniform(0, 1, (20, 2))
    tab = paths(Xq)
    assert tab.shape == (20, 3) and gp._h.table_calls == 1 and gp._h.rows_calls == 0
    few = paths(Xq[:8])                        # eight rows go by value: one path per call
    assert gp._h.table_calls == 1 and gp._h.rows_calls == 3 and np.allclose(few, tab[:8], rtol=0, atol=1e-12)
    two = paths(Xq[:2])                        # two rows: four copies of them fit a call
    assert gp._h.rows_calls == 4 and np.allclose(two, tab[:2], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        paths(np.zeros((3, 5)))
    f, df = paths.value_and_gradient(Xq[:4], path=[0, 1, 2, 0])
    assert np.allclose(f, tab[[0, 1, 2, 3], [0, 1, 2, 0]], rtol=0, atol=1e-12) and df.shape == (4, 2)
    idx, val = paths.argmin(Xq)
    assert np.array_equal(idx, np.argmin(tab, axis=0))
    # other paths took their place on the handle
    other = PP.PosteriorPaths(gp, size=1, num_features=8, seed=3)
    with pytest.raises(RuntimeError, match="another fit"):
        paths(Xq)
    assert other(Xq).shape == (20, 1)
    # new hyper-parameters, a pending refit, new data: each raises instead of re-solving silently
    calls = gp._h.set_calls
    gp.kern.variance = 1.4
    with pytest.raises(RuntimeError):
        other(Xq)
    gp.kern.variance = 1.1
    assert other(Xq).shape == (20, 1)
    gp._dirty = True
    with pytest.raises(RuntimeError):
        other(Xq)
    gp._dirty = False
    gp._data_epoch += 1
    with pytest.raises(RuntimeError):
        other.argmin(Xq)
    assert gp._h.set_calls == calls


def test_acquisition_ts_refusals():
    space = gpo.Design_space(DOMAIN)
    gm = _gpmodel()
    for model in (_HostModel(), gpo.GPModel(sparse=True, verbose=False), gpo.GPModel_MCMC.__new__(gpo.GPModel_MCMC), object()):
        with pytest.raises(NotImplementedError):
            gpo.AcquisitionTS(model, space)
    with pytest.raises(NotImplementedError, match="cost"):
        gpo.AcquisitionTS(gm, space, cost_withGradients=lambda x: (np.ones((x.shape[0], 1)), np.zeros(x.shape)))
    with pytest.raises(NotImplementedError, match="constraints"):
        gpo.AcquisitionTS(gm, space, feasibility=object())
    acq = gpo.AcquisitionTS(gm, space, num_paths=2, num_features=8, seed=1)
    with pytest.raises(NotImplementedError, match="constraints"):
        acq._set_feasibility(object())
    with pytest.raises(NotImplementedError):
        gpo.AcquisitionLP(gm, space, None, acq)
    with pytest.raises(NotImplementedError, match="replica groups"):
        acq.argbest(np.zeros((3, 2)), devices=[0])
    for kw in ({"num_paths": 0}, {"num_paths": 65}, {"num_features": 0}, {"num_features": 4097}):
        with pytest.raises(ValueError):
            gpo.AcquisitionTS(gm, space, **kw)
    with pytest.raises(ValueError):
        acq.select_path(2)
    X, Y = _data()
    with pytest.raises(NotImplementedError, match="local_penalization"):
        gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model=_gpmodel(), acquisition_type="TS", normalize_Y=False,
                                 evaluator_type="local_penalization", batch_size=2)
    with pytest.raises(NotImplementedError):
        gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model=_gpmodel(), acquisition_type="TS", normalize_Y=False,
                                 cost_withGradients=lambda x: (np.ones((x.shape[0], 1)), np.zeros(x.shape)))
    with pytest.raises(NotImplementedError):
        gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model=_gpmodel(), acquisition_type="TS", normalize_Y=False,
                                 constraint_function=lambda x: x[:, :1] - 0.5, C=X[:, :1] - 0.5)


def test_acquisition_ts_scores_the_selected_path_and_redraws_on_refit():
    gm = _gpmodel()
    gp, h = gm.model, gm.model._h
    acq = gpo.AcquisitionTS(gm, gpo.Design_space(DOMAIN), num_paths=3, num_features=16, seed=5)
    Xq = np.random.RandomState(1).uniform(0, 1, (30, 2))
    v0 = acq.acquisition_function(Xq)
    assert v0.shape == (30, 1) and acq.draws == 1 and h.set_calls == 1
    tab = acq.table_on_paths(Xq)
    assert tab.shape == (30, 3) and np.array_equal(tab[:, 0], v0[:, 0])     # f itself, to be minimised: LCB's sign convention
    acq.select_path(2)
    v2, dv2 = acq.acquisition_function_withGradients(Xq[:5])
    assert np.allclose(v2[:, 0], tab[:5, 2], rtol=0, atol=1e-12) and dv2.shape == (5, 2)
    assert np.array_equal(-acq._compute_acq(Xq[:5]), acq.acquisition_function(Xq[:5]))
    i, v = acq.argbest(Xq)
    assert i == int(np.argmin(tab[:, 2])) and v == tab[i, 2]
    idx, val = acq.topk(Xq, 4)
    assert np.array_equal(idx, np.argsort(tab[:, 2], kind="stable")[:4])
    more, dmore = acq.acquisition_function_withGradients(Xq[:11])           # groups of eight rows
    assert more.shape == (11, 1) and dmore.shape == (11, 2) and [p.size for p in h.row_paths[-2:]] == [8, 3]
    assert acq.draws == 1 and h.set_calls == 1
    # a refit with other hyper-parameters, new data, or paths of someone else on the handle: redrawn, once each
    gp.kern.variance = 1.5
    assert not np.array_equal(acq.acquisition_function(Xq), tab[:, 2:3]) and acq.draws == 2
    acq.acquisition_function(Xq)
    assert acq.draws == 2
    gp._data_epoch += 1
    acq.acquisition_function(Xq[:2])
    assert acq.draws == 3
    PP.PosteriorPaths(gp, size=1, num_features=8, seed=1)
    acq.acquisition_function(Xq[:2])
    assert acq.draws == 4 and h.paths_info() == (3, 16)
    # the same seed draws the same sequence of paths
    again = gpo.AcquisitionTS(_gpmodel(), gpo.Design_space(DOMAIN), num_paths=3, num_features=16, seed=5)
    assert np.array_equal(again.acquisition_function(Xq), v0)


@pytest.mark.parametrize("parallel", [False, True])
def test_thompson_paths_batch_wiring(parallel):
    X, Y = _data()
    gm = _gpmodel()
    h = gm.model._h
    np.random.seed(3)
    opt = gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model=gm, acquisition_type="TS", num_features=16,
                                   sampler_seed=4, normalize_Y=False, evaluator_type="thompson_sampling", batch_size=3,
                                   parallel_anchors=parallel)
    assert isinstance(opt.acquisition, gpo.AcquisitionTS) and isinstance(opt.evaluator, bo.ThompsonPathsBatch)
    assert opt.acquisition.num_features == 16
    opt.evaluator.num_samples = 60
    xb = np.atleast_2d(opt.suggest_next_locations())
    assert xb.shape == (3, 2) and np.all(xb >= 0) and np.all(xb <= 1)
    assert opt.acquisition.draws == 1 and h.paths_info() == (3, 16)         # B paths, drawn once for the batch
    # element b is a minimiser of ITS path: no worse than its anchor table's best under that path, and every gradient call
    # carried the path of the run it belongs to
    np.random.seed(3)
    anchors_table = opt.space.samples_uniform(60)
    tab = opt.acquisition.table_on_paths(anchors_table)
    own = opt.acquisition.values_on_paths(xb, np.arange(3))[:, 0]
    assert np.all(own <= tab.min(axis=0) + 1e-12)
    used = np.concatenate(h.row_paths[:-1])
    assert set(used.tolist()) == {0, 1, 2}
    if parallel:
        assert any(p.size > 1 for p in h.row_paths) and all(np.all(np.diff(p) > 0) for p in h.row_paths[:-1])
    else:
        assert all(p.size == 1 for p in h.row_paths[:-1])
    assert len({tuple(np.round(r, 12)) for r in xb}) == 3
    # every other acquisition keeps the reference's marginal Thompson batch
    ei = gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model=_HostModel(), acquisition_type="EI", normalize_Y=False,
                                  evaluator_type="thompson_sampling", batch_size=2)
    assert type(ei.evaluator) is bo.ThompsonBatch
    with pytest.raises(TypeError):
        bo.ThompsonPathsBatch(ei.acquisition, 2)


def test_sequential_draws_a_fresh_path_per_suggestion():
    X, Y = _data()
    gm = _gpmodel()
    opt = gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, model=gm, acquisition_type="TS", num_features=16,
                                   sampler_seed=4, normalize_Y=False)
    assert opt.evaluator is None
    opt.acquisition_optimizer.num_samples, opt.acquisition_optimizer.maxiter = 40, 5
    np.random.seed(1)
    a = opt.suggest_next_locations()
    b = opt.suggest_next_locations()
    assert opt.acquisition.draws == 2 and a.shape == b.shape == (1, 2) and not np.array_equal(a, b)


def test_lockstep_driver_hands_out_the_instances_of_its_rows():
    centres = [np.array([0.2, 0.1]), np.array([-0.4, 0.3]), np.array([0.0, 0.9])]
    seen = []

    def fbatch(xs, idx):
        seen.append(list(idx))
        c = np.array([centres[i] for i in idx])
        return ((xs - c) ** 2).sum(1) * np.array([1.0 + 50 * i for i in idx]), 2 * (xs - c) * np.array([[1.0 + 50 * i] for i in idx])

    res = parameterization.lbfgsb_lockstep(fbatch, [np.zeros(2)] * 3, with_index=True)
    for r, c in zip(res, centres):
        assert np.allclose(r[0], c, atol=1e-6)
    assert seen[0] == [0, 1, 2] and all(s == sorted(s) for s in seen)


def test_the_gumbel_sampler_is_the_default_and_unchanged():
    X, Y = _data()
    gm = _HostModel()
    gm.updateModel(X, Y, None, None)
    space = gpo.Design_space(DOMAIN)
    np.random.seed(7)
    a = gpo.MinValueSampler(gm, space, 6, 120, seed=3)
    ya = a.sample()
    np.random.seed(7)
    b = gpo.MinValueSampler(gm, space, 6, 120, seed=3, sampler="gumbel")
    yb = b.sample()
    assert a.sampler == "gumbel" and np.array_equal(ya, yb) and a.last_fit == b.last_fit
    acq = gpo.AcquisitionMES(gm, space, num_samples=4, grid_size=50, seed=1)
    assert acq.sampler.sampler == "gumbel"
    with pytest.raises(ValueError):
        gpo.MinValueSampler(gm, space, 6, 120, sampler="sobol")
    # the paths sampler needs the exact model's handle ...
    with pytest.raises(NotImplementedError, match="paths"):
        gpo.AcquisitionMES(gm, space, num_samples=4, grid_size=50, seed=1, sampler="paths").sampler.sample()
    # ... and over it yields K minima of K paths, clipped at the incumbent
    em = _gpmodel()
    s = gpo.MinValueSampler(em, space, 5, 80, seed=2, sampler="paths", num_features=16)
    np.random.seed(2)
    y = s.sample()
    assert y.shape == (5,) and np.all(np.isfinite(y)) and np.all(y <= em.get_fmin()) and em.model._h.paths_info() == (5, 16)
    assert s.last_argmin.shape == (5,)


def test_a_handful_of_rows_goes_by_value_whatever_the_dimension():
    """The rows entry makes its own passes (M D <= 128 coordinates each): the callers do not cap the dimension."""
    gp = _GP(D=20)
    paths = PP.PosteriorPaths(gp, size=10, num_features=8, seed=2)
    x = np.random.RandomState(1).uniform(0, 1, (1, 20))
    assert paths(x).shape == (1, 10) and gp._h.table_calls == 0 and [p.size for p in gp._h.row_paths] == [8, 2]
    f, df = paths.value_and_gradient(np.repeat(x, 8, axis=0), path=np.arange(8))
    assert f.shape == (8,) and df.shape == (8, 20)
    gm = _gpmodel(_GP(D=20))
    acq = gpo.AcquisitionTS(gm, None, num_paths=2, num_features=8, seed=1)
    v, dv = acq.acquisition_function_withGradients(np.repeat(x, 8, axis=0))
    assert v.shape == (8, 1) and dv.shape == (8, 20) and gm.model._h.table_calls == 0
    assert acq.acquisition_function(np.repeat(x, 8, axis=0)).shape == (8, 1) and gm.model._h.table_calls == 0
