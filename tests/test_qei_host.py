"""CPU: the host logic of ``AcquisitionQEI``, ``JointBatch`` and the ``BayesianOptimization(acquisition_type='qEI')`` wiring over a
stub handle -- the flattening, the tiled bounds, the start selection, the rounding, every refusal and its message, the base
samples (reproducible from ``seed``, re-sent only when the handle changes) -- and what the package exports."""
import types

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib, joint_ei
from gaussian_process_optimization_amd.acquisitions import _host_topk
from gaussian_process_optimization_amd.bayesian_optimization import InvalidConfigError

DOMAIN = [{"name": "x", "type": "continuous", "domain": (0.0, 1.0)}, {"name": "y", "type": "continuous", "domain": (-1.0, 2.0)}]
MIXED = [{"name": "x", "type": "continuous", "domain": (0.0, 1.0)}, {"name": "k", "type": "discrete", "domain": (0.0, 0.5, 1.0)}]
FMIN = 0.3


class _StubHandle(object):
    """What AcquisitionQEI asks of ``_lib.Handle``: -qEI is a bowl around ``target`` (one target row per point of the batch)."""

    def __init__(self, target):
        self.target = np.asarray(target, dtype=float)
        self.qei_key, self.Z, self.sets, self.calls = None, None, 0, []

    def fmin(self):
        return FMIN

    def qei_set(self, Z, key=None):
        self.Z, self.qei_key = np.array(Z), key
        self.sets += 1

    def qei_rows(self, Xq, par=0.0, fmin=0.0, y_mean=0.0, y_std=1.0, include_noise=True, grad=False, posterior=False):
        Xq = np.asarray(Xq, dtype=float)
        self.calls.append(dict(shape=Xq.shape, par=par, fmin=fmin, y_mean=y_mean, y_std=y_std, include_noise=include_noise, grad=grad))
        d = Xq - self.target[:Xq.shape[0]]
        v = float((d * d).sum()) - 1.0
        return (v, 2.0 * d) if grad else v


def _model(target, **kw):
    gm = gpo.GPModel(max_iters=0, verbose=False, **kw)
    gm.model = types.SimpleNamespace(output_dim=1, normalizer=None, kern=types.SimpleNamespace(Gower=False),
                                     _ensure_fit=lambda: None, _h=_StubHandle(target))
    return gm


def _acq(q=3, domain=DOMAIN, seed=4, target=None, **kw):
    space = gpo.Design_space(domain)
    target = np.tile([0.25, 0.5], (q, 1)) + 0.1 * np.arange(q)[:, None] if target is None else target
    gm = _model(target)
    acq = gpo.AcquisitionQEI(gm, space, gpo.AcquisitionOptimizer(space), batch_size=q, num_samples=32, seed=seed, **kw)
    # the candidates' ranking on the host (the device's gp_acq_topk takes its place): the lowest coordinate sums first
    acq._ei.topk = lambda X, k, sense=-1, devices=None: _host_topk(np.asarray(X).sum(1), k, sense)
    return acq, gm


def test_exports_and_constants():
    assert "AcquisitionQEI" in gpo.__all__ and "JointBatch" in gpo.__all__
    assert gpo.joint_ei.AcquisitionQEI is gpo.AcquisitionQEI and gpo.AcquisitionQEI.analytical_gradient_prediction is True
    assert (_lib.GP_QEI_MAX_S, _lib.GP_QEI_MAX_Q) == (4096, 8)
    for name in ("qei_set", "qei_info", "qei_stats", "qei_rows"):
        assert callable(getattr(_lib.Handle, name))
    assert {"gp_qei_set", "gp_qei_info", "gp_qei_stats", "gp_qei_rows"} <= {n for n, _, _ in _lib.SIGNATURES}


def test_flattening_and_the_call_per_row():
    acq, gm = _acq(q=3)
    h = gm.model._h
    X = np.random.RandomState(0).uniform(0, 1, (4, 6))
    assert acq.batches(X).shape == (4, 3, 2) and np.array_equal(acq.batches(X)[2, 1], X[2, 2:4])      # row-major, point by point
    assert acq.batches(X[0]).shape == (1, 3, 2)
    v = acq.acquisition_function(X)
    v2, dv = acq.acquisition_function_withGradients(X)
    assert v.shape == (4, 1) and dv.shape == (4, 6) and np.array_equal(v, v2)
    want = ((X.reshape(4, 3, 2) - h.target) ** 2).sum((1, 2)) - 1.0
    assert np.allclose(v[:, 0], want, rtol=1e-15) and np.allclose(dv, 2 * (X - h.target.ravel()), rtol=1e-15)
    assert len(h.calls) == 8 and all(c["shape"] == (3, 2) for c in h.calls)                             # one gp_qei_rows call per row
    assert all(c["par"] == 0.01 and c["fmin"] == FMIN and (c["y_mean"], c["y_std"]) == (0.0, 1.0) and c["include_noise"] is True
               for c in h.calls)
    assert [c["grad"] for c in h.calls] == [False] * 4 + [True] * 4
    with pytest.raises(ValueError, match="flattened"):
        acq.acquisition_function(X[:, :4])
    assert acq.argbest(X) == (int(np.argmin(want)), float(want.min()))
    with pytest.raises(NotImplementedError, match="batches"):
        acq.topk(X, 2)


def test_normaliser_and_jitter_reach_the_call():
    acq, gm = _acq(q=2, jitter=0.05)
    gm.model.normalizer = types.SimpleNamespace(mean=np.array([1.5]), std=np.array([2.0]),
                                                inverse_mean=lambda a: a * 2.0 + 1.5)
    acq.acquisition_function(np.zeros((1, 4)))
    c = gm.model._h.calls[-1]
    assert (c["par"], c["y_mean"], c["y_std"]) == (0.05, 1.5, 2.0) and c["fmin"] == FMIN * 2.0 + 1.5    # as AcquisitionEI takes them


def test_tiled_bounds():
    acq, _ = _acq(q=3)
    assert acq.tiled_bounds() == [(0.0, 1.0), (-1.0, 2.0)] * 3


def test_start_selection():
    acq, _ = _acq(q=3, seed=9)
    rs = np.random.RandomState(9)
    X = gpo.Design_space(DOMAIN).samples_uniform(1000, rs)            # the candidates optimize() will draw: seeded by ``seed``
    order = np.argsort(X.sum(1), kind="stable")[:15]
    S = acq.starts()
    assert S.shape == (1 + joint_ei.NUM_RANDOM_STARTS, 3, 2)
    assert np.array_equal(S[0], X[order[:3]])                            # the q best under marginal EI, in order
    best = {tuple(r) for r in X[order]}
    for s in S[1:]:                                                      # random q-subsets of the best 5 q, no repeats
        assert {tuple(r) for r in s} <= best and len({tuple(r) for r in s}) == 3
    assert len({s.tobytes() for s in S[1:]}) > 1
    acq2, _ = _acq(q=3, seed=9)
    assert np.array_equal(acq2.starts(), S)                              # reproducible from the seed


def test_optimize_returns_the_batch_and_rounds_row_by_row():
    target = np.array([[0.2, 0.4], [0.7, 0.9], [0.5, 0.1]])
    acq, gm = _acq(q=3, domain=MIXED, target=target)
    x, fx = acq.optimize()
    assert x.shape == (3, 2) and fx.shape == (1, 1)
    assert np.allclose(x[:, 0], target[:, 0], atol=1e-5)                 # the bowl's minimum in the continuous variable
    assert np.array_equal(x[:, 1], [0.5, 1.0, 0.0])                      # the discrete one snapped, every row on its own
    assert np.isclose(fx[0, 0], ((x - target) ** 2).sum() - 1.0, rtol=1e-12)      # the value of what is returned
    assert acq.last_starts.shape == (5, 3, 2) and acq.last_start_values.shape == (5,)
    assert fx[0, 0] <= acq.last_start_values.min() + 0.03                # (rounding k moved it by at most 3 * 0.1^2)
    calls = gm.model._h.calls
    assert all(c["shape"] == (3, 2) for c in calls)
    jb = gpo.JointBatch(acq, 3)
    xb = jb.compute_batch()
    assert xb.shape == (3, 2) and np.allclose(xb, x, atol=1e-5)
    with pytest.raises(NotImplementedError):
        jb.compute_batch(duplicate_manager=object())
    with pytest.raises(TypeError):
        gpo.JointBatch(gpo.AcquisitionEI(gm, gpo.Design_space(MIXED)), 3)
    with pytest.raises(ValueError):
        gpo.JointBatch(acq, 2)


def test_same_seed_same_batch():
    a, _ = _acq(q=2, seed=3)
    b, _ = _acq(q=2, seed=3)
    assert np.array_equal(a.optimize()[0], b.optimize()[0])


def test_base_samples():
    a, gm = _acq(q=3, seed=4)
    b, _ = _acq(q=3, seed=4)
    c, _ = _acq(q=3, seed=5)
    assert a.Z.shape == (32, 3) and np.array_equal(a.Z, b.Z) and not np.array_equal(a.Z, c.Z)
    assert np.array_equal(a.Z, np.random.default_rng(4).standard_normal((32, 3)))
    assert not a.Z.flags.writeable
    h = gm.model._h
    assert a.uploads == 0 and h.sets == 0                               # drawn at construction, sent at the first call
    X = np.zeros((2, 6))
    a.acquisition_function(X)
    a.acquisition_function_withGradients(X)
    assert a.uploads == 1 and h.sets == 1 and np.array_equal(h.Z, a.Z) and h.qei_key == a._key
    h2 = _StubHandle(h.target)                                          # the model rebuilt its handle
    gm.model._h = h2
    a.acquisition_function(X)
    a.acquisition_function(X)
    assert a.uploads == 2 and h2.sets == 1 and np.array_equal(h2.Z, a.Z)
    h2.qei_key = ("someone", "else")                                    # another object's samples took their place
    a.acquisition_function(X)
    assert a.uploads == 3 and h2.qei_key == a._key


def test_a_positive_return_code_is_a_linalg_error():
    class _Lib(object):
        @staticmethod
        def gp_qei_rows(*a):
            return 2

    h = _lib.Handle.__new__(_lib.Handle)
    h.lib, h.h, h.D = _Lib(), None, 2
    with pytest.raises(np.linalg.LinAlgError, match="row 2") as e:
        h.qei_rows(np.zeros((3, 2)), grad=True)
    assert e.value.args[1] == 2
    with pytest.raises(ValueError, match="shape"):
        h.qei_rows(np.zeros((3, 5)))
    acq, gm = _acq(q=2)

    def failing(*a, **k):
        raise np.linalg.LinAlgError("gp_qei_rows: the batch's joint covariance is not positive definite at row 2", 2)
    gm.model._h.qei_rows = failing
    with pytest.raises(np.linalg.LinAlgError):
        acq.acquisition_function(np.zeros((1, 4)))


def test_refused_models_and_options():
    space = gpo.Design_space(DOMAIN)
    style = "joint expected improvement scores batches over our exact GPModel"
    with pytest.raises(NotImplementedError, match=style + ".*foreign, MCMC, warped or input-warped"):
        gpo.AcquisitionQEI(object(), space)
    for foreign in (gpo.GPModel_MCMC(verbose=False), gpo.WarpedGPModel(verbose=False) if hasattr(gpo, "WarpedGPModel") else object(),
                    gpo.InputWarpedGPModel(space, verbose=False)):
        with pytest.raises(NotImplementedError, match=style):
            gpo.AcquisitionQEI(foreign, space)
    with pytest.raises(NotImplementedError, match=style + ".*sparse=True"):
        gpo.AcquisitionQEI(gpo.GPModel(sparse=True, verbose=False), space)
    with pytest.raises(NotImplementedError, match=style + ".*Gower"):
        gpo.AcquisitionQEI(gpo.GPModel(Gower=True, space=space, verbose=False), space)
    with pytest.raises(NotImplementedError, match=style + ".*mean function"):
        gpo.AcquisitionQEI(gpo.GPModel(mean_function=gpo.mappings.Linear(2, 1), verbose=False), space)
    gm = _model(np.zeros((2, 2)))
    with pytest.raises(NotImplementedError, match="no cost model"):
        gpo.AcquisitionQEI(gm, space, cost_withGradients=lambda x: (np.ones((x.shape[0], 1)), np.zeros(x.shape)))
    with pytest.raises(NotImplementedError, match="no black-box constraints"):
        gpo.AcquisitionQEI(gm, space, feasibility=object())
    with pytest.raises(NotImplementedError, match="no black-box constraints"):
        gpo.AcquisitionQEI(gm, space)._set_feasibility(object())
    for bad in (0, 9):
        with pytest.raises(ValueError, match="between 1 and 8 points"):
            gpo.AcquisitionQEI(gm, space, batch_size=bad)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="between 1 and 4096 base samples"):
            gpo.AcquisitionQEI(gm, space, num_samples=bad)
    # what only shows once the model has data: several outputs, a Gower kernel object
    acq = gpo.AcquisitionQEI(gm, space)
    gm.model.output_dim = 2
    with pytest.raises(NotImplementedError, match=style + ".*2 outputs"):
        acq.acquisition_function(np.zeros((1, 4)))
    gm.model.output_dim, gm.model.kern.Gower = 1, True
    with pytest.raises(NotImplementedError, match=style + ".*Gower"):
        acq.acquisition_function(np.zeros((1, 4)))
    gm.model = None
    with pytest.raises(RuntimeError, match="updateModel first"):
        acq.acquisition_function(np.zeros((1, 4)))


def test_front_door_wiring():
    X = np.random.RandomState(1).uniform(0, 1, (6, 2))
    Y = X.sum(1)[:, None]
    kw = dict(f=None, domain=DOMAIN, X=X, Y=Y, acquisition_type="qEI")
    for ev in ("sequential", None, "joint"):
        bo = gpo.BayesianOptimization(evaluator_type=ev, batch_size=3, num_qei_samples=64, sampler_seed=2, acquisition_jitter=0.02,
                                      parallel_anchors=True, **kw)      # parallel_anchors: accepted, ignored
        acq = bo.acquisition
        assert isinstance(acq, gpo.AcquisitionQEI) and isinstance(bo.evaluator, gpo.JointBatch) and bo.evaluator.acquisition is acq
        assert (acq.batch_size, acq.num_samples, acq.jitter, acq.seed) == (3, 64, 0.02, 2) and acq.Z.shape == (64, 3)
    bo = gpo.BayesianOptimization(batch_size=1, **kw)
    assert bo.acquisition.batch_size == 1 and isinstance(bo.evaluator, gpo.JointBatch) and bo.acquisition.num_samples == 256
    for ev in ("local_penalization", "thompson_sampling", "random"):
        with pytest.raises(InvalidConfigError, match="batch as a whole"):
            gpo.BayesianOptimization(evaluator_type=ev, batch_size=3, **kw)
    with pytest.raises(ValueError, match="1 to 8"):
        gpo.BayesianOptimization(batch_size=9, **kw)
    with pytest.raises(InvalidConfigError, match="'joint' evaluator"):
        gpo.BayesianOptimization(f=None, domain=DOMAIN, X=X, Y=Y, acquisition_type="EI", evaluator_type="joint", batch_size=2)
    with pytest.raises(NotImplementedError, match="qEI.*no black-box constraints"):
        gpo.BayesianOptimization(batch_size=2, constraint_function=lambda x: x[:, :1] - 0.5, C=X[:, :1] - 0.5, **kw)
    with pytest.raises(NotImplementedError, match="no cost model"):
        gpo.BayesianOptimization(batch_size=2, cost_withGradients=lambda x: (np.ones((x.shape[0], 1)), np.zeros(x.shape)), **kw)
    with pytest.raises(NotImplementedError, match="joint expected improvement scores batches"):
        gpo.BayesianOptimization(batch_size=2, model_type="input_warped_GP", **kw)
    with pytest.raises(NotImplementedError, match="joint expected improvement scores batches"):
        gpo.BayesianOptimization(batch_size=2, model=gpo.GPModel(sparse=True, verbose=False), **kw)
