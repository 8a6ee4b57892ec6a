"""Which calls the acquisition classes make for each kind of model (no GPU): EI / LCB / MPI and AcquisitionLP over stand-ins for
the model, the GP behind it, its handle and its replica group that only RECORD (method name, arguments) in one shared log and answer
with arrays of the right shapes.  The grid: model kind (exact, exact with a pending refit, exact without a normaliser, sparse with
and without ``device_acquisitions``, foreign) x 1 / 8 / 9 rows x value / gradient, arg-best with and without ``exclude`` and
``devices``, top-k with k = 5 and 65; for AcquisitionLP no batch, an empty batch given as arrays, a batch of 3, and softplus.

The expected log of every cell (tests/golden/score_routes.json) was recorded from the commit BEFORE the routes of the exact and the
sparse model were folded into one, by ``grid()`` below run against that commit's package; it is data, not derived from the code
under test.  A cell holds the calls in order, each with its arguments by name (arrays as shape and sum), and the shapes of what came back."""
import inspect
import json
import os

import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import acquisitions as A
from gaussian_process_optimization_amd.gpmodel import GPModel

D = 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_routes.json")


def _brief(v):
    """An argument or a result as JSON-able data: arrays by shape and sum, containers element by element."""
    if isinstance(v, np.ndarray):
        return ["array", list(v.shape), round(float(v.sum()), 9)]
    if isinstance(v, (tuple, list, range)):
        return [_brief(e) for e in v]
    if isinstance(v, dict):
        return {k: _brief(e) for k, e in sorted(v.items())}
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


class _Recorder(object):
    """Stands in for ``real`` (_lib.Handle or _lib.Group): logs ``(prefix.method, arguments by name)`` of every method asked of
    it, bound to the real method's signature with its defaults filled in -- a call means the same however it spells its
    arguments, and a call the real method would not take fails here too -- and answers through ``reply``."""

    def __init__(self, prefix, real, log, reply):
        self._prefix, self._real, self._log, self._reply = prefix, real, log, reply

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sig = inspect.signature(getattr(self._real, name))

        def call(*args, **kw):
            bound = sig.bind(self, *args, **kw)
            bound.apply_defaults()
            named = dict(list(bound.arguments.items())[1:])
            self._log.append([self._prefix + "." + name, _brief(named)])
            return self._reply(name, named)
        return call


def _scores(M):
    return np.cos(1.0 + 2.0 * np.arange(M))          # distinct, unordered


class _Table(object):
    """The replies of a handle or a group: what the real ones return, by shape."""

    def __init__(self):
        self.M = 0

    def __call__(self, name, kw):
        if name == "set_candidates":
            self.M = kw["Xs"].shape[0]
            return None
        if name in ("acq_rows", "sparse_acq_rows"):
            M = np.asarray(kw["Xs"]).shape[0]
            out = _scores(M) if kw["lp"] is not None else _scores(M)[:, None]
            return (out, np.ones((M, D))) if kw["grad"] else out
        if name in ("acq", "sparse_acq", "acq_grad", "acq_lp", "acq_lp_grad"):
            flat = name.startswith("acq_lp") or kw.get("lp") is not None
            out = _scores(self.M) if flat else _scores(self.M)[:, None]
            return (out, np.ones((self.M, D))) if (name.endswith("grad") or kw.get("grad")) else out
        if name.endswith("argbest"):
            return 2, -0.5
        if name.endswith("topk"):
            return np.arange(kw["k"], dtype=np.int64), np.zeros(kw["k"])
        if name == "fmin":
            return -1.25
        raise AssertionError("unexpected call " + name)


class _Normaliser(object):
    mean, std = np.array([0.3]), np.array([1.7])

    def inverse_mean(self, v):
        return v * self.std + self.mean


class _GP(object):
    """What the acquisitions ask of the GP object behind a GPModel."""
    output_dim = 1

    def __init__(self, log, sparse, dirty, normaliser):
        self._log, self._sparse, self._dirty = log, sparse, dirty
        self.normalizer = _Normaliser() if normaliser else None
        self._reply = _Table()
        self._h = _Recorder("h", _lib.Handle, log, self._reply)

    def _note(self, name, *args):
        self._log.append(["gp." + name, _brief(args)])

    def _stage(self, x, fit=True):
        self._note("_stage", x, fit)
        self._reply.M = x.shape[0]

    def _predict_resident(self, noise):
        self._note("_predict_resident", noise)
        self._dirty = False

    def _ensure_fit(self):
        self._note("_ensure_fit")

    def _stage_table(self, x):
        self._note("_stage_table", x)
        self._reply.M = x.shape[0]

    def _device_group(self, devices):
        self._note("_device_group", devices)
        if self._sparse:
            raise NotImplementedError("replica groups score the exact GP")
        return _Recorder("grp", _lib.Group, self._log, _Table())


class _Posterior(object):
    """predict / predict_withGradients / get_fmin of a BOModel, recorded."""
    analytical_gradient_prediction = True
    MCMC_sampler = False

    def predict(self, X, with_noise=True):
        X = np.atleast_2d(X)
        self.log.append(["model.predict", _brief((X,))])
        return 0.1 * _scores(X.shape[0])[:, None], 0.5 + 0.1 * np.arange(X.shape[0])[:, None]

    def predict_withGradients(self, X):
        X = np.atleast_2d(X)
        self.log.append(["model.predict_withGradients", _brief((X,))])
        m, s = 0.1 * _scores(X.shape[0])[:, None], 0.5 + 0.1 * np.arange(X.shape[0])[:, None]
        return m, s, np.full(X.shape, 0.25), np.full(X.shape, -0.5)

    def get_fmin(self):
        self.log.append(["model.get_fmin", []])
        return -0.75


class _Ours(_Posterior, GPModel):
    def __init__(self, log, sparse, flag, dirty, normaliser):
        self.log, self.sparse, self.device_acquisitions = log, sparse, flag
        self.model = _GP(log, sparse, dirty, normaliser)


class _Foreign(_Posterior):
    sparse = device_acquisitions = True

    def __init__(self, log):
        self.log = log
        self.model = _GP(log, False, False, True)


KINDS = {"exact": lambda log: _Ours(log, False, False, False, True),
         "exact_dirty": lambda log: _Ours(log, False, False, True, True),
         "exact_raw": lambda log: _Ours(log, False, False, False, False),
         "sparse_on": lambda log: _Ours(log, True, True, False, True),
         "sparse_off": lambda log: _Ours(log, True, False, False, True),
         "foreign": _Foreign}
BASES = {"EI": lambda m: A.AcquisitionEI(m, jitter=0.02), "LCB": lambda m: A.AcquisitionLCB(m, exploration_weight=1.5),
         "MPI": lambda m: A.AcquisitionMPI(m, jitter=0.03)}
BATCHES = ("none", "empty", "three", "softplus")


def _penalised(model, base, batch, x):
    lp = A.AcquisitionLP(model, acquisition=base, transform="softplus" if batch == "softplus" else "none")
    if batch == "empty":
        lp.X_batch, lp.r_x0, lp.s_x0 = np.zeros((0, D)), np.zeros(0), np.zeros(0)
    elif batch != "none":
        lp.update_batches(x[:3] + 0.013, 2.5, -1.0)
    return lp


def _ops(acq, x, penalised):
    """(name, thunk) of every operation of the grid on ``acq``."""
    for M in (1, 8, 9):
        yield "value/%d" % M, lambda M=M: acq.acquisition_function(x[:M])
        yield "gradient/%d" % M, lambda M=M: acq.acquisition_function_withGradients(x[:M])
    for dev in (None, [0, 0]):
        tag = "" if dev is None else "/devices"
        if penalised:
            yield "argbest" + tag, lambda dev=dev: acq.argbest(x[:9], +1, exclude=[1, 4], devices=dev)
            yield "argbest_all" + tag, lambda dev=dev: acq.argbest(x[:9], -1, devices=dev)
        else:
            yield "argbest" + tag, lambda dev=dev: acq.argbest(x[:9], -1, devices=dev)
            for k in (5, 65):
                yield "topk%d%s" % (k, tag), lambda dev=dev, k=k: acq.topk(x[:9], k, +1, devices=dev)
            yield "topk5_short" + tag, lambda dev=dev: acq.topk(x[:3], 5, -1, devices=dev)


def grid():
    """{cell id: {"calls": [...], "result": ...}} of the whole grid, each cell on a fresh model."""
    x = np.random.RandomState(3).uniform(0, 1, (9, D))
    cells = {}
    for kind, make in sorted(KINDS.items()):
        for name, base in sorted(BASES.items()):
            for batch in (None,) + BATCHES:
                for op in [o for o, _ in _ops(None, x, batch is not None)]:
                    log = []
                    model = make(log)
                    acq = base(model)
                    if batch is not None:
                        acq = _penalised(model, acq, batch, x)
                    del log[:]                                  # (update_batches predicts at the batch: not part of the cell)
                    thunk = dict(_ops(acq, x, batch is not None))[op]
                    try:
                        with np.errstate(all="ignore"):
                            result = _brief(thunk())
                    except NotImplementedError as e:
                        result = "NotImplementedError: " + str(e)
                    cells["%s/%s/%s/%s" % (kind, name, batch or "plain", op)] = dict(calls=log, result=result)
    return cells


with open(GOLDEN) as _f:
    _WANT = json.load(_f)
_GOT = {}


def _got():
    if not _GOT:
        _GOT.update(json.loads(json.dumps(grid())))            # (through JSON: tuples and lists compare alike)
    return _GOT


def test_the_grid_is_the_recorded_one():
    assert sorted(_got()) == sorted(_WANT) and len(_WANT) == 6 * 3 * (14 + 4 * 10)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_route_makes_the_recorded_calls(kind):
    bad = [c for c in sorted(_WANT) if c.startswith(kind + "/") and _got()[c] != _WANT[c]]
    for c in bad[:5]:
        print(c, "\n  want", _WANT[c], "\n  got ", _got()[c])
    assert not bad, "%d cells of %s differ, the first: %s" % (len(bad), kind, bad[0])


def test_the_lp_batch_is_packed_once_per_batch():
    """The few-rows path converts the batch once per batch object, not per call (an L-BFGS run makes hundreds of calls)."""
    log = []
    model = KINDS["exact"](log)
    lp = _penalised(model, BASES["EI"](model), "three", np.random.RandomState(3).uniform(0, 1, (9, D)))
    x = np.full((1, D), 0.4)
    lp.acquisition_function(x)
    held = lp._lp_packed
    lp.acquisition_function_withGradients(x)
    assert lp._lp_packed is held and held[1][1].flags["C_CONTIGUOUS"]
    lp.update_batches(x, 2.5, -1.0)
    assert lp._lp_packed is None
