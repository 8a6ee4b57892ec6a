"""CPU: the mean-function mappings (mappings.py) against NumPy, the order and names of a model's parameters with one, the calls a
model with a mean function makes on its handle -- over a recording stand-in defined here --, and the refusals.  No GPU."""
import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import acquisitions as A
from gaussian_process_optimization_amd import mappings as M


# ---- the mappings -------------------------------------------------------------------------------------------------------------------
def _data(N=7, D=3, P=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, D)), rng.standard_normal((N, P))


def test_linear_against_numpy():
    X, dF = _data()
    np.random.seed(3)
    expect = np.random.randn(3, 2)
    np.random.seed(3)
    lin = M.Linear(3, 2)
    assert np.array_equal(lin.A_matrix, expect)                 # drawn with np.random.randn, as the reference draws it
    assert np.array_equal(lin.f(X), X @ expect)
    lin.update_gradients(dF, X)
    assert np.array_equal(lin.A.gradient, (X.T @ dF).reshape(-1))
    assert np.array_equal(lin.gradients_X(dF, X), dF @ expect.T)
    assert lin.input_dim == 3 and lin.output_dim == 2 and lin.name == "linmap"


def test_constant_against_numpy():
    X, dF = _data()
    con = M.Constant(3, 2, value=1.5)
    assert np.array_equal(con.C.values, [1.5, 1.5])
    assert np.array_equal(con.f(X), np.full((7, 2), 1.5))
    con.update_gradients(dF, X)
    assert np.array_equal(con.C.gradient, dF.sum(0))
    assert np.array_equal(con.gradients_X(dF, X), np.zeros_like(X))
    assert np.array_equal(M.Constant(3, 2, value=[1.0, -2.0]).C.values, [1.0, -2.0])
    assert np.array_equal(M.Constant(3, 2).C.values, [0.0, 0.0])
    with pytest.raises(ValueError):
        M.Constant(3, 2, value=np.zeros((2, 2)))


def test_additive_against_numpy():
    X, dF = _data()
    lin, con = M.Linear(3, 2), M.Constant(3, 2, value=[0.5, -1.0])
    add = M.Additive(lin, con)
    assert np.array_equal(add.f(X), X @ lin.A_matrix + np.array([0.5, -1.0]))
    add.update_gradients(dF, X)
    assert np.array_equal(lin.A.gradient, (X.T @ dF).reshape(-1)) and np.array_equal(con.C.gradient, dF.sum(0))
    assert np.array_equal(add.gradients_X(dF, X), dF @ lin.A_matrix.T)
    with pytest.raises(AssertionError):
        M.Additive(M.Linear(3, 2), M.Constant(2, 2))
    with pytest.raises(AssertionError):
        M.Additive(M.Linear(3, 2), M.Constant(3, 1))


def test_affine_parts_and_device_gradients():
    lin, lin2, con = M.Linear(3, 2), M.Linear(3, 2), M.Constant(3, 2, value=[0.5, -1.0])
    assert M.affine_parts(lin)[1] is None and np.array_equal(M.affine_parts(lin)[0], lin.A_matrix)
    assert M.affine_parts(con)[0] is None and np.array_equal(M.affine_parts(con)[1], [0.5, -1.0])
    Aa, bb = M.affine_parts(M.Additive(M.Additive(lin, con), lin2))
    assert np.array_equal(Aa, lin.A_matrix + lin2.A_matrix) and np.array_equal(bb, [0.5, -1.0])
    dA, db = np.arange(6.0).reshape(3, 2), np.array([7.0, 8.0])
    M.set_affine_gradients(M.Additive(M.Additive(lin, con), lin2), dA, db)
    assert np.array_equal(lin.A.gradient, dA.reshape(-1)) and np.array_equal(lin2.A.gradient, dA.reshape(-1))
    assert np.array_equal(con.C.gradient, db)
    # unconstrained: the optimiser sees the values themselves, negative ones included
    con.C.set([-3.0, 2.0])
    assert np.array_equal(con.optimizer_array, [-3.0, 2.0])
    twin = M.Additive(lin, con).copy()
    assert np.array_equal(twin.param_array, np.r_[lin.A.values, con.C.values]) and twin.mapping1 is not lin


class _Other(M.Mapping):
    def f(self, X):
        return np.tanh(X[:, :1])


# ---- a model over a recording stand-in handle ---------------------------------------------------------------------------------------
class _Handle(object):
    """Records the calls a model makes; answers with fixed numbers (dA = 1, 2, ... and db = -1, -2, ...)."""
    calls = None

    def __init__(self, device=0):
        self.calls, self.device = [], device

    def _note(self, name, *a):
        self.calls.append((name,) + a)

    def set_data(self, X, Y):
        self.D, self.P = X.shape[1], Y.shape[1]
        self._note("set_data", X.shape, Y.copy())

    def set_gower(self, *a):
        pass

    def set_params(self, *a):
        self._note("set_params")

    def mean_set(self, A=None, b=None):
        self._note("mean_set", None if A is None else np.array(A), None if b is None else np.array(b))

    def mean_grad(self):
        self._note("mean_grad")
        return np.arange(1.0, self.D * self.P + 1).reshape(self.D, self.P), -np.arange(1.0, self.P + 1)

    def fit(self, maxtries=5):
        self._note("fit")
        return -1.0, 0.0, 0.0

    def fit_grad(self, nls, maxtries=5):
        self._note("fit_grad")
        return (-1.0, 0.0, 0.0), (0.25, np.full(nls, 0.5), 0.75)

    def lml_grad(self, nls):
        self._note("lml_grad")
        return 0.25, np.full(nls, 0.5), 0.75

    def append(self, *a):
        raise AssertionError("a model with a mean function refits")

    def count(self, name):
        return sum(1 for c in self.calls if c[0] == name)

    def close(self):
        pass


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", _Handle)


def _model(mean, N=6, D=3, P=2, **kw):
    rng = np.random.default_rng(1)
    return gpo.GPRegression(rng.uniform(0, 1, (N, D)), rng.standard_normal((N, P)), gpo.kern.RBF(D, 1.0, 0.5), noise_var=0.1,
                            mean_function=mean, **kw)


def test_parameter_order_and_names(stand_in):
    lin, con = M.Linear(3, 2), M.Constant(3, 2, value=[0.5, -1.0])
    m = _model(M.Additive(lin, con))
    assert np.array_equal(m.param_array, np.r_[lin.A.values, [0.5, -1.0], 1.0, 0.5, 0.1])      # [mean parameters, variance, lengthscale, noise]
    names = list(m.parameter_names_flat())
    assert len(names) == 11 and "linmap.A" in names[0] and "constmap.C" in names[6]
    assert "variance" in names[8] and "lengthscale" in names[9] and "Gaussian_noise" in names[10]
    x = m.optimizer_array
    assert np.array_equal(x[:8], np.r_[lin.A.values, [0.5, -1.0]])      # unconstrained
    g = m.gradient
    assert np.array_equal(g, np.r_[np.arange(1.0, 7.0), [-1.0, -2.0], 0.25, 0.5, 0.75])
    assert m.mean_function.input_dim == 3 and m.mean_function.output_dim == 2


def test_one_mean_set_per_change_and_one_mean_grad_per_evaluation(stand_in):
    lin, con = M.Linear(3, 2), M.Constant(3, 2)
    m = _model(M.Additive(lin, con))
    h = m._h
    assert h.count("mean_set") == 0 and h.count("set_data") == 1
    m.log_likelihood()
    assert h.count("mean_set") == 1 and h.count("fit") == 1
    m.log_likelihood()
    assert h.count("mean_set") == 1                              # nothing changed: nothing sent
    sent = [c for c in h.calls if c[0] == "mean_set"][-1]
    assert np.array_equal(sent[1], lin.A_matrix) and np.array_equal(sent[2], [0.0, 0.0])
    x = m.optimizer_array.copy()
    for k in range(3):
        x[0] += 0.1
        before = (h.count("mean_set"), h.count("mean_grad"), h.count("fit_grad"))
        f, g = m._obj_grad(x)
        assert (h.count("mean_set"), h.count("mean_grad"), h.count("fit_grad")) == tuple(b + 1 for b in before)
        assert g.size == 11 and f == 1.0
    sent = [c for c in h.calls if c[0] == "mean_set"][-1]
    assert sent[1][0, 0] == x[0]
    # a Linear alone sends no b, a Constant alone no A
    for mean, has in ((M.Linear(3, 2), (True, False)), (M.Constant(3, 2, 1.0), (False, True))):
        mm = _model(mean)
        mm.log_likelihood()
        s = [c for c in mm._h.calls if c[0] == "mean_set"][-1]
        assert ((s[1] is not None), (s[2] is not None)) == has


def test_no_mean_function_no_mean_calls(stand_in):
    m = _model(None)
    m.log_likelihood()
    m._obj_grad(m.optimizer_array + 0.1)
    assert m.gradient.size == 3
    assert m._h.count("mean_set") == 0 and m._h.count("mean_grad") == 0 and m.mean_function is None


def test_mean_acts_on_the_normalised_targets(stand_in):
    m = _model(M.Constant(3, 2, 1.0), normalizer=True)
    Y = [c for c in m._h.calls if c[0] == "set_data"][-1][2]
    assert np.allclose(Y.mean(0), 0.0, atol=1e-12) and np.allclose(Y.std(0), 1.0)      # the handle (and so the mean) sees normalised Y


def test_lockstep_and_append_fall_back(stand_in):
    m = _model(M.Linear(3, 2))
    assert m._lockstep_applies(4) is False and _model(None)._lockstep_applies(4) is True
    m.log_likelihood()
    n = m._h.count("set_data")
    m.append_XY(np.full((1, 3), 0.5), np.vstack([m.Y, np.zeros((1, 2))]))       # refits: set_data, never append
    assert m._h.count("set_data") == n + 1 and m.num_data == 7
    with pytest.raises(NotImplementedError):
        m._device_group((0, 0))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_other_mappings_are_refused(stand_in):
    with pytest.raises(NotImplementedError):
        _model(_Other(3, 2))
    with pytest.raises(NotImplementedError):
        _model(M.Additive(M.Linear(3, 2), _Other(3, 2)))
    with pytest.raises(AssertionError):
        _model(M.Linear(2, 2))                                    # the reference's asserts on input_dim / output_dim
    with pytest.raises(AssertionError):
        _model(M.Linear(3, 1))
    with pytest.raises(AssertionError):
        _model(object())


@pytest.mark.parametrize("cls", ["InputWarpedGP", "WarpedGP", "SparseGPRegression"])
def test_the_three_model_classes_refuse_a_mean_function(stand_in, cls):
    rng = np.random.default_rng(2)
    X, Y = rng.uniform(0, 1, (6, 2)), rng.standard_normal((6, 1))
    with pytest.raises(NotImplementedError):
        getattr(gpo.models, cls)(X, Y, mean_function=M.Linear(2, 1))


def test_gpmodel_surface(stand_in):
    with pytest.raises(NotImplementedError):
        gpo.GPModel(sparse=True, mean_function=M.Linear(2, 1))
    with pytest.raises(NotImplementedError):
        gpo.GPModel_MCMC(mean_function=M.Linear(2, 1))
    lin = M.Linear(2, 1)
    gm = gpo.GPModel(mean_function=lin, max_iters=0, verbose=False)
    rng = np.random.default_rng(3)
    gm.updateModel(rng.uniform(0, 1, (5, 2)), rng.standard_normal((5, 1)), None, None)
    assert gm.model.mean_function is lin and len(gm.get_model_parameters_names()) == 2 + 3
    # entropy search keeps the host route with a mean function
    es = A.AcquisitionEntropySearch.__new__(A.AcquisitionEntropySearch)
    es.device, es.model = True, gm
    assert es._es_device_ok() is False
