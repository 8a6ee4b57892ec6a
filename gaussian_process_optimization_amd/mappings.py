"""Mean-function mappings -- host mirror of ``GPy.mappings`` as far as the device takes them.

Reference: GPy/GPy/core/mapping.py (``Mapping``), GPy/GPy/mappings/linear.py (``Linear``: F(X) = X A), constant.py
(``Constant``: F(X) = C) and additive.py (``Additive``: the sum of two mappings).  ``GPRegression(mean_function=...)`` takes
exactly these: an affine trend m(x) = x^T A + b, which the handle keeps resident (``gp_mean_set``) and adds on the device
wherever a posterior mean is formed.  Their parameters are unconstrained (paramz' ``Param`` without a transform).
"""
import numpy as np

from .parameterization import Param, Parameterized
from .warping_functions import _Free


class Mapping(Parameterized):
    """A parametric map from ``input_dim`` to ``output_dim`` columns (core/mapping.py:9-27)."""

    def __init__(self, input_dim, output_dim, name='mapping'):
        self.input_dim = int(input_dim)
        self.output_dim = int(output_dim)
        super(Mapping, self).__init__(name)

    def f(self, X):
        raise NotImplementedError

    def gradients_X(self, dL_dF, X):
        raise NotImplementedError

    def update_gradients(self, dL_dF, X):
        raise NotImplementedError


class Linear(Mapping):
    """F(X) = X A with A [input_dim, output_dim], drawn from N(0, 1) as the reference draws it (linear.py:27-30)."""

    def __init__(self, input_dim, output_dim, name='linmap'):
        super(Linear, self).__init__(input_dim, output_dim, name)
        self.A = Param('A', np.random.randn(self.input_dim, self.output_dim), _Free())
        self.link_parameter(self.A)

    @property
    def A_matrix(self):
        """``A`` as [input_dim, output_dim] (the parameter itself is flat)."""
        return self.A.values.reshape(self.input_dim, self.output_dim)

    def f(self, X):
        return np.dot(np.asarray(X, dtype=float), self.A_matrix)

    def update_gradients(self, dL_dF, X):
        self.A.gradient = np.dot(np.asarray(X, dtype=float).T, dL_dF).reshape(-1)

    def gradients_X(self, dL_dF, X):
        return np.dot(dL_dF, self.A_matrix.T)

    def copy(self):
        state = np.random.get_state()     # (a copy draws nothing from the global generator)
        twin = Linear(self.input_dim, self.output_dim, self.name)
        np.random.set_state(state)
        twin.A._v[:] = self.A.values
        return twin


class Constant(Mapping):
    """F(X) = C, one value per output (constant.py:22-40); a scalar ``value`` fills every output."""

    def __init__(self, input_dim, output_dim, value=0., name='constmap'):
        super(Constant, self).__init__(input_dim, output_dim, name)
        value = np.atleast_1d(np.asarray(value, dtype=float))
        if value.ndim != 1:
            raise ValueError("bad constant values: pass a float or a flat vector")
        if value.size == 1:
            value = np.ones(self.output_dim) * value
        self.C = Param('C', value, _Free())
        self.link_parameter(self.C)

    def f(self, X):
        return np.tile(self.C.values[None, :], (np.asarray(X).shape[0], 1))

    def update_gradients(self, dL_dF, X):
        self.C.gradient = np.asarray(dL_dF, dtype=float).sum(0)

    def gradients_X(self, dL_dF, X):
        return np.zeros_like(np.asarray(X, dtype=float))

    def copy(self):
        return Constant(self.input_dim, self.output_dim, self.C.values.copy(), self.name)


class Additive(Mapping):
    """F(X) = F1(X) + F2(X) (additive.py:22-39)."""

    def __init__(self, mapping1, mapping2):
        assert mapping1.input_dim == mapping2.input_dim
        assert mapping1.output_dim == mapping2.output_dim
        super(Additive, self).__init__(mapping1.input_dim, mapping1.output_dim)
        self.mapping1 = mapping1
        self.mapping2 = mapping2
        self.link_parameters(self.mapping1, self.mapping2)

    def f(self, X):
        return self.mapping1.f(X) + self.mapping2.f(X)

    def update_gradients(self, dL_dF, X):
        self.mapping1.update_gradients(dL_dF, X)
        self.mapping2.update_gradients(dL_dF, X)

    def gradients_X(self, dL_dF, X):
        return self.mapping1.gradients_X(dL_dF, X) + self.mapping2.gradients_X(dL_dF, X)

    def copy(self):
        return Additive(self.mapping1.copy(), self.mapping2.copy())


def check_affine(mapping):
    """Raise ``NotImplementedError`` unless ``mapping`` is a ``Linear``, a ``Constant`` or an ``Additive`` of those: the
    mappings the device's mean function m(x) = x^T A + b can represent."""
    if isinstance(mapping, Additive):
        check_affine(mapping.mapping1)
        check_affine(mapping.mapping2)
    elif not isinstance(mapping, (Linear, Constant)):
        raise NotImplementedError("the accelerated path takes mappings.Linear, mappings.Constant or an Additive of those as "
                                  "the mean function; got %s" % type(mapping).__name__)


def affine_parts(mapping):
    """(A [D, P] or None, b [P] or None) of an affine mapping: what ``Handle.mean_set`` takes."""
    if isinstance(mapping, Linear):
        return mapping.A_matrix.copy(), None
    if isinstance(mapping, Constant):
        return None, mapping.C.values.copy()
    (A1, b1), (A2, b2) = affine_parts(mapping.mapping1), affine_parts(mapping.mapping2)
    return (A1 if A2 is None else A2 if A1 is None else A1 + A2), (b1 if b2 is None else b2 if b1 is None else b1 + b2)


def set_affine_gradients(mapping, dA, db):
    """``update_gradients`` from the device's sums dL/dA = X^T alpha and dL/db = 1^T alpha (``Handle.mean_grad``): every
    ``Linear`` below ``mapping`` takes dA, every ``Constant`` db, as ``Additive.update_gradients`` hands dL_dF to both parts."""
    if isinstance(mapping, Linear):
        mapping.A.gradient = np.asarray(dA, dtype=float).reshape(-1).copy()
    elif isinstance(mapping, Constant):
        mapping.C.gradient = np.asarray(db, dtype=float).reshape(-1).copy()
    else:
        set_affine_gradients(mapping.mapping1, dA, db)
        set_affine_gradients(mapping.mapping2, dA, db)
