"""Black-box constraints: ``FeasibilityModel`` -- one exact GP per constraint, and the probability that a location satisfies
them all (Gardner et al. 2014; Gelbart et al. 2014).

A constraint ``c_k(x) <= bounds[k]`` is known only through evaluations.  ``update(X, C)`` fits GP ``k`` to column ``k`` of ``C``
(standardised per column); the probability of feasibility is

    F(x) = prod_k Phi((bounds[k] - m_k(x)) / s_k(x)),

``m_k`` / ``s_k`` the predictive mean and standard deviation of constraint ``k`` (likelihood noise included, the variance
clipped at 1e-10 as the acquisitions clip theirs).  Everything is carried as ``log F``: a location far inside the infeasible side
keeps a finite value and a usable gradient  ``sum_k lambda(z_k) (-dm_k - z_k ds_k) / s_k``,  ``lambda = phi / Phi``.

EI and MPI take a model with ``feasibility=``: the acquisition becomes ``a(x) F(x)`` with the incumbent over the FEASIBLE
observations, scored on the device (``gp_feas_table`` + ``GP_ACQ_TIMES_FEAS`` for tables, ``gp_acq_rows_feas`` for the
optimiser's calls); while no observation is feasible the rule is the probability of feasibility alone (``GP_ACQ_POF``).
``generation`` tells the routes when a cached table is stale.

A constraint known only as a yes / no -- the simulation diverged, the build failed -- is a BINARY column (``kinds``): it holds 1
where the constraint was violated and 0 where it was satisfied, is not standardised (c_mean 0, c_std 1), has bound 0, and its
model is a ``GPClassModel`` (probit classifier, Laplace fit).  That model answers with the latent mean m and sqrt(s^2 + 1), so
``Phi((0 - m) / sqrt(s^2 + 1))`` -- the very term above -- is the probability that the constraint is satisfied, and the device
fold takes the classifier's handle as it takes a regression handle.

When every constraint model is our exact ``GPModel`` (or ``GPClassModel``) on one device ``log_probability`` runs through ``gp_feas_rows``; otherwise
(a foreign model) the same formulas run in NumPy on top of ``predict_withGradients`` -- which is also the host comparator of the
device route (``host=True``).
"""
import numpy as np
from scipy.special import log_ndtr

from . import _lib
from . import gpmodel as _gpmodel
from .gpmodel import GPModel, GPClassModel

_VAR_FLOOR = 1e-10
_HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)


def _normaliser(gp):
    nz = getattr(gp, "normalizer", None)
    return (0.0, 1.0) if nz is None else (float(nz.mean[0]), float(nz.std[0]))


class FeasibilityModel(object):
    """``num_constraints`` constraint GPs (``GPModel(device=device, **gpmodel_kwargs)`` each; ``models`` may be replaced by any
    objects with ``updateModel`` and ``predict_withGradients``), upper bounds ``bounds`` (a scalar or one per constraint).
    ``kinds``: per column ``'value'`` (the default: a real-valued ``c_k(x) <= bounds[k]``) or ``'binary'`` (1 = violated, 0 =
    satisfied; bound 0, no standardisation, a ``GPClassModel``)."""

    _CLASS_KWARGS = ("optimizer", "max_iters", "optimize_restarts", "verbose", "ARD")

    def __init__(self, num_constraints, bounds=0.0, kinds=None, device=0, **gpmodel_kwargs):
        K = int(num_constraints)
        if not 1 <= K <= _lib.GP_FEAS_MAX:
            raise ValueError("between 1 and %d constraints, got %r" % (_lib.GP_FEAS_MAX, num_constraints))
        if gpmodel_kwargs.get("sparse", False):
            raise NotImplementedError("a constraint model is an exact GP: sparse=True is not available")
        self.num_constraints = K
        self.bounds = np.broadcast_to(np.asarray(bounds, dtype=float), (K,)).copy()
        if not np.all(np.isfinite(self.bounds)):
            raise ValueError("the bounds must be finite")
        if kinds is None:
            kinds = ('value',) * K
        if isinstance(kinds, str):
            kinds = (kinds,) * K
        self.kinds = tuple(kinds)
        if len(self.kinds) != K or any(k not in ('value', 'binary') for k in self.kinds):
            raise ValueError("kinds takes 'value' or 'binary' for each of the %d constraints, got %r" % (K, kinds))
        self.binary = np.array([k == 'binary' for k in self.kinds])
        self.bounds[self.binary] = 0.0       # a binary column's bound is 0 on the latent scale
        self.device = device
        class_kwargs = {k: v for k, v in gpmodel_kwargs.items() if k in self._CLASS_KWARGS}
        self.models = [GPClassModel(device=device, **class_kwargs) if b else GPModel(device=device, **gpmodel_kwargs)
                       for b in self.binary]
        self.generation = 0
        self.c_mean, self.c_std = np.zeros(K), np.ones(K)
        self.feasible_rows = np.empty(0, dtype=np.int64)
        self.num_rows = 0
        self._pack = None

    # ---- data ------------------------------------------------------------------------------------------------------------
    def feasible(self, C):
        """Row mask: every constraint value within its bound."""
        C = np.atleast_2d(np.asarray(C, dtype=float))
        if C.shape[1] != self.num_constraints:
            raise ValueError("expected %d constraint columns, got %d" % (self.num_constraints, C.shape[1]))
        self._check_binary(C)
        return np.all(np.where(self.binary, C == 0.0, C <= self.bounds), axis=1)

    def _check_binary(self, C):
        if self.binary.any() and not np.all((C[:, self.binary] == 0.0) | (C[:, self.binary] == 1.0)):
            raise ValueError("a binary constraint column holds 1 (violated) or 0 (satisfied)")

    def violation(self, C):
        """How far each row is from feasibility: the sum over the constraints of max(c_k - bounds[k], 0) in units of column k's
        standard deviation over the rows of ``C`` (0 for a feasible row); a binary column adds its label, 1 where violated.  THE
        definition of 'least violating' (``BayesianOptimization`` reports the row that minimises it while no observation is
        feasible)."""
        C = np.atleast_2d(np.asarray(C, dtype=float))
        self._check_binary(C)
        std = C.std(axis=0)
        value = np.maximum(C - self.bounds, 0.0) / np.where(std > 0, std, 1.0)
        return np.where(self.binary, C, value).sum(axis=1)

    def update(self, X, C):
        """Fit constraint GP k to (X, standardised C[:, k]) and move ``generation``; ``feasible_rows`` are the rows of X (the
        scored model's training rows) that satisfy every constraint."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        C = np.atleast_2d(np.asarray(C, dtype=float))
        if C.shape != (X.shape[0], self.num_constraints):
            raise ValueError("expected constraint values [%d, %d], got %s" % (X.shape[0], self.num_constraints, C.shape))
        self._check_binary(C)
        mean, std = C.mean(axis=0), C.std(axis=0)
        std = np.where(std > 0, std, 1.0)
        mean, std = np.where(self.binary, 0.0, mean), np.where(self.binary, 1.0, std)   # labels are not standardised
        for k, m in enumerate(self.models):
            m.updateModel(X, ((C[:, k] - mean[k]) / std[k])[:, None], None, None)
        self.c_mean, self.c_std = mean, std
        self.feasible_rows = np.flatnonzero(self.feasible(C)).astype(np.int64)
        self.num_rows = X.shape[0]
        self._pack = None
        self.generation += 1

    # ---- where it runs -----------------------------------------------------------------------------------------------------
    def _device_models(self, device=None):
        """True when every constraint model is our exact GPModel or GPClassModel, fitted, one output, on one device (``device``
        when given)."""
        dev = self.models[0].device if device is None else device
        for m in self.models:
            if type(m) not in (_gpmodel.GPModel, _gpmodel.GPClassModel) or m.sparse or m.model is None or m.device != dev:
                return False
            if m.model.output_dim != 1 or not hasattr(m.model.kern, "_kernel_id"):
                return False
        return self.generation > 0

    def device_pack(self, device=None):
        """The ``_lib.FeasPack`` of the current generation (handles fitted), or None when the constraints are scored on the host."""
        if not self._device_models(device):
            return None
        for m in self.models:
            m.model._ensure_fit()
        if self._pack is None or self._pack[0] != self.generation:
            shift, scale = zip(*[_normaliser(m.model) for m in self.models])
            c_std = self.c_std * np.array(scale)
            c_mean = self.c_mean + self.c_std * np.array(shift)
            self._pack = (self.generation, _lib.FeasPack([m.model._h for m in self.models], self.bounds, c_mean, c_std))
        return self._pack[1]

    # ---- log F -------------------------------------------------------------------------------------------------------------
    def log_probability(self, x, host=False):
        """log F [M] at the rows of ``x``."""
        x = np.atleast_2d(np.asarray(x, dtype=float))
        pack = None if host else self.device_pack()
        if pack is not None:
            return pack.rows(x)
        return self._host(x, False)[0]

    def log_probability_withGradients(self, x, host=False):
        """(log F [M], d log F / dx [M, D])."""
        x = np.atleast_2d(np.asarray(x, dtype=float))
        pack = None if host else self.device_pack()
        if pack is not None:
            return pack.rows(x, grad=True)
        return self._host(x, True)

    def _host(self, x, grad):
        """The formulas of csrc/acq_math.h (feas_terms, feas_grad) in NumPy on top of ``predict_withGradients``."""
        if self.generation < 1:
            raise RuntimeError("FeasibilityModel.update first")
        logF = np.zeros(x.shape[0])
        dlogF = np.zeros(x.shape) if grad else None
        for k, model in enumerate(self.models):
            mean, sd, dmean, dsd = model.predict_withGradients(x)
            cs = self.c_std[k]
            m = np.ravel(mean) * cs + self.c_mean[k]
            v = np.maximum((np.ravel(sd) * cs) ** 2, _VAR_FLOOR)
            s = np.sqrt(v)
            z = (self.bounds[k] - m) / s
            t = log_ndtr(z)
            logF = t if k == 0 else logF + t
            if grad:
                lam = np.exp(-0.5 * z * z - _HALF_LOG_2PI - t)
                dm = cs * np.asarray(dmean).reshape(x.shape)
                # (d sd / dx of the model is d var / dx / (2 sd): the same quantity the device forms from d var / dx)
                ds = cs * np.asarray(dsd).reshape(x.shape) * (np.ravel(sd) * cs / s)[:, None]
                g = (lam / s)[:, None] * (-dm - z[:, None] * ds)
                dlogF = g if k == 0 else dlogF + g
        return logF, dlogF
