"""Multi-objective Bayesian optimisation: expected hypervolume improvement (EHVI) over K = 2 or 3 objectives, all minimised.

Each objective has an exact GP of its own; the objectives are taken as independent.  With ``r`` the reference point and the part of
``(-inf, r]`` that the observed Pareto front does not dominate cut into axis-parallel cells ``[l_c, u_c]`` (``l_ck = -inf`` allowed),
the hypervolume improvement of an outcome ``y`` is ``sum_c prod_k [(u_ck - y_k)^+ - (l_ck - y_k)^+]`` and its expectation has the
closed form (Emmerich et al. 2011; Yang et al. 2019)

    EHVI(x) = sum_c prod_k (Psi_k(u_ck) - Psi_k(l_ck)),   Psi_k(c) = s_k (z Phi(z) + phi(z)),  z = (c - m_k) / s_k,  Psi_k(-inf) = 0,

``m_k`` / ``s_k`` the predictive mean and standard deviation of objective ``k`` (likelihood noise included, the variance clipped at
1e-10 as the acquisitions clip theirs).  ``Psi`` is EI with incumbent ``c`` and no jitter, so ``d Psi / dm = -Phi`` and
``d Psi / ds = phi`` give the gradient.

``nondominated_cells`` builds the decomposition on the host -- K = 2: the n + 1 strips between the front's points sorted by the
first objective; K = 3: slabs along the third objective, each carrying the strips of the projected front of the points below it,
at most (n + 1)(n + 2) / 2 cells -- as K sorted level arrays and index pairs into them, the layout ``gp_ehvi_set`` takes.
``AcquisitionEHVI`` scores on the device when every objective model is our exact ``GPModel`` on one device (``gp_ehvi_table`` /
``_argbest`` / ``_topk`` for tables, ``gp_ehvi_rows`` for the optimiser's calls); otherwise the same formulas run in NumPy on top
of ``predict_withGradients`` -- which is also the host comparator of the device route (``host=True``).
``MultiObjectiveBayesianOptimization`` is the loop around it.
"""
import copy
import time

import numpy as np
from scipy.special import erfc

from . import _lib
from . import gpmodel as _gpmodel
from .acquisitions import _FEW_ROWS, _host_topk, _pick, _Unconstrained
from .bayesian_optimization import AcquisitionOptimizer, Design_space, kernel_from_name
from .cost import constant_cost_withGradients
from .gpmodel import GPModel

_VAR_FLOOR = 1e-10
_ROOT_2 = np.sqrt(2.0)
_ROOT_2PI = np.sqrt(2.0 * np.pi)
MAX_OBJECTIVES = _lib.GP_EHVI_MAX_OBJ
MAX_FRONT_VALUES = _lib.GP_EHVI_MAX_LEVELS - 2      # distinct front values per axis: the levels also hold -inf and r_k
MAX_CELLS = _lib.GP_EHVI_MAX_CELLS


def _objectives(Y, ref=None):
    """``Y`` as outcomes [n, K] (and ``ref`` as a reference point [K]); no rows is n = 0 with K from ``ref`` (or 2)."""
    Y = np.asarray(Y, dtype=float)
    if ref is not None:
        ref = np.asarray(ref, dtype=float).ravel()
    if Y.size == 0:
        Y = np.empty((0, Y.shape[1] if Y.ndim == 2 and Y.shape[1] else (2 if ref is None else ref.size)))
    Y = np.atleast_2d(Y)
    if Y.ndim != 2 or not 2 <= Y.shape[1] <= MAX_OBJECTIVES:
        raise ValueError("expected outcomes [n, K] with K = 2 or %d, got shape %s" % (MAX_OBJECTIVES, Y.shape))
    if ref is None:
        return Y
    if ref.size != Y.shape[1] or not np.all(np.isfinite(ref)):
        raise ValueError("the reference point takes one finite entry per objective (%d), got %r" % (Y.shape[1], ref))
    return Y, ref


def pareto_front(Y, return_index=False):
    """The non-dominated rows of ``Y`` [n, K] (minimisation), duplicates once, sorted lexicographically; with ``return_index``
    also a row of ``Y`` each came from."""
    Y = _objectives(Y)
    if Y.shape[0] == 0:
        return (Y, np.empty(0, dtype=np.int64)) if return_index else Y
    U, first = np.unique(Y, axis=0, return_index=True)
    le = np.all(U[:, None, :] <= U[None, :, :], axis=2)       # le[i, j]: row i is nowhere worse than row j
    lt = np.any(U[:, None, :] < U[None, :, :], axis=2)
    keep = ~np.any(le & lt, axis=0)
    return (U[keep], first[keep]) if return_index else U[keep]


def _hv2(P, ref):
    """Area dominated by the rows of ``P`` [n, 2] (every row strictly below ``ref``) inside (-inf, ref]."""
    if P.shape[0] == 0:
        return 0.0
    P = P[np.lexsort((P[:, 1], P[:, 0]))]
    area, low = 0.0, ref[1]
    for a, b in P:
        if b < low:
            area += (ref[0] - a) * (low - b)
            low = b
    return area


def hypervolume(Y, ref):
    """The hypervolume the rows of ``Y`` [n, K] dominate inside (-inf, ref], K = 2 or 3 (minimisation).  Rows that are not strictly
    below ``ref`` in every objective contribute nothing."""
    Y, ref = _objectives(Y, ref)
    P = Y[np.all(Y < ref, axis=1)]
    if P.shape[1] == 2:
        return _hv2(P, ref)
    P = P[np.argsort(P[:, 2], kind="stable")]
    edges = np.append(P[:, 2], ref[2])
    vol = 0.0
    for j in range(P.shape[0]):
        if edges[j + 1] > edges[j]:
            vol += (edges[j + 1] - edges[j]) * _hv2(P[:j + 1, :2], ref[:2])
    return vol


def _strips(P, ref, la, lb):
    """The strips of the region (-inf, ref] minus what the 2-D front ``P`` dominates, as index pairs into the level arrays ``la``,
    ``lb`` (entry 0 of each: -inf; the last: ref): lists (lo_a, lo_b), (hi_a, hi_b)."""
    F = pareto_front(P)                                # sorted by the first objective, the second strictly decreasing
    ia = np.concatenate(([0], np.searchsorted(la[1:], F[:, 0]) + 1, [la.size - 1]))
    ib = np.concatenate(([lb.size - 1], np.searchsorted(lb[1:], F[:, 1]) + 1))
    n = F.shape[0]
    return [(ia[i], 0) for i in range(n + 1)], [(ia[i + 1], ib[i]) for i in range(n + 1)]


def nondominated_cells(Y, ref):
    """The cell decomposition of the part of (-inf, ref] that the rows of ``Y`` [n, K] do not dominate, K = 2 or 3:
    ``(levels, cell_lo, cell_hi)`` -- ``levels`` a list of K increasing arrays (entry 0 is -inf, then the front's distinct values
    below ``ref[k]``, then ``ref[k]``), ``cell_lo`` / ``cell_hi`` [C, K] indices into them with lo < hi.  ``ValueError`` names the
    cap when an axis has more than ``MAX_FRONT_VALUES`` distinct front values or there are more than ``MAX_CELLS`` cells."""
    Y, ref = _objectives(Y, ref)
    K = ref.size
    F = pareto_front(Y[np.all(Y < ref, axis=1)])
    levels = []
    for k in range(K):
        vals = np.unique(F[:, k])
        if vals.size > MAX_FRONT_VALUES:
            raise ValueError("objective %d: %d distinct front values, more than the %d the device takes per axis "
                             "(GP_EHVI_MAX_LEVELS = %d levels with -inf and the reference)"
                             % (k, vals.size, MAX_FRONT_VALUES, _lib.GP_EHVI_MAX_LEVELS))
        levels.append(np.concatenate(([-np.inf], vals, [ref[k]])))
    if K == 2:
        lo, hi = _strips(F, ref, levels[0], levels[1])
    else:
        lo, hi = [], []
        lz = levels[2]
        for j in range(lz.size - 1):                     # slab [lz[j], lz[j + 1]]: the points at or below its lower edge
            slo, shi = _strips(F[F[:, 2] <= lz[j], :2], ref[:2], levels[0], levels[1])
            lo += [s + (j,) for s in slo]
            hi += [s + (j + 1,) for s in shi]
            if len(lo) > MAX_CELLS:
                break
    if len(lo) > MAX_CELLS:
        raise ValueError("more than %d cells (GP_EHVI_MAX_CELLS): thin the front or move the reference point" % MAX_CELLS)
    return levels, np.array(lo, dtype=np.intc).reshape(-1, K), np.array(hi, dtype=np.intc).reshape(-1, K)


def hypervolume_improvement_from_cells(y, levels, cell_lo, cell_hi):
    """sum_c prod_k [(u_ck - y_k)^+ - (l_ck - y_k)^+] for one outcome ``y`` [K]: the hypervolume the front gains with it."""
    total = 0.0
    for lo, hi in zip(cell_lo, cell_hi):
        p = 1.0
        for k, yk in enumerate(np.asarray(y, dtype=float).ravel()):
            low = levels[k][lo[k]]
            p *= max(levels[k][hi[k]] - yk, 0.0) - (max(low - yk, 0.0) if np.isfinite(low) else 0.0)
        total += p
    return total


def ehvi_host(m, s, levels, cell_lo, cell_hi, grad=False):
    """The formulas of csrc/acq_math.h (ehvi_level) and csrc/ehvi.hip in NumPy: ``m``, ``s`` [K, M] the un-normalised predictive
    mean and (clipped) standard deviation.  Returns EHVI [M] and, with ``grad``, the partials G_m, G_s [K, M]."""
    K, M = m.shape
    psi, Phi, phi = [], [], []
    for k in range(K):
        c = levels[k][1:, None]
        z = (c - m[k][None, :]) / s[k][None, :]
        p = np.exp(-0.5 * z * z) / _ROOT_2PI
        P = 0.5 * erfc(-z / _ROOT_2)
        zero = np.zeros((1, M))
        psi.append(np.vstack((zero, s[k][None, :] * (z * P + p))))
        Phi.append(np.vstack((zero, P)))
        phi.append(np.vstack((zero, p)))
    d = [psi[k][cell_hi[:, k]] - psi[k][cell_lo[:, k]] for k in range(K)]       # [C, M] each
    value = np.prod(d, axis=0).sum(axis=0)
    if not grad:
        return value
    Gm, Gs = np.empty((K, M)), np.empty((K, M))
    for k in range(K):
        others = np.prod([d[j] for j in range(K) if j != k], axis=0)
        Gm[k] = (others * (Phi[k][cell_lo[:, k]] - Phi[k][cell_hi[:, k]])).sum(axis=0)
        Gs[k] = (others * (phi[k][cell_hi[:, k]] - phi[k][cell_lo[:, k]])).sum(axis=0)
    return value, Gm, Gs


def _normaliser(gp):
    nz = getattr(gp, "normalizer", None)
    return (0.0, 1.0) if nz is None else (float(nz.mean[0]), float(nz.std[0]))


class AcquisitionEHVI(object):
    """Expected hypervolume improvement of K = 2 or 3 objective models (``models``: a list of ``GPModel``s, or any objects with
    ``predict_withGradients``) over ``reference_point``.  ``set_front(Y, y_mean, y_std)`` gives it the observed outcomes (raw
    units) and the standardisation the models were fitted under (model k saw ``(Y[:, k] - y_mean[k]) / y_std[k]``).

    ``acquisition_function`` returns the NEGATED value [M, 1] as every acquisition here does, ``acquisition_function_withGradients``
    its x-gradient [M, D] as well; ``argbest`` / ``topk`` rank a table; ``optimize`` hands it to the acquisition optimiser
    (``parallel_anchors=True`` works: the rows entry has gradients and a row does not depend on its company).  When every model
    is our exact single-output ``GPModel``, fitted, on one device, all of it runs on the device; ``host=True`` forces the NumPy
    rule.  Not available: a cost model, black-box constraints (``feasibility=``), local penalisation."""
    analytical_gradient_prediction = True
    analytical_gradient_acq = True
    _per_cost = False
    _rule = None
    _takes_no_penaliser = ("expected hypervolume improvement has no penalised batches: the penaliser's exclusion balls are built "
                           "from one objective's Lipschitz constant")

    def __init__(self, models, space=None, optimizer=None, reference_point=None, cost_withGradients=None, feasibility=None):
        models = list(models)
        if not 2 <= len(models) <= MAX_OBJECTIVES:
            raise ValueError("between 2 and %d objective models, got %d" % (MAX_OBJECTIVES, len(models)))
        if cost_withGradients is not None and cost_withGradients is not constant_cost_withGradients:
            raise NotImplementedError("expected hypervolume improvement takes no cost model: EHVI per unit of cost is not "
                                      "implemented")
        if feasibility is not None:
            raise NotImplementedError("expected hypervolume improvement takes no black-box constraints: EHVI times the "
                                      "probability of feasibility is not implemented")
        if reference_point is None:
            raise ValueError("reference_point is needed: one entry per objective")
        self.models = models
        self.model = models[0]
        self.num_objectives = K = len(models)
        self.space = _Unconstrained() if space is None else space
        self.optimizer = optimizer
        self.reference_point = np.asarray(reference_point, dtype=float).ravel().copy()
        if self.reference_point.size != K or not np.all(np.isfinite(self.reference_point)):
            raise ValueError("the reference point takes one finite entry per objective (%d)" % K)
        self.y_mean, self.y_std = np.zeros(K), np.ones(K)
        self.generation = 0
        self.set_front(np.empty((0, K)))
        self._pack = None

    # ---- the front -------------------------------------------------------------------------------------------------------------
    def set_front(self, Y, y_mean=None, y_std=None):
        """The observed outcomes ``Y`` [n, K] in raw units (rows beyond the reference point stay out of the front) and the
        standardisation of the models' targets; moves ``generation``."""
        self.levels, self.cell_lo, self.cell_hi = nondominated_cells(Y, self.reference_point)
        if y_mean is not None:
            self.y_mean = np.asarray(y_mean, dtype=float).ravel().copy()
            self.y_std = np.asarray(y_std, dtype=float).ravel().copy()
            if self.y_mean.size != self.num_objectives or self.y_std.size != self.num_objectives or not np.all(self.y_std > 0):
                raise ValueError("y_mean and y_std take one entry per objective, y_std positive")
        self.generation += 1

    # ---- where it runs -----------------------------------------------------------------------------------------------------------
    def _device_models(self):
        dev = getattr(self.models[0], "device", None)
        for m in self.models:
            if type(m) is not _gpmodel.GPModel or m.sparse or m.model is None or m.device != dev:
                return False
            if m.model.output_dim != 1 or not hasattr(m.model.kern, "_kernel_id"):
                return False
        return True

    def device_pack(self):
        """The ``_lib.EhviPack`` with the current decomposition resident on the scored handle (the handles fitted), or None when
        the acquisition is scored on the host."""
        if not self._device_models():
            return None
        gps = [m.model for m in self.models]
        for gp in gps:
            gp._ensure_fit()
        shift, scale = (np.array(v) for v in zip(*[_normaliser(gp) for gp in gps]))
        key = (self.generation, tuple(id(gp._h) for gp in gps), tuple(shift), tuple(scale))
        if self._pack is None or self._pack[0] != key:
            pack = _lib.EhviPack([gp._h for gp in gps], self.y_mean + self.y_std * shift, self.y_std * scale)
            pack.set_cells(self.levels, self.cell_lo, self.cell_hi)
            self._pack = (key, pack)
        return self._pack[1]

    def _locations(self, x):
        x = np.asarray(x, dtype=float)
        return x if x.ndim == 2 else np.atleast_2d(x)

    def _indicator(self, x):
        constrained = getattr(self.space, "has_constraints", None)
        return self.space.indicator_constraints(x) if constrained is not None and constrained() else None

    def _table(self, x):
        pack = self.device_pack()
        if pack is not None:
            self.models[0].model._stage(x)
        return pack

    # ---- the contract ----------------------------------------------------------------------------------------------------------
    def acquisition_function(self, x, host=False):
        """-EHVI(x) [M, 1]."""
        x = self._locations(x)
        pack = None if host else (self.device_pack() if x.shape[0] <= _FEW_ROWS else self._table(x))
        if pack is None:
            f = self._host(x, False)
        else:
            f = pack.rows(x) if x.shape[0] <= _FEW_ROWS else pack.table()
        ind = self._indicator(x)
        return f if ind is None else f * ind

    def acquisition_function_withGradients(self, x, host=False):
        """(-EHVI(x) [M, 1], -d EHVI / dx [M, D])."""
        x = self._locations(x)
        pack = None if host else self.device_pack()
        f, df = self._host(x, True) if pack is None else pack.rows(x, grad=True)
        ind = self._indicator(x)
        return (f, df) if ind is None else (f * ind, df * ind)

    def argbest(self, x, sense=-1, exclude=(), devices=None):
        """Row index and value of the best entry of ``acquisition_function(x)`` (sense=-1: the largest EHVI), the rows of
        ``exclude`` out of the running.  Ties -> lowest index."""
        if devices is not None:
            raise NotImplementedError("replica groups score one objective: expected hypervolume improvement runs on one device")
        x = self._locations(x)
        pack = self._table(x) if self._indicator(x) is None else None
        if pack is not None:
            return pack.argbest(sense, exclude)
        v = self.acquisition_function(x)[:, 0].copy()
        v[list(exclude)] = np.inf if sense < 0 else -np.inf
        return _pick(v, sense)

    def topk(self, x, k, sense=-1, devices=None):
        if devices is not None:
            raise NotImplementedError("replica groups score one objective: expected hypervolume improvement runs on one device")
        x = self._locations(x)
        pack = self._table(x) if (self._indicator(x) is None and k <= 64) else None
        if pack is not None:
            return pack.topk(sense, k)
        return _host_topk(self.acquisition_function(x)[:, 0], k, sense)

    def optimize(self, duplicate_manager=None):
        return self.optimizer.optimize(f=self.acquisition_function, f_df=self.acquisition_function_withGradients,
                                       duplicate_manager=duplicate_manager)

    # ---- the host rule ---------------------------------------------------------------------------------------------------------
    def _host(self, x, grad):
        K, M = self.num_objectives, x.shape[0]
        m, s = np.empty((K, M)), np.empty((K, M))
        dm, ds = [], []
        for k, model in enumerate(self.models):
            mean, sd, dmean, dsd = model.predict_withGradients(x)
            ys = self.y_std[k]
            m[k] = np.ravel(mean) * ys + self.y_mean[k]
            raw = np.ravel(sd) * ys
            s[k] = np.sqrt(np.maximum(raw ** 2, _VAR_FLOOR))
            if grad:
                dm.append(ys * np.asarray(dmean).reshape(x.shape))
                # (d sd / dx of the model is d var / dx / (2 sd): the same quantity the device forms from d var / dx)
                ds.append(ys * np.asarray(dsd).reshape(x.shape) * (raw / s[k])[:, None])
        if not grad:
            return -ehvi_host(m, s, self.levels, self.cell_lo, self.cell_hi)[:, None]
        value, Gm, Gs = ehvi_host(m, s, self.levels, self.cell_lo, self.cell_hi, grad=True)
        dvalue = np.zeros(x.shape)
        for k in range(K):
            dvalue = dvalue + Gm[k][:, None] * dm[k] + Gs[k][:, None] * ds[k]
        return -value[:, None], -dvalue


class MultiObjectiveBayesianOptimization(object):
    """Bayesian optimisation of ``num_objectives`` = 2 or 3 objectives, all minimised, by expected hypervolume improvement.

    ``f`` returns [n, K]; ``domain`` as for ``BayesianOptimization``.  One ``GPModel`` per objective, fitted to that column
    standardised (the model keywords of ``BayesianOptimization``: ``kernel`` -- a name, or an object copied per model --, ``ARD``,
    ``noise_var``, ``exact_feval``, ``model_optimizer_type``, ``max_iters``, ``optimize_restarts``, ``parallel_restarts``).  The
    default ``reference_point`` is ``max + 0.1 (max - min)`` per objective over the initial design; it is fixed from then on, and
    observations beyond it stay in the data and are left out of the front.  Results: ``pareto_X``, ``pareto_Y``, ``hypervolume``.
    Batches, a cost model, black-box constraints and local penalisation are not available."""

    def __init__(self, f, domain, num_objectives, X=None, Y=None, reference_point=None, initial_design_numdata=5,
                 exact_feval=False, acquisition_optimizer_type='lbfgs', model_update_interval=1, verbosity=False,
                 verbosity_model=False, device=0, parallel_anchors=False, constraints=None, cost_withGradients=None,
                 constraint_function=None, evaluator_type='sequential', batch_size=1, models=None, **kwargs):
        K = int(num_objectives)
        if not 2 <= K <= MAX_OBJECTIVES:
            raise ValueError("between 2 and %d objectives, got %r" % (MAX_OBJECTIVES, num_objectives))
        if cost_withGradients is not None:
            raise NotImplementedError("expected hypervolume improvement takes no cost model")
        if constraint_function is not None:
            raise NotImplementedError("expected hypervolume improvement takes no black-box constraints")
        if evaluator_type == 'local_penalization':
            raise NotImplementedError(AcquisitionEHVI._takes_no_penaliser)
        if evaluator_type not in ('sequential', None) or int(batch_size) != 1:
            raise NotImplementedError("expected hypervolume improvement suggests one location at a time: batches are not available")
        self.f = f
        self.num_objectives = K
        self.space = Design_space(domain, constraints)
        self.model_update_interval = model_update_interval
        self.verbosity = verbosity
        kernel = kwargs.get('kernel', None)

        def kern():
            if isinstance(kernel, str):
                return kernel_from_name(kernel, self.space.dimensionality, ARD=kwargs.get('ARD', False))
            return copy.deepcopy(kernel)

        self.models = list(models) if models is not None else [GPModel(
            kernel=kern(), noise_var=kwargs.get('noise_var', None), exact_feval=exact_feval,
            optimizer=kwargs.get('model_optimizer_type', 'lbfgs'), max_iters=kwargs.get('max_iters', 1000),
            optimize_restarts=kwargs.get('optimize_restarts', 5), verbose=verbosity_model, ARD=kwargs.get('ARD', False),
            space=self.space, device=device, parallel_restarts=kwargs.get('parallel_restarts', False)) for _ in range(K)]
        if len(self.models) != K:
            raise ValueError("expected %d objective models, got %d" % (K, len(self.models)))
        if X is None:
            X = self.space.samples_uniform(initial_design_numdata)
        self.X = np.atleast_2d(np.asarray(X, dtype=float))
        if Y is None:
            if f is None:
                raise ValueError("f=None requires X and Y")
            Y = self._evaluate(self.X)
        self.Y = np.asarray(Y, dtype=float).reshape(self.X.shape[0], -1)
        if self.Y.shape[1] != K:
            raise ValueError("expected outcomes [%d, %d], got %s" % (self.X.shape[0], K, self.Y.shape))
        self.reference_point = self.default_reference_point(self.Y) if reference_point is None else \
            np.asarray(reference_point, dtype=float).ravel().copy()
        self.acquisition_optimizer = AcquisitionOptimizer(self.space, acquisition_optimizer_type, parallel=parallel_anchors)
        self.acquisition = AcquisitionEHVI(self.models, self.space, self.acquisition_optimizer, self.reference_point)
        self.num_acquisitions = 0
        self.suggested_sample = None
        self.cum_time = 0.0

    @staticmethod
    def default_reference_point(Y):
        """max + 0.1 (max - min) per objective over the rows of ``Y`` (a constant column: max + 0.1)."""
        Y = np.atleast_2d(np.asarray(Y, dtype=float))
        top, span = Y.max(axis=0), Y.max(axis=0) - Y.min(axis=0)
        return top + 0.1 * np.where(span > 0, span, 1.0)

    def _evaluate(self, X):
        X = np.atleast_2d(X)
        return np.asarray(self.f(X), dtype=float).reshape(X.shape[0], -1)

    def _update_model(self):
        if self.num_acquisitions % self.model_update_interval == 0:
            mean, std = self.Y.mean(axis=0), self.Y.std(axis=0)
            std = np.where(std > 0, std, 1.0)
            for k, m in enumerate(self.models):
                m.updateModel(self.X, ((self.Y[:, k] - mean[k]) / std[k])[:, None], None, None)
            self.acquisition.set_front(self.Y, mean, std)

    def suggest_next_locations(self):
        self._update_model()
        self.suggested_sample, _ = self.acquisition.optimize()
        return self.suggested_sample

    def run_optimization(self, max_iter=0, max_time=np.inf, verbosity=False):
        """``max_iter`` rounds of refit, suggestion and evaluation; returns ``(pareto_X, pareto_Y)``."""
        if self.f is None:
            raise ValueError("Cannot run the optimization loop without the objective function")
        t0 = time.time()
        it = 0
        while it < max_iter and (time.time() - t0) < max_time:
            try:
                x = self.suggest_next_locations()
            except np.linalg.LinAlgError:
                break
            self.X = np.vstack((self.X, x))
            self.Y = np.vstack((self.Y, self._evaluate(x)))
            self.num_acquisitions += 1
            it += 1
            if verbosity or self.verbosity:
                print("num acquisition: %d, hypervolume: %.6g, time elapsed: %.2fs"
                      % (self.num_acquisitions, self.hypervolume, time.time() - t0))
        self.cum_time = time.time() - t0
        return self.pareto_X, self.pareto_Y

    # ---- results -----------------------------------------------------------------------------------------------------------------
    def _front(self):
        inside = np.flatnonzero(np.all(self.Y < self.reference_point, axis=1))
        F, rows = pareto_front(self.Y[inside].reshape(-1, self.num_objectives), return_index=True)
        return F, inside[rows]

    @property
    def pareto_Y(self):
        """The observed front inside the reference point, [n, K]."""
        return self._front()[0]

    @property
    def pareto_X(self):
        return self.X[self._front()[1]]

    @property
    def hypervolume(self):
        return hypervolume(self.Y, self.reference_point)
