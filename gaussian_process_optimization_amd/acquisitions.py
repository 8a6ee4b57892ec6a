"""EI / LCB / MPI and the local-penalisation batch acquisition, scored on the device.

Contract mirrored (names, arguments, return shapes and signs): GPyOpt/GPyOpt/acquisitions/base.py:7-68
(``acquisition_function`` returns the NEGATED value weighted by constraints and cost), EI.py:7-51, LCB.py:6-46, MPI.py:7-51,
LP.py:10-140, GPyOpt/GPyOpt/core/evaluators/batch_local_penalization.py:7-70, GPyOpt/GPyOpt/util/general.py:113-129.

Where the work runs.  With the HIP ``GPModel``, one output column, constant cost and no constraints, EVERY entry point goes to
libgphip on the whole candidate block at once: values (``gp_acq``), values + x-gradients (``gp_acq_grad``), arg-best / top-k
(``gp_acq_argbest`` / ``gp_acq_topk``), the penalised batch acquisition and its gradient (``gp_acq_lp`` / ``gp_acq_lp_grad``).
A sparse ``GPModel`` built with ``device_acquisitions=True`` takes the same route through the sparse twins (``gp_sparse_acq``,
``gp_sparse_acq_argbest`` / ``_topk``, ``gp_sparse_acq_rows``) over a candidate table of the sparse model's own.
EI and MPI under the evaluation-time cost model (``cost.CostModel`` over our exact ``GPModel``) stay on those routes: the handle
holds a snapshot of the cost GP's posterior mean (``gp_cost_set``) and divides the scores itself (``GP_ACQ_PER_COST``).
EI and MPI with black-box constraints (``feasibility=<FeasibilityModel>``) score ``a(x) F(x)``, F the probability of feasibility of
the constraint GPs, with the incumbent over the feasible observations: tables through ``gp_feas_table`` + ``GP_ACQ_TIMES_FEAS``
(values, arg-best, top-k, and the penalised values / arg-best of ``AcquisitionLP``), one-location and lockstep calls through
``gp_acq_rows_feas``; while no observation is feasible the rule is ``GP_ACQ_POF``, the probability of feasibility alone.
Anything else (a foreign ``BOModel``, a user's cost function, string constraints, several outputs) is scored by ``_Rule`` below from
``model.predict[_withGradients]``: each acquisition is one rule giving its value and its two partial derivatives with respect
to the posterior mean and standard deviation, and every class shares the chain rule built on them.

``AcquisitionEntropySearch`` (ES.py:11-207) is not a rule of mean and deviation: it scores through ``gp_es_*`` (representers, EP
sweeps, tables, one-location calls) with the belief's closing algebra in ``entropy_search.py``; see the class.
"""
import numpy as np
from scipy.special import erfc, log_ndtr, ndtr

from . import _lib
from .cost import CostModel, constant_cost_withGradients
from .gpmodel import GPModel, GPModel_MCMC

_FEW_ROWS = 8            # up to this many locations go down as ONE gp_*_rows call (include/gphip.h): the L-BFGS inner loop
_ROOT_2 = np.sqrt(2)
_ROOT_2PI = np.sqrt(2 * np.pi)
_STD_FLOOR = 1e-10


def get_quantiles(acquisition_par, fmin, m, s):
    """Standardised improvement ``z = (fmin - m - par) / s`` with its normal density and distribution value, returned as
    ``(pdf, cdf, z)``; ``s`` is floored at 1e-10 (in place for arrays).  Same contract as general.py:113-129."""
    if isinstance(s, np.ndarray):
        np.maximum(s, _STD_FLOOR, out=s)
    else:
        s = max(s, _STD_FLOOR)
    z = (fmin - m - acquisition_par) / s
    pdf = np.exp(-0.5 * z ** 2) / _ROOT_2PI
    cdf = 0.5 * erfc(-z / _ROOT_2)
    return pdf, cdf, z


class _Unconstrained(object):
    """Stand-in design space when none is given: every point feasible."""

    def indicator_constraints(self, x):
        return np.ones((np.atleast_2d(x).shape[0], 1))

    def has_constraints(self):
        return False


class _Rule(object):
    """One acquisition as a function of the posterior mean ``mu`` and standard deviation ``sd`` (column vectors):
    ``terms`` returns (value, d value / d mu, d value / d sd); the x-gradient follows by the chain rule in ``gradient``."""

    def __init__(self, device_id, needs_fmin):
        self.device_id = device_id
        self.needs_fmin = needs_fmin

    def terms(self, par, fmin, mu, sd):
        raise NotImplementedError

    def value(self, par, fmin, mu, sd):
        return self.terms(par, fmin, mu, sd)[0]

    def gradient(self, par, fmin, mu, sd, dmu_dx, dsd_dx):
        val, wrt_mu, wrt_sd = self.terms(par, fmin, mu, sd)
        return val, wrt_mu * dmu_dx + wrt_sd * dsd_dx


class _ExpectedImprovement(_Rule):
    def terms(self, par, fmin, mu, sd):
        pdf, cdf, z = get_quantiles(par, fmin, mu, sd)
        return sd * (z * cdf + pdf), -cdf, pdf


class _LowerConfidenceBound(_Rule):
    def terms(self, par, fmin, mu, sd):
        return -mu + par * sd, -1.0, par


class _ProbabilityOfImprovement(_Rule):
    def terms(self, par, fmin, mu, sd):
        pdf, cdf, z = get_quantiles(par, fmin, mu, sd)
        slope = -(pdf / sd)
        return cdf, slope, slope * z


class _MaxValueEntropy(_Rule):
    """Max-value entropy search (Wang & Jegelka 2017, mirrored for a minimum) over K samples y* of the minimum's value, which
    travel in the ``par`` slot of ``terms`` (the rule has no other parameter and reads no fmin):
        g_k = (mu - y*_k) / sd,  h(g) = g lambda(g) / 2 - log Phi(g),  value = mean_k h(g_k),
        h'(g) = -(lambda / 2) (1 + g^2 + g lambda),  d value / d mu = mean_k h'(g_k) / sd,  d value / d sd = -mean_k h'(g_k) g_k / sd,
    lambda = phi / Phi formed in log space; at and below g = -20, where those forms cancel, h, lambda and the bracket of h' come
    from the asymptotic series of Phi, as on the device (``mes_h``, csrc/acq_math.h)."""

    @staticmethod
    def _h(g):
        """(h, h') [shape of g]."""
        far = g <= -20.0
        near = np.where(far, 0.0, g)
        logcdf = log_ndtr(near)
        with np.errstate(under='ignore'):
            lam = np.exp(-0.5 * near * near - 0.5 * np.log(2 * np.pi) - logcdf)
            h = 0.5 * near * lam - logcdf
            hp = -(0.5 * lam) * (1.0 + near * near + near * lam)
        if np.any(far):
            gf = np.where(far, g, -20.0)
            g2 = gf * gf
            t = 1.0 / g2
            term, R, S, W = np.ones_like(t), np.ones_like(t), np.zeros_like(t), np.zeros_like(t)
            for i in range(1, 17):      # T_i = (-1)^i (2i-1)!! g^-2i: R = 1 + sum T_i, S = sum -2 i T_i, W = sum T_i g^2
                term = term * (-(2 * i - 1) * t)
                R = R + term
                S = S + (-2 * i) * term
                W = W + term * g2
            h = np.where(far, W / (2.0 * R) + np.log(-gf) + 0.5 * np.log(2 * np.pi) - np.log(R), h)
            hp = np.where(far, -(0.5 * (-gf / R)) * (S / R), hp)
        return h, hp

    def terms(self, ystar, fmin, mu, sd):
        y = np.asarray(ystar, dtype=float).reshape(1, -1)
        sd = np.maximum(np.asarray(sd, dtype=float).reshape(-1, 1), _STD_FLOOR)
        g = (np.asarray(mu, dtype=float).reshape(-1, 1) - y) / sd
        h, slope = self._h(g)
        return (h.mean(axis=1, keepdims=True), slope.mean(axis=1, keepdims=True) / sd,
                -(slope * g).mean(axis=1, keepdims=True) / sd)


_RULES = {"EI": _ExpectedImprovement(_lib.GP_ACQ_EI, True),
          "LCB": _LowerConfidenceBound(_lib.GP_ACQ_LCB, False),
          "MPI": _ProbabilityOfImprovement(_lib.GP_ACQ_MPI, True),
          "MES": _MaxValueEntropy(_lib.GP_ACQ_MES, False)}


def _pick(values, sense):
    """Lowest-index arg-best of a 1-D score vector (NumPy argmin / argmax semantics)."""
    i = int(np.argmin(values) if sense < 0 else np.argmax(values))
    return i, float(values[i])


def _host_topk(scores, k, sense):
    """The ``k`` best entries of a 1-D score vector in order, (indices, values): equal scores lowest index first, index -1 and
    the value nothing loses to in the tail when there are fewer than ``k`` (what gp_acq_topk returns)."""
    ranked = np.argsort(scores if sense < 0 else -scores, kind="stable")[:k]
    idx = np.full(k, -1, dtype=np.int64)
    val = np.full(k, np.inf if sense < 0 else -np.inf)
    idx[:ranked.size] = ranked
    val[:ranked.size] = scores[ranked]
    return idx, val


def _unit_cost_unconstrained(acq):
    """Unit cost and no constraints: what every device route asks of the acquisition object besides its model."""
    if acq.cost_withGradients is not constant_cost_withGradients:
        return False
    constrained = getattr(acq.space, "has_constraints", None)
    return not (constrained is not None and constrained())


def _unconstrained(acq):
    constrained = getattr(acq.space, "has_constraints", None)
    return not (constrained is not None and constrained())


def _device_cost(acq):
    """The ``CostModel`` whose cost the device can divide by, or None: ``cost_withGradients`` is the bound
    ``_cost_gp_withGradients`` of a ``CostModel`` whose cost GP is our exact ``GPModel`` -- fitted, one output, no Gower kernel, on
    the scored model's device.  (A user's callable is not one, whatever it computes: it keeps the host rule.)"""
    fn = acq.cost_withGradients
    cm = getattr(fn, "__self__", None)
    if not isinstance(cm, CostModel) or getattr(fn, "__func__", None) is not CostModel._cost_gp_withGradients:
        return None
    m = getattr(cm, "cost_model", None)
    if type(m) is not GPModel or m.sparse or m.model is None or not cm._fitted():
        return None
    if m.model.output_dim != 1 or m._gower() or getattr(m.model.kern, "Gower", False):
        return None
    if not hasattr(m.model.kern, "_kernel_id") or m.device != getattr(acq.model, "device", None):
        return None
    return cm


def _cost_ok(acq):
    """Unit cost or a device cost, and no constraints: what the device routes ask of the acquisition besides its model."""
    return _unit_cost_unconstrained(acq) or (_device_cost(acq) is not None and _unconstrained(acq))


def _sync_cost(acq, h):
    """Before a flagged call on handle ``h`` (its data set): upload the cost surface unless ``h`` holds this cost model's
    current generation.  The surface is the cost GP's inputs, alpha, kernel parameters and normaliser."""
    cm = _device_cost(acq)
    if cm is None:
        return
    key = (id(cm), cm.generation)
    if h.cost_key == key:
        return
    gp = cm.cost_model.model
    gp._ensure_fit()
    k = gp.kern
    shift, scale = _normaliser(gp)
    h.cost_set(gp.X, gp._h.alpha(), k._kernel_id, k.ARD, float(k.variance), k.lengthscale.values, shift, scale, key=key)


def _sync_mes(acq, h):
    """Before a scoring call on handle ``h`` of an acquisition that scores over samples of the minimum's value (AcquisitionMES):
    the samples of the model's current fit, resident on ``h``.  Drawing them makes the sampler's table the resident candidates,
    so this comes BEFORE the call's own table is staged."""
    sync = getattr(acq, "_sync_mes", None)
    if sync is not None:
        sync(h)


def _normaliser(gp):
    """(mean, std) the targets of ``gp`` were normalised with: the ``y_mean`` / ``y_std`` of every scoring call."""
    nz = gp.normalizer
    return (0.0, 1.0) if nz is None else (float(nz.mean[0]), float(nz.std[0]))


def _sync_feas(acq, h):
    """Before a flagged table call on handle ``h`` (its candidates resident): cache the probability of feasibility over them
    unless ``h`` holds this feasibility model's current generation for this table (``Handle.set_candidates`` drops the key with
    the table).  Returns the key."""
    fm = acq.feasibility
    key = (id(fm), fm.generation)
    if h.feas_key != key or not _feas_resident(acq, h):
        h.feas_table(acq._feas_pack(), key=key)
    return key


def _feas_resident(acq, h):
    """Whether the LIBRARY still holds the cache ``h.feas_key`` speaks of, over a table of ``h.M`` rows: a rows call that took
    the substitution fallback (gp_acq_rows_feas, gp_acq_rows, gp_predict_rows: the first calls after a fit above N = 4096,
    options small_m / rows_build) made its locations the resident table inside the C entry and dropped the cache with the old one,
    which the Python-side key does not see."""
    return h.feas_info() == (acq.feasibility.num_constraints, h.M)


# ---- the device routes of EI / LCB / MPI and of the penalised acquisition on top of them ---------------------------------
class _Route(object):
    """How the acquisition ``acq`` (an AcquisitionBase with a ``_rule``) reaches libgphip for one kind of model, as four
    operations with the same arguments for every kind (few rows inside ``score``, table values, arg-best, top-k); ``lp`` is
    None or the penaliser's (transform, Xb, r_x0, s_x0).  The two routes are module constants: a call creates no object."""
    rows = None         # the Handle method of the few-rows call

    def score(self, acq, x, grad, lp):
        """Up to ``_FEW_ROWS`` locations go down by value in ONE gp_*_rows call (what scipy's L-BFGS-B issues, optimizer.py:36-61:
        hundreds of calls between two fits, each bound by host time); more become the resident table (``values``)."""
        x = np.asarray(x, dtype=float)
        if x.ndim != 2:
            x = np.atleast_2d(x)
        feas = getattr(acq, "feasibility", None) is not None
        if feas and lp is not None:       # penalised rows fold the penaliser inside the fused finish: tables only
            if grad:
                raise NotImplementedError("the penalised acquisition over black-box constraints has no gradient calls")
            return self.values(acq, x, False, lp)
        if x.shape[0] > _FEW_ROWS and not (feas and grad):
            return self.values(acq, x, grad, lp)
        gp = acq.model.model
        gp._ensure_fit()
        if acq._per_cost:
            _sync_cost(acq, gp._h)
        _sync_mes(acq, gp._h)
        shift, scale = _normaliser(gp)
        if feas:      # any number of rows: gp_acq_rows_feas makes the groups of eight itself (the lockstep optimiser's call)
            return gp._h.acq_rows_feas(acq._feas_pack(), x, acq._acq_id, acq._par(), acq._fmin(), shift, scale, grad=grad)
        return getattr(gp._h, self.rows)(x, acq._acq_id, acq._par(), acq._fmin(), shift, scale, grad=grad, lp=lp)


class _ExactRoute(_Route):
    """gp_acq* over the resident candidate block of the exact model; ``devices``: over replicas of it (gp_group_*)."""
    rows = "acq_rows"

    @staticmethod
    def _stage(acq, x):
        """Make ``x`` the resident candidate block (refitting first if data or hyper-parameters changed) and return what
        every scoring call takes: the handle, fmin and the normaliser's mean / std."""
        gp = acq.model.model
        _sync_mes(acq, gp._h)      # (its sampler stages a table of its own: ahead of this call's)
        given = x
        x = np.atleast_2d(np.asarray(x, dtype=float))
        feas = getattr(acq, "feasibility", None) is not None
        held = getattr(acq, "_feas_table", None)
        # the same table object again under the same generation (the penalised table loop): it is still resident, with its cache
        again = (feas and not gp._dirty and held is not None and held[0] is given and held[1] == x.shape
                 and gp._h.feas_key == held[2] and held[2] == (id(acq.feasibility), acq.feasibility.generation)
                 and gp._h.M == x.shape[0] and _feas_resident(acq, gp._h))
        if again:
            pass
        elif gp._dirty:
            gp._stage(x, fit=False)        # pending refit: fit + posterior at x go down as ONE call
            gp._predict_resident(True)     # GPModel.predict: with_noise=True (gpmodel.py:102)
        else:
            gp._stage(x)
        if acq._per_cost:
            _sync_cost(acq, gp._h)
        if feas:
            acq._feas_table = (given, x.shape, _sync_feas(acq, gp._h))
        return (gp._h, acq._fmin()) + _normaliser(gp)

    @staticmethod
    def _group(acq, x, devices):
        """``x`` split over the replicas of the model on ``devices``: the group, fmin, normaliser mean / std."""
        if acq._per_cost:
            raise NotImplementedError("replica groups score without a cost model: not available with cost_withGradients="
                                      "'evaluation_time'")
        if getattr(acq, "feasibility", None) is not None:
            raise NotImplementedError("replica groups score without black-box constraints: not available with feasibility=")
        if getattr(acq, "_sync_mes", None) is not None:
            raise NotImplementedError("replica groups hold no samples of the minimum's value: MES scores its table on one device")
        gp = acq.model.model
        grp = gp._device_group(devices)
        grp.set_candidates(np.atleast_2d(np.asarray(x, dtype=float)))
        nz = gp.normalizer
        fmin = grp.fmin() if acq._rule.needs_fmin else 0.0
        if acq._rule.needs_fmin and nz is not None:
            fmin = float(nz.inverse_mean(np.array([[fmin]]))[0, 0])
        return (grp, fmin) + _normaliser(gp)

    def values(self, acq, x, grad, lp):
        if grad and getattr(acq, "feasibility", None) is not None:
            raise NotImplementedError("the table gradient entries take no probability of feasibility")
        h, fmin, shift, scale = self._stage(acq, x)
        if lp is None:      # the exact handle names its four table calls: acq / acq_grad / acq_lp / acq_lp_grad
            return (h.acq_grad if grad else h.acq)(acq._acq_id, acq._par(), fmin, shift, scale)
        return (h.acq_lp_grad if grad else h.acq_lp)(acq._acq_id, acq._par(), fmin, lp[0], Xb=lp[1], r_x0=lp[2], s_x0=lp[3],
                                                     y_mean=shift, y_std=scale)

    def argbest(self, acq, x, sense, lp, exclude, devices):
        o, fmin, shift, scale = self._stage(acq, x) if devices is None else self._group(acq, x, devices)
        if lp is None:
            return o.acq_argbest(acq._acq_id, acq._par(), fmin, sense, shift, scale)
        return o.acq_lp_argbest(acq._acq_id, acq._par(), fmin, lp[0], sense, Xb=lp[1], r_x0=lp[2], s_x0=lp[3], exclude=exclude,
                                y_mean=shift, y_std=scale)

    def topk(self, acq, x, k, sense, devices):
        o, fmin, shift, scale = self._stage(acq, x) if devices is None else self._group(acq, x, devices)
        return o.acq_topk(acq._acq_id, acq._par(), fmin, sense, k, shift, scale)


class _SparseRoute(_Route):
    """gp_sparse_acq* over the sparse model's own candidate table."""
    rows = "sparse_acq_rows"

    @staticmethod
    def _stage(acq, x, devices=None):
        """Make ``x`` the sparse model's resident table (not uploaded again while it is the same table)."""
        gp = acq.model.model
        if devices is not None:
            gp._device_group(devices)      # replica groups score the exact GP: NotImplementedError
        gp._stage_table(np.atleast_2d(np.asarray(x, dtype=float)))
        if acq._per_cost:
            _sync_cost(acq, gp._h)
        return (gp._h, acq._fmin()) + _normaliser(gp)

    def values(self, acq, x, grad, lp):
        h, fmin, shift, scale = self._stage(acq, x)
        return h.sparse_acq(acq._acq_id, acq._par(), fmin, shift, scale, grad=grad, lp=lp)

    def argbest(self, acq, x, sense, lp, exclude, devices):
        h, fmin, shift, scale = self._stage(acq, x, devices)
        return h.sparse_acq_argbest(acq._acq_id, acq._par(), fmin, sense, shift, scale, lp=lp, exclude=exclude)

    def topk(self, acq, x, k, sense, devices):
        h, fmin, shift, scale = self._stage(acq, x, devices)
        return h.sparse_acq_topk(acq._acq_id, acq._par(), fmin, sense, k, shift, scale)


_EXACT, _SPARSE = _ExactRoute(), _SparseRoute()


class AcquisitionBase(object):
    """base.py:7-68.  Subclasses either name a ``_rule`` (EI / LCB / MPI) or override ``_compute_acq`` /
    ``_compute_acq_withGradients`` as in GPyOpt."""
    analytical_gradient_prediction = False
    _rule = None
    feasibility = None      # a FeasibilityModel: black-box constraints behind EI / MPI (``_set_feasibility``)
    # (table, shape, key) of the last table this acquisition had the probability of feasibility cached for.  The table is known
    # by OBJECT IDENTITY and shape (and the library is asked whether its cache still stands): scoring the same ndarray again
    # under the same generation neither uploads it nor caches it again -- so a caller who refills that array IN PLACE must pass
    # a new array (or a copy), or gets the scores of the old contents.  The reference also keeps the caller's table alive.
    _feas_table = None
    _feas_incumbent = None  # (key, value): the feasible incumbent of one fit and one generation (``_feasible_fmin``)

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None):
        self.model = model
        self.space = _Unconstrained() if space is None else space
        self.optimizer = optimizer
        self.analytical_gradient_acq = self.analytical_gradient_prediction and self.model.analytical_gradient_prediction
        self.cost_withGradients = cost_withGradients or constant_cost_withGradients

    # ---- what the rule needs ---------------------------------------------------------------------------------------
    @property
    def _per_cost(self):
        """The device divides this acquisition's scores by the cost: EI or MPI (LCB takes no cost) under a device cost."""
        return (self.cost_withGradients is not constant_cost_withGradients and self._rule is not None
                and self._rule.device_id != _lib.GP_ACQ_LCB and _device_cost(self) is not None)

    @property
    def _acq_id(self):
        """The ``type`` of the scoring calls: the rule, with GP_ACQ_PER_COST under a device cost; under black-box constraints
        with GP_ACQ_TIMES_FEAS, the rule GP_ACQ_POF while no observation is feasible."""
        if self._rule is None:
            return None
        rule = self._rule.device_id
        if self.feasibility is not None:
            rule = (_lib.GP_ACQ_POF if self._no_feasible_row() else rule) | _lib.GP_ACQ_TIMES_FEAS
        return rule | _lib.GP_ACQ_PER_COST if self._per_cost else rule

    def _par(self):
        raise NotImplementedError

    def _fmin(self):
        if self.feasibility is not None:
            return self._feasible_fmin()
        return self.model.get_fmin() if self._rule.needs_fmin else 0.0

    # ---- black-box constraints ---------------------------------------------------------------------------------------
    def _set_feasibility(self, feasibility):
        """EI / MPI over our exact GPModel take a FeasibilityModel; every other scored model raises."""
        if feasibility is None:
            return
        m = self.model
        if type(m) is not GPModel or getattr(m, "sparse", False):
            raise NotImplementedError("black-box constraints score our exact GPModel: a foreign, sparse, MCMC or warped model "
                                      "is not available with feasibility=")
        self.feasibility = feasibility

    def _no_feasible_row(self):
        return self.feasibility.feasible_rows.size == 0

    def _feasible_fmin(self):
        """The incumbent over the feasible observations (gp_fmin_rows); 0 while there is none (GP_ACQ_POF reads no fmin)."""
        rows = self.feasibility.feasible_rows
        if rows.size == 0 or not self._rule.needs_fmin:
            return 0.0
        gp = self.model.model
        gp._ensure_fit()
        if self.feasibility.num_rows != gp.X.shape[0]:
            raise ValueError("the feasibility model saw %d observations, the scored model has %d: update both with the same X"
                             % (self.feasibility.num_rows, gp.X.shape[0]))
        # once per fit and generation, as gp_fmin is cached per fit: an L-BFGS run asks for it with every location
        key = (id(self.feasibility), self.feasibility.generation, id(gp), getattr(gp, "_data_epoch", None),
               getattr(gp, "_lml", None), getattr(gp, "_jitter", None))
        held = self._feas_incumbent
        if held is not None and held[0] == key:
            return held[1]
        lowest = gp._h.fmin_rows(rows)
        if gp.normalizer is not None:
            lowest = float(gp.normalizer.inverse_mean(np.array([[lowest]]))[0, 0])
        self._feas_incumbent = (key, lowest)
        return lowest

    def _feas_pack(self):
        pack = self.feasibility.device_pack(self.model.device)
        if pack is None:
            raise NotImplementedError("the constraint models are not exact GPModels on the scored model's device")
        return pack

    def _feas_on_device(self):
        return self.feasibility is None or self.feasibility.device_pack(self.model.device) is not None

    # ---- device route ----------------------------------------------------------------------------------------------
    def _device_ok(self):
        """True when libgphip can score this acquisition by itself: our exact GPModel, one output, unit cost or a device cost
        (``_device_cost``), no constraints.
        (The device entries score the exact posterior: a sparse model takes the sparse route or the host rule.)"""
        m = self.model
        if self._rule is None or not isinstance(m, GPModel) or m.model is None or getattr(m, "sparse", False):
            return False
        return _cost_ok(self) and m.model.output_dim == 1 and self._feas_on_device()

    def _sparse_device_ok(self):
        """True when libgphip scores this acquisition over the SPARSE posterior (gp_sparse_acq*): our GPModel with ``sparse=True``
        and ``device_acquisitions=True``, one output, unit cost, no constraints."""
        m = self.model
        if self._rule is None or not isinstance(m, GPModel) or m.model is None:
            return False
        if not (getattr(m, "sparse", False) and getattr(m, "device_acquisitions", False)):
            return False
        return _cost_ok(self) and m.model.output_dim == 1

    def _route(self):
        """THE choice of where this acquisition is scored: the exact route, the sparse route, or None (the host rule)."""
        if self._device_ok():
            return _EXACT
        return _SPARSE if self._sparse_device_ok() else None

    # ---- the contract ----------------------------------------------------------------------------------------------
    def acquisition_function(self, x):
        """-(acq(x) * feasibility(x)) / cost(x), [M, 1]  (base.py:33-39)."""
        route = self._route()
        if route is not None:
            return route.score(self, x, False, None)
        price, _ = self.cost_withGradients(x)
        if self.feasibility is not None:      # constraint models scored on the host: the same product from log_probability
            x = np.atleast_2d(np.asarray(x, dtype=float))
            val = np.ones((x.shape[0], 1)) if self._no_feasible_row() else self._compute_acq(x)
            val = val * np.exp(self.feasibility.log_probability(x))[:, None]
            return -(val * self.space.indicator_constraints(x)) / price
        return -(self._compute_acq(x) * self.space.indicator_constraints(x)) / price

    def acquisition_function_withGradients(self, x):
        """The same value and its x-gradient [M, D]  (base.py:42-50)."""
        route = self._route()
        if route is not None:
            return route.score(self, x, True, None)
        if self.feasibility is not None:
            x = np.atleast_2d(np.asarray(x, dtype=float))
            if self._no_feasible_row():
                val, dval = np.ones((x.shape[0], 1)), np.zeros(x.shape)
            else:
                val, dval = self._compute_acq_withGradients(x)
            logF, dlogF = self.feasibility.log_probability_withGradients(x)
            F = np.exp(logF)[:, None]
            val, dval = val * F, F * (dval + val * dlogF)
        else:
            val, dval = self._compute_acq_withGradients(x)
        price, dprice = self.cost_withGradients(x)
        feasible = self.space.indicator_constraints(x)
        quotient = val / price
        dquotient = (dval * price - val * dprice) / (price ** 2)
        return -quotient * feasible, -dquotient * feasible

    def argbest(self, x, sense=-1, devices=None):
        """Row index and value of the best entry of ``acquisition_function(x)``: sense=-1 the smallest (GPyOpt's convention,
        anchor_points_generator.py:61), sense=+1 the largest (run.py:1241 takes ``np.argmax``).  Ties -> lowest index.
        ``devices=[0, 1, ...]``: the table is split over replicas of the model on those GPUs, still from this one process."""
        route = self._route()
        if route is not None:
            return route.argbest(self, x, sense, None, (), devices)
        return _pick(self.acquisition_function(x)[:, 0], sense)

    def topk(self, x, k, sense=-1, devices=None):
        """The ``k`` best rows in order, (indices, values): what ``AnchorPointsGenerator.get`` keeps
        (anchor_points_generator.py:59-61).  Equal scores lowest index first; fewer than ``k`` rows -> index -1 in the tail.
        ``devices``: as in ``argbest``."""
        route = self._route()
        if route is not None and k <= 64:
            return route.topk(self, x, k, sense, devices)
        return _host_topk(self.acquisition_function(x)[:, 0], k, sense)

    def optimize(self, duplicate_manager=None):
        """Hand the (negated) acquisition to the acquisition optimiser (base.py:52-60)."""
        kw = dict(f=self.acquisition_function, duplicate_manager=duplicate_manager)
        if self.analytical_gradient_acq:
            kw["f_df"] = self.acquisition_function_withGradients
        return self.optimizer.optimize(**kw)

    # ---- host scoring from model.predict (foreign models, cost, constraints) -----------------------------------------
    def _compute_acq(self, x):
        if self._rule is None:
            raise NotImplementedError('a subclass without a _rule scores itself')
        mu, sd = self.model.predict(x)
        return self._rule.value(self._par(), self._fmin(), mu, sd)

    def _compute_acq_withGradients(self, x):
        if self._rule is None:
            raise NotImplementedError('a subclass without a _rule scores itself')
        fmin = self._fmin()
        mu, sd, dmu_dx, dsd_dx = self.model.predict_withGradients(x)
        return self._rule.gradient(self._par(), fmin, mu, sd, dmu_dx, dsd_dx)


class AcquisitionEI(AcquisitionBase):
    """Expected improvement (EI.py:7-51): ``jitter`` is the improvement margin.  ``feasibility`` (a ``FeasibilityModel``) weights it
    by the probability of feasibility of black-box constraints.  A candidate table scored repeatedly under it is recognised by
    object identity and shape: refill a table in place and it must be passed as a new array (see ``_feas_table``)."""
    analytical_gradient_prediction = True
    _rule = _RULES["EI"]

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None, jitter=0.01, feasibility=None):
        super().__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        self.jitter = jitter
        self._set_feasibility(feasibility)

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        return AcquisitionEI(model, space, optimizer, cost_withGradients, jitter=config['jitter'])

    def _par(self):
        return self.jitter


class AcquisitionLCB(AcquisitionBase):
    """GP lower confidence bound (LCB.py:6-46); a cost model is ignored, as in the reference."""
    analytical_gradient_prediction = True
    _rule = _RULES["LCB"]

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None, exploration_weight=2, feasibility=None):
        if feasibility is not None:      # -mean + w sd changes sign: a product with a probability is meaningless
            raise ValueError("LCB takes no black-box constraints: use EI or MPI with feasibility=")
        super().__init__(model, space, optimizer)
        self.exploration_weight = exploration_weight
        if cost_withGradients is not None:
            print('The set cost function is ignored! LCB acquisition does not make sense with cost.')

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        return AcquisitionLCB(model, space, optimizer, cost_withGradients, exploration_weight=config['weight'])

    def _par(self):
        return self.exploration_weight


class AcquisitionMPI(AcquisitionBase):
    """Maximum probability of improvement (MPI.py:7-51).  ``feasibility``: as for ``AcquisitionEI``, the same identity contract for
    a table scored repeatedly."""
    analytical_gradient_prediction = True
    _rule = _RULES["MPI"]

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None, jitter=0.01, feasibility=None):
        super().__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        self.jitter = jitter
        self._set_feasibility(feasibility)

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        return AcquisitionMPI(model, space, optimizer, cost_withGradients, jitter=config['jitter'])

    def _par(self):
        return self.jitter


class AcquisitionMES(AcquisitionBase):
    """Max-value entropy search (Wang & Jegelka, ICML 2017): the expected reduction of the entropy of the VALUE y* of the global
    minimum, a closed form of the posterior mean and deviation at a location given ``num_samples`` samples of y* -- so, unlike
    ``AcquisitionEntropySearch``, it has an analytic gradient and runs through every route EI has: values, gradients, arg-best,
    top-k, the one-location calls, ``AcquisitionLP`` and the evaluation-time cost (it is a gain, >= 0, as EI is).  GPyOpt has no
    MES: an addition.

    The samples come from ``max_value.MinValueSampler`` over ``grid_size`` uniform draws of the space plus the model's X, drawn
    with ``seed`` and clipped at the incumbent; they are redrawn whenever the model's fit has changed (new data or new
    hyper-parameters), as the belief of ``AcquisitionEntropySearch`` is.  ``sampler='paths'`` takes the samples the paper itself
    takes instead of the Gumbel fit: the minima over that table of ``num_samples`` posterior paths of ``num_features`` features
    (posterior_paths.py; the exact HIP ``GPModel`` only).  With the exact HIP ``GPModel`` (one output) the sampler's
    sums and every score run on the device (``gp_mes_*``, ``GP_ACQ_MES``); a foreign, sparse or warped model is scored on the host
    from ``model.predict[_withGradients]`` by the same rule.  Not available: a model that samples its hyper-parameters, black-box
    constraints, replica groups."""
    analytical_gradient_prediction = True
    _rule = _RULES["MES"]

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, num_samples=10, grid_size=10000, seed=None,
                 sampler='gumbel', num_features=1024):
        if isinstance(model, GPModel_MCMC):
            raise NotImplementedError("MES scores one posterior: not available with a model that samples its hyper-parameters")
        from .max_value import MinValueSampler
        super().__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        self.sampler = MinValueSampler(model, self.space, num_samples, grid_size, seed, sampler=sampler, num_features=num_features)
        self.ystar = None
        self.draws = 0                  # how often the samples were drawn (the handles' staleness key; tests)
        self._fit_signature = None

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        return AcquisitionMES(model, space, optimizer, cost_withGradients, num_samples=config.get('num_min_samples', 10),
                              grid_size=config.get('mes_grid_size', 10000), seed=config.get('sampler_seed', None))

    def _par(self):
        return 0.0

    def _set_feasibility(self, feasibility):
        if feasibility is not None:
            raise NotImplementedError("MES takes no black-box constraints: feasibility= weights EI and MPI")

    def _device_ok(self):
        """Our exact GPModel itself (a warped or sparse model keeps the host rule)."""
        return type(self.model) is GPModel and super()._device_ok()

    def _sparse_device_ok(self):
        return False

    def _signature(self):
        """What the samples were drawn for: the GP object, its data and its parameters (AcquisitionEntropySearch._signature)."""
        gp = getattr(self.model, "model", None)
        return (id(gp), getattr(gp, "_data_epoch", None), np.asarray(getattr(gp, "param_array", ()), dtype=float).tobytes())

    def _samples(self):
        """The samples of the model's current fit, drawn when it has changed."""
        sig = self._signature()
        if self.ystar is None or self._fit_signature != sig:
            self.ystar = np.ascontiguousarray(self.sampler.sample(), dtype=float)
            self._fit_signature = self._signature()
            self.draws += 1
        return self.ystar

    def _sync_mes(self, h):
        self.model.model._ensure_fit()
        ystar = self._samples()
        key = (id(self), self.draws)
        if h.mes_key != key:      # (the library keeps the samples across refits and new data: the key alone decides)
            h.mes_set(ystar, key=key)

    def _compute_acq(self, x):
        mu, sd = self.model.predict(x)
        return self._rule.value(self._samples(), 0.0, mu, sd)

    def _compute_acq_withGradients(self, x):
        ystar = self._samples()
        mu, sd, dmu_dx, dsd_dx = self.model.predict_withGradients(x)
        return self._rule.gradient(ystar, 0.0, mu, sd, dmu_dx, dsd_dx)


class AcquisitionTS(AcquisitionBase):
    """Thompson sampling proper: the acquisition IS a sample of the posterior function, -f_s(x) under LCB's sign convention (so
    ``acquisition_function`` returns f_s, to be minimised), with its analytic gradient.  The samples are posterior paths
    (posterior_paths.py, pathwise conditioning; GPyOpt has nothing of the kind: its 'thompson_sampling' evaluator draws
    independent marginals to pick anchors and then optimises the ordinary acquisition).  ``num_paths`` paths of ``num_features``
    random Fourier features are resident at a time; ``select_path(s)`` chooses the one scored.  They are drawn with ``seed`` and
    redrawn whenever the model's fit has changed, and ``optimize`` draws fresh ones for every suggestion.  Table values, arg-best,
    top-k and the one-location calls all run on the device (``gp_paths_*``).  Only the exact HIP ``GPModel`` with one output, a
    Euclidean kernel and no mean function has paths; a cost model, black-box constraints and ``AcquisitionLP`` are refused."""
    analytical_gradient_prediction = True

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None, num_paths=1, num_features=1024, seed=None,
                 feasibility=None):
        if type(model) is not GPModel or getattr(model, "sparse", False):
            raise NotImplementedError("Thompson sampling draws posterior paths of our exact GPModel: a foreign, sparse, MCMC or "
                                      "warped model has none")
        if cost_withGradients is not None and cost_withGradients is not constant_cost_withGradients:
            raise NotImplementedError("Thompson sampling takes no cost model: a sample of the function is not a gain to divide")
        if feasibility is not None:
            raise NotImplementedError("Thompson sampling takes no black-box constraints: feasibility= weights EI and MPI")
        if not 1 <= int(num_paths) <= _lib.GP_PATHS_MAX_S:
            raise ValueError("between 1 and %d paths, got %r" % (_lib.GP_PATHS_MAX_S, num_paths))
        if not 1 <= int(num_features) <= _lib.GP_PATHS_MAX_F:
            raise ValueError("between 1 and %d features, got %r" % (_lib.GP_PATHS_MAX_F, num_features))
        super().__init__(model, space, optimizer)
        self.num_paths, self.num_features = int(num_paths), int(num_features)
        self._rng = np.random.default_rng(seed)
        self.paths = None
        self.path = 0
        self.draws = 0                  # how often the paths were drawn (tests)
        self._fit_signature = None

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        return AcquisitionTS(model, space, optimizer, cost_withGradients, num_paths=config.get('num_paths', 1),
                             num_features=config.get('num_features', 1024), seed=config.get('sampler_seed', None))

    def _set_feasibility(self, feasibility):
        if feasibility is not None:
            raise NotImplementedError("Thompson sampling takes no black-box constraints: feasibility= weights EI and MPI")

    def select_path(self, s):
        """Score path ``s`` of the resident ``num_paths`` from now on."""
        if not 0 <= int(s) < self.num_paths:
            raise ValueError("path %r outside 0..%d" % (s, self.num_paths - 1))
        self.path = int(s)

    def _signature(self):
        from .posterior_paths import fit_signature
        gp = self.model.model
        return (id(gp),) + fit_signature(gp)

    def redraw(self, num_paths=None):
        """New paths for the model's current fit (``num_paths`` of them from now on, when given)."""
        from .posterior_paths import PosteriorPaths, draw
        if num_paths is not None:
            if not 1 <= int(num_paths) <= _lib.GP_PATHS_MAX_S:
                raise ValueError("between 1 and %d paths, got %r" % (_lib.GP_PATHS_MAX_S, num_paths))
            self.num_paths = int(num_paths)
            self.path = min(self.path, self.num_paths - 1)
        gp = self.model.model
        if gp is None:
            raise RuntimeError("the model has no data yet: updateModel first")
        gp._ensure_fit()
        seed = int(self._rng.integers(0, 2 ** 63 - 1))
        self.paths = PosteriorPaths(gp, draws=draw(gp.kern, gp.num_data, gp.input_dim, self.num_paths, self.num_features, seed))
        self._fit_signature = self._signature()
        self.draws += 1
        return self.paths

    def _paths(self):
        """The paths of the model's current fit, drawn when it has changed (or when other paths took their place on the handle)."""
        gp = self.model.model
        if gp is None:
            raise RuntimeError("the model has no data yet: updateModel first")
        gp._ensure_fit()
        if (self.paths is None or self._fit_signature != self._signature() or self.paths.size != self.num_paths
                or gp._h.paths_key != self.paths._key):
            self.redraw()
        return self.paths

    def _indicator(self, x):
        constrained = getattr(self.space, "has_constraints", None)
        return self.space.indicator_constraints(x) if constrained is not None and constrained() else None

    def _locations(self, x):
        x = np.asarray(x, dtype=float)
        return x if x.ndim == 2 else np.atleast_2d(x)

    def values_on_paths(self, x, path, grad=False):
        """f [M, 1] (and df/dx [M, D]) at the rows of ``x``, row i on path ``path[i]`` (or all on one): in groups of up to
        ``_FEW_ROWS`` rows, one gp_paths_rows call each -- the lockstep optimisers' call."""
        x = self._locations(x)
        paths = self._paths()
        M = x.shape[0]
        path = np.broadcast_to(np.asarray(path, dtype=np.int32).ravel(), (M,)) if np.size(path) == 1 else np.asarray(path, dtype=np.int32)
        f = np.empty((M, 1))
        df = np.empty(x.shape) if grad else None
        for k in range(0, M, _FEW_ROWS):
            r = paths.model._h.paths_rows(x[k:k + _FEW_ROWS], path[k:k + _FEW_ROWS], *paths._normaliser(), grad=grad)
            if grad:
                f[k:k + _FEW_ROWS, 0], df[k:k + _FEW_ROWS] = r
            else:
                f[k:k + _FEW_ROWS, 0] = r
        ind = self._indicator(x)
        if ind is not None:
            f = f * ind
            if grad:
                df = df * ind
        return (f, df) if grad else f

    def _table(self, x):
        """The resident paths over the rows of ``x`` as the resident table: (handle, normaliser mean, std)."""
        paths = self._paths()
        h = paths.model._h
        h.set_candidates(x)
        return (h,) + paths._normaliser()

    def acquisition_function(self, x):
        """f_s(x) of the selected path, [M, 1]: up to ``_FEW_ROWS`` rows by value, more through the table kernel."""
        x = self._locations(x)
        if x.shape[0] <= _FEW_ROWS:
            return self.values_on_paths(x, self.path)
        h, shift, scale = self._table(x)
        f = h.paths_table(shift, scale)[self.path][:, None].copy()
        ind = self._indicator(x)
        return f if ind is None else f * ind

    def acquisition_function_withGradients(self, x):
        return self.values_on_paths(x, self.path, grad=True)

    def table_on_paths(self, x):
        """Every resident path over the rows of ``x``: [M, num_paths] (the batch evaluator's anchor table)."""
        x = self._locations(x)
        h, shift, scale = self._table(x)
        t = h.paths_table(shift, scale).T
        ind = self._indicator(x)
        return t if ind is None else t * ind

    def argbest(self, x, sense=-1, devices=None):
        if devices is not None:
            raise NotImplementedError("replica groups hold no posterior paths: Thompson sampling scores its table on one device")
        x = self._locations(x)
        if self._indicator(x) is not None:
            return _pick(self.acquisition_function(x)[:, 0], sense)
        h, shift, scale = self._table(x)
        idx, val = h.paths_argbest(sense, shift, scale)
        return int(idx[self.path]), float(val[self.path])

    def topk(self, x, k, sense=-1, devices=None):
        if devices is not None:
            raise NotImplementedError("replica groups hold no posterior paths: Thompson sampling scores its table on one device")
        x = self._locations(x)
        return _host_topk(self.acquisition_function(x)[:, 0] if x.shape[0] > _FEW_ROWS else
                          self.values_on_paths(x, self.path)[:, 0], k, sense)

    def optimize(self, duplicate_manager=None):
        """A fresh path for every suggestion, then the acquisition optimiser on it."""
        self.redraw()
        return super().optimize(duplicate_manager=duplicate_manager)

    def _compute_acq(self, x):
        return -self.acquisition_function(x)

    def _compute_acq_withGradients(self, x):
        f, df = self.acquisition_function_withGradients(x)
        return -f, -df


# ---- acquisitions integrated over the hyper-parameter samples ----------------------------------------------------------
class _IntegratedAcquisition(AcquisitionBase):
    """The mean over the model's HMC samples of an EI / MPI / LCB rule, each sample with its own fmin, mean and standard
    deviation (acquisitions/EI_mcmc.py:32-59, MPI_mcmc.py:32-59, LCB_mcmc.py:33-60).  With the HIP ``GPModel_MCMC``, unit cost
    and no constraints the resident ensemble is scored on the device: up to ``_FEW_ROWS`` rows by ``gp_ens_acq_rows``, larger
    blocks by ``gp_ens_acq`` over the candidate table (with gradients: in passes of ``_FEW_ROWS`` rows), ``argbest`` by
    ``gp_ens_acq_argbest``.  Otherwise the reference's formulas run on the host over the model's lists."""
    analytical_gradient_prediction = True

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None):
        super().__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        assert self.model.MCMC_sampler, 'Samples from the hyper-parameters are needed to compute the integrated ' + self._name

    def _ens_ok(self):
        if not isinstance(self.model, GPModel_MCMC) or self.model.model is None or self.model.hmc_samples is None:
            return False
        return _cost_ok(self)

    def _ens_handle(self):
        h = self.model.model._h
        if self._per_cost:
            _sync_cost(self, h)
        return h

    def acquisition_function(self, x):
        if not self._ens_ok():
            return super().acquisition_function(x)
        x = np.atleast_2d(np.asarray(x, dtype=float))
        h = self._ens_handle()
        if x.shape[0] <= _FEW_ROWS:
            return h.ens_acq_rows(x, self._acq_id, self._par())
        h.set_candidates(x)
        return h.ens_acq(self._acq_id, self._par())

    def acquisition_function_withGradients(self, x):
        if not self._ens_ok():
            return super().acquisition_function_withGradients(x)
        x = np.atleast_2d(np.asarray(x, dtype=float))
        h = self._ens_handle()
        parts = [h.ens_acq_rows(x[i:i + _FEW_ROWS], self._acq_id, self._par(), grad=True) for i in range(0, x.shape[0], _FEW_ROWS)]
        return np.vstack([p[0] for p in parts]), np.vstack([p[1] for p in parts])

    def argbest(self, x, sense=-1, devices=None):
        if not self._ens_ok() or devices is not None:
            if devices is not None:
                raise NotImplementedError("replica groups score one hyper-parameter vector: not available with GPModel_MCMC")
            return _pick(self.acquisition_function(x)[:, 0], sense)
        h = self._ens_handle()
        h.set_candidates(np.atleast_2d(np.asarray(x, dtype=float)))
        return h.ens_acq_argbest(self._acq_id, self._par(), sense)

    def _fmin(self):
        raise NotImplementedError("an integrated acquisition has one fmin per sample")

    def _compute_acq(self, x):
        means, stds = self.model.predict(x)
        fmins = self.model.get_fmin()
        total = 0
        for mu, sd, fmin in zip(means, stds, fmins):
            total = total + self._rule.value(self._par(), fmin, mu, sd)
        return total / len(means)

    def _compute_acq_withGradients(self, x):
        means, stds, dmdxs, dsdxs = self.model.predict_withGradients(x)
        fmins = self.model.get_fmin()
        total, dtotal = 0, 0
        for mu, sd, fmin, dmu, dsd in zip(means, stds, fmins, dmdxs, dsdxs):
            val, dval = self._rule.gradient(self._par(), fmin, mu, sd, dmu, dsd)
            total, dtotal = total + val, dtotal + dval
        return total / len(means), dtotal / len(means)


class AcquisitionEI_MCMC(_IntegratedAcquisition):
    """Integrated expected improvement (EI_mcmc.py:7-59)."""
    _rule = _RULES["EI"]
    _name = "EI"

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None, jitter=0.01):
        super().__init__(model, space, optimizer, cost_withGradients)
        self.jitter = jitter

    def _par(self):
        return self.jitter


class AcquisitionMPI_MCMC(_IntegratedAcquisition):
    """Integrated probability of improvement (MPI_mcmc.py:7-59)."""
    _rule = _RULES["MPI"]
    _name = "MPI"

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None, jitter=0.01):
        super().__init__(model, space, optimizer, cost_withGradients)
        self.jitter = jitter

    def _par(self):
        return self.jitter


class AcquisitionLCB_MCMC(_IntegratedAcquisition):
    """Integrated lower confidence bound (LCB_mcmc.py:7-60); a cost model is ignored, as in the reference."""
    _rule = _RULES["LCB"]
    _name = "GP-LCB"

    def __init__(self, model, space=None, optimizer=None, cost_withGradients=None, exploration_weight=2):
        super().__init__(model, space, optimizer, None)
        self.exploration_weight = exploration_weight

    def _par(self):
        return self.exploration_weight


# ---- local penalisation ---------------------------------------------------------------------------------------------
def _log_transform(acq, transform):
    """(log T(acq), d log T / d acq) of the positive base acquisition: T = identity ('none': log(acq + 1e-50), slope
    1 / acq) or softplus (log of log(1 + e^acq), taken as log(acq) from 40 on; slope 1 / (softplus (1 + e^-acq)))."""
    acq = np.asarray(acq, dtype=float)
    if transform == 'softplus':
        big = acq >= 40.
        soft = np.log1p(np.exp(acq))
        return np.where(big, np.log(np.where(big, acq, 1.0)), np.log(soft)), 1. / (soft * (1. + np.exp(-acq)))
    if transform == 'none':
        return np.log(acq + 1e-50), 1. / acq
    return acq, np.ones_like(acq)


def _exclusion(x, centres, radius, width):
    """Per (point, centre): z = (|x - centre| - radius) / width and the distance itself, [M, nb] each."""
    gap = np.atleast_2d(x)[:, None, :] - np.atleast_2d(centres)[None, :, :]
    dist = np.sqrt(np.square(gap).sum(-1))
    return (dist - radius) / width, dist


class AcquisitionLP(AcquisitionBase):
    """Local-penalisation wrapper of a base acquisition for batch design (Gonzalez et al. 2016; LP.py:10-140), always in log
    space: ``-log T(acq(x)) - sum_k log Phi((|x - x_k| - r_k) / s_k)`` over the batch points x_k chosen so far."""
    analytical_gradient_prediction = True

    def __init__(self, model, space=None, optimizer=None, acquisition=None, transform='none'):
        if isinstance(acquisition, AcquisitionTS):
            raise NotImplementedError("Thompson sampling spreads a batch by drawing one path per element: it is not penalised "
                                      "(use the 'thompson_sampling' evaluator)")
        if getattr(acquisition, "_takes_no_penaliser", None):      # (multi_objective.AcquisitionEHVI: the sentence why)
            raise NotImplementedError(acquisition._takes_no_penaliser)
        super().__init__(model, space, optimizer)
        self.acq = acquisition
        kind = str(transform).lower()
        # LCB can be negative, so its plain logarithm is replaced by log(softplus) (LP.py:32-35)
        self.transform = 'softplus' if (kind == 'none' and isinstance(acquisition, AcquisitionLCB)) else kind
        self.X_batch = self.r_x0 = self.s_x0 = None
        self._lp_packed = None

    def update_batches(self, X_batch, L, Min):
        """Set (or with None: clear) the batch chosen so far; radii and widths of its exclusion balls come from the model's
        prediction at the batch, the Lipschitz constant ``L`` and the best observed value ``Min`` (LP.py:41-62)."""
        self.X_batch, have_batch = X_batch, X_batch is not None
        if have_batch:
            self.r_x0, self.s_x0 = self._ball_parameters(X_batch, L, Min)
        self._lp_packed = None          # (transform, Xb, r, s) as contiguous float64, built once per batch (see _lp_spec)

    def _ball_parameters(self, centres, L, Min):
        mu, spread = self.model.predict(np.atleast_2d(centres))
        # the reference floors what ``predict`` returns as its second output (a standard deviation here) at 1e-16 and takes
        # the square root of it once more; kept, since r / s define the batch the reference would pick
        width = np.sqrt(np.maximum(spread, 1e-16)) / L
        return ((mu - Min) / L).ravel(), width.ravel()

    # -- host scoring (foreign models) -------------------------------------------------------------------------------
    def _score_on_host(self, x):
        with np.errstate(over='ignore'):
            logt, _ = _log_transform(-self.acq.acquisition_function(x)[:, 0], self.transform)
        score = -logt
        if self.X_batch is not None:
            z, _ = _exclusion(x, self.X_batch, self.r_x0, self.s_x0)
            score = score - log_ndtr(z).sum(axis=-1)
        return score

    def _penalty_slope(self, x):
        """What the reference subtracts from every gradient component (LP.py:91-103): sum over the batch of
        pdf(z) / (s Phi(z) |x - x_k|) -- the direction factor is absent there, and so here."""
        z, dist = _exclusion(x, self.X_batch, self.r_x0, self.s_x0)
        mass = ndtr(z)
        with np.errstate(divide='ignore', invalid='ignore'):
            term = 1. / (self.s_x0 * _ROOT_2PI * mass) * np.exp(-np.square(z) / 2) / dist
        term[mass < 1e-50] = 0.
        return term.sum(axis=1)[:, None]

    # -- device route ------------------------------------------------------------------------------------------------
    def _lp_route(self):
        """The route of the base acquisition, when it scores this model and the transform is one the device knows."""
        base = self.acq
        if base is None or base.model is not self.model or self.transform not in ('none', 'softplus'):
            return None
        if base._per_cost:      # the device penalises the base acquisition at unit cost: a base with a cost keeps the host rule
            return None
        return base._route()

    def _lp_device_ok(self):
        return self._lp_route() is _EXACT

    def _lp_sparse_ok(self):
        return self._lp_route() is _SPARSE

    @property
    def _softplus(self):
        """The ``transform`` argument of the device entries: 1 softplus, 0 none."""
        return 1 if self.transform == 'softplus' else 0

    def _lp_spec(self):
        """(transform, Xb, r_x0, s_x0) of the batch in force as contiguous float64, built once per batch: an L-BFGS run of
        compute_batch makes hundreds of calls with one batch (per object identity of the batch attributes: assigning new
        arrays renews it)."""
        src = (self.X_batch, self.r_x0, self.s_x0, self.transform)
        held = getattr(self, "_lp_packed", None)
        if held is not None:
            was = held[0]
            if was[0] is src[0] and was[1] is src[1] and was[2] is src[2] and was[3] is src[3]:
                return held[1]
        if self.X_batch is None:
            lp = (self._softplus, None, None, None)
        else:
            lp = (self._softplus, np.ascontiguousarray(np.atleast_2d(self.X_batch), dtype=float),
                  np.ascontiguousarray(np.atleast_1d(self.r_x0), dtype=float),
                  np.ascontiguousarray(np.atleast_1d(self.s_x0), dtype=float))
        self._lp_packed = (src, lp)
        return lp

    def acquisition_function(self, x):
        """1-D array like the reference's (LP.py:105-110)."""
        route = self._lp_route()
        if route is not None:
            return route.score(self.acq, x, False, self._lp_spec())
        return self._score_on_host(x)

    def d_acquisition_function(self, x):
        return self.acquisition_function_withGradients(x)[1]

    def acquisition_function_withGradients(self, x):
        """(value [M], gradient [M, D])  (LP.py:112-140)."""
        if getattr(self.acq, "feasibility", None) is not None:
            raise NotImplementedError("the penalised acquisition over black-box constraints scores tables (values, arg-best): "
                                      "it has no gradient calls")
        x = np.atleast_2d(np.asarray(x, dtype=float))
        route = self._lp_route()
        if route is not None:
            return route.score(self.acq, x, True, self._lp_spec())
        neg, dneg = self.acq.acquisition_function_withGradients(x)
        with np.errstate(over='ignore', divide='ignore'):
            _, slope = _log_transform(-neg[:, 0], self.transform)
        grad = slope[:, None] * dneg
        if self.X_batch is not None:
            grad = grad - self._penalty_slope(x)
        return self.acquisition_function(x), grad

    def argbest(self, x, sense=+1, exclude=(), devices=None):
        """Arg-best of ``acquisition_function(x)`` with the rows in ``exclude`` masked out (run.py:1241,1249-1252).
        ``devices``: the table split over replicas of the model on those GPUs, from this one process (gp_group_*)."""
        route = self._lp_route()
        if route is not None:
            return route.argbest(self.acq, x, sense, self._lp_spec(), exclude, devices)
        scores = np.array(self.acquisition_function(x), dtype=float)
        scores[list(exclude)] = -np.inf if sense > 0 else np.inf
        return _pick(scores, sense)


def estimate_L(model, bounds, storehistory=True):
    """Lipschitz constant of the posterior mean over the box ``bounds``: the largest |d mean / dx| over 500 uniform draws
    plus the training inputs, polished by L-BFGS-B from the best of them; 10 for a flat model
    (core/evaluators/batch_local_penalization.py:52-70).  ``model`` is the GP (``GPModel.model``): all 500 + N predictive
    gradients come from ONE batched device call."""
    from scipy.optimize import minimize

    mean_jac = getattr(model, "mean_gradients", None)      # the HIP model: d mean / dx without the variance's share of the work

    def neg_slope(pts):
        jac = mean_jac(np.atleast_2d(pts)) if mean_jac is not None else model.predictive_gradients(np.atleast_2d(pts))[0]
        return -np.sqrt((jac * jac).sum(1))

    box = np.asarray(list(bounds), dtype=float)
    # the global generator is consumed as the reference consumes it -- 500 values for the first variable, then 500 for the
    # second, ... (util/general.py:63-73) -- so that a seeded run starts L-BFGS from the reference's point
    unit = np.random.uniform(size=(box.shape[0], 500))
    draws = (box[:, :1] + (box[:, 1:] - box[:, :1]) * unit).T
    pool = np.vstack([draws, model.X])
    start = pool[np.argmin(neg_slope(pool))]
    polished = minimize(lambda p: float(neg_slope(p).ravel()[0]), start, method='L-BFGS-B', bounds=[tuple(b) for b in box],
                        options={'maxiter': 200})
    steepest = -float(polished.fun)
    return steepest if steepest >= 1e-7 else 10


class LocalPenalization(object):
    """Batch evaluator: pick ``batch_size`` points one after the other, each time penalising the acquisition around the
    points already chosen (core/evaluators/batch_local_penalization.py:7-49)."""

    def __init__(self, acquisition, batch_size):
        self.acquisition = acquisition
        self.batch_size = batch_size

    def _constants(self):
        gp = self.acquisition.model.model
        return estimate_L(gp, self.acquisition.space.get_bounds()), gp.Y.min()

    def compute_batch(self, duplicate_manager=None, context_manager=None):
        """Batch by optimising the (penalised) acquisition over the domain."""
        lp = self.acquisition
        assert isinstance(lp, AcquisitionLP)
        lp.update_batches(None, None, None)
        batch = lp.optimize()[0]
        if self.batch_size >= 2:
            lipschitz, best_seen = self._constants()
            for _ in range(self.batch_size - 1):
                lp.update_batches(batch, lipschitz, best_seen)
                batch = np.vstack((batch, lp.optimize()[0]))
        lp.update_batches(None, None, None)
        return batch

    def compute_batch_from_table(self, table, sense=+1, devices=None, lipschitz=None):
        """The candidate-table variant the thesis driver uses (run.py:1234-1258): ``batch_size`` distinct rows of ``table`` by
        repeated arg-best of the penalised acquisition; ``devices``: scored on several GPUs from this one process.
        ``lipschitz``: a constant estimated earlier for the same model (run.py re-estimates the same L for each of its
        three acquisitions, :1244); None estimates it here, after the first row, as the driver does."""
        lp = self.acquisition
        lp.update_batches(None, None, None)
        rows = [lp.argbest(table, sense, devices=devices)[0]]
        if self.batch_size >= 2:
            if lipschitz is None:
                lipschitz, best_seen = self._constants()
            else:
                best_seen = self.acquisition.model.model.Y.min()
            while len(rows) < self.batch_size:
                lp.update_batches(np.atleast_2d(table[rows]), lipschitz, best_seen)
                rows.append(lp.argbest(table, sense, exclude=rows, devices=devices)[0])
        lp.update_batches(None, None, None)
        return rows


# ---- entropy search ---------------------------------------------------------------------------------------------------
class AcquisitionEntropySearch(AcquisitionBase):
    """Entropy search (Hennig & Schuler 2012; ES.py:11-207): the expected reduction of the entropy of the belief over where the
    minimum lies, the belief held on ``num_representer_points`` points drawn by ``sampler`` from ``proposal_function`` (default:
    log expected improvement inside the bounds, -inf outside; it takes one location or a matrix of them).  Constructor
    arguments and refusals are the reference's; ``device`` is the addition.

    Where the work runs.  With the exact HIP ``GPModel``, one output, unit cost and no constraints (and ``device`` left True):
    the representers' posterior (``gp_es_set_representers``), the EP sweeps of p_min (``gp_es_pmin``) and every score
    (``gp_es_acq`` / ``gp_es_acq_argbest`` over the candidate block, ``gp_es_acq_rows`` for up to eight locations) run on the device; the closing algebra of the belief stays
    on the host (entropy_search.py).  Otherwise -- a sparse model, a cost model, constraints, ``device=False`` -- the reference's
    per-candidate arithmetic runs on the host over ``predict``, ``predict_covariance`` and ``get_covariance_between_points``; a
    sparse model serves a whole block of candidates with one ``predict`` and one ``get_covariance_between_points`` (the
    representers stay resident on the device: ``gp_sparse_cov_between``).

    A deliberate difference: the reference samples representers and computes the belief once and never again
    (``_required_parameters_initialized``); here both are renewed whenever the model's fit has changed (new data or new
    hyper-parameters), since the belief describes the posterior it was computed from."""
    analytical_gradient_prediction = False

    def __init__(self, model, space, sampler, optimizer=None, cost_withGradients=None, num_samples=100,
                 num_representer_points=50, proposal_function=None, burn_in_steps=50, device=True):
        if not isinstance(model, GPModel):
            raise RuntimeError("The current entropy search implementation supports only GPModel as model")
        from scipy.stats import norm
        super().__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        self.analytical_gradient_acq = False
        self.input_dim = len(self.space.get_bounds())
        self.num_repr_points = num_representer_points
        self.burn_in_steps = burn_in_steps
        self.sampler = sampler
        self.device = bool(device)
        self.proposal_function = proposal_function or self._default_proposal()
        self.W = norm.ppf(np.linspace(1. / (num_samples + 1), 1 - 1. / (num_samples + 1), num_samples))[np.newaxis, :]
        self.repr_points = self.repr_points_log = self.logP = None
        self._fit_signature = None
        self._belief_on_device = False

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        raise NotImplementedError("Not implemented")

    def _default_proposal(self):
        box = np.asarray(self.space.get_bounds(), dtype=float)
        ei = AcquisitionEI(self.model, self.space)

        def log_ei(x):
            x = np.asarray(x, dtype=float)
            rows = np.atleast_2d(x)
            inside = np.all((box[:, 0] <= rows) & (rows <= box[:, 1]), axis=1)
            out = np.full(rows.shape[0], -np.inf)
            if inside.any():
                gain = -ei.acquisition_function(rows[inside]) if ei._device_ok() else ei._compute_acq(rows[inside])
                with np.errstate(divide='ignore'):
                    out[inside] = np.log(np.clip(np.ravel(gain), 0., np.inf))
            return float(out[0]) if x.ndim == 1 else out
        return log_ei

    # ---- the belief ------------------------------------------------------------------------------------------------------
    def _es_device_ok(self):
        if not self.device or self.model.model is None or getattr(self.model, "sparse", False):
            return False
        if getattr(self.model.model, "mean_function", None) is not None:   # the gp_es_* entries refuse a resident mean function
            return False
        return _unit_cost_unconstrained(self) and self.model.model.output_dim == 1

    def _signature(self):
        """What the belief was computed for: the GP object, its data and its parameters."""
        gp = self.model.model
        return (id(gp), getattr(gp, "_data_epoch", None), np.asarray(getattr(gp, "param_array", ()), dtype=float).tobytes())

    def _update_parameters(self):
        """Representers, their log-proposal values and the belief over them (ES.py:85-112), for the model's current fit."""
        from . import entropy_search as _es
        pts, logs = self.sampler.get_samples(self.num_repr_points, self.proposal_function, self.burn_in_steps)
        pts, logs = np.atleast_2d(np.asarray(pts, dtype=float)), np.asarray(logs, dtype=float).reshape(-1)
        if np.any(np.isnan(logs)) or np.any(np.isposinf(logs)):
            raise RuntimeError("Sampler generated representer points with invalid log values: {}".format(logs))
        keep = ~np.isneginf(logs)      # a representer the proposal gives no mass cannot be the minimum (ES.py:97-102)
        pts, logs = pts[keep], logs[keep]
        if pts.shape[0] < 1:
            raise RuntimeError("Sampler generated no representer point with a finite log value")
        on_device = self._es_device_ok()
        gp = self.model.model
        if on_device:
            gp._ensure_fit()
            shift, scale = _normaliser(gp)
            mu, cov = gp._h.es_set_representers(pts, shift, scale)
            cov = np.maximum(cov, 1e-10)       # GPModel._predict's floor, on every entry (gpmodel.py:99)
        else:
            mu = np.ravel(self.model.predict(pts)[0])
            cov = self.model.predict_covariance(pts)
        R = pts.shape[0]
        if R == 1:      # one point is the minimum with certainty: nothing to propagate
            belief = (np.zeros(1), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1, 1)))
        else:
            sites = gp._h.es_pmin(mu, cov) if on_device else None
            belief = _es.joint_min(mu, cov, sites)
        self.repr_points, self.repr_points_log = pts, logs.reshape(-1, 1)
        self.dlogPdMu, self.dlogPdSigma, self.dlogPdMudMu = belief[1:]
        self.logP = belief[0].reshape(-1, 1)
        self._Q = _es.quadratic_forms(self.dlogPdSigma, self.dlogPdMudMu)
        if on_device:
            gp._h.es_set_belief(self.logP, self.repr_points_log, self.dlogPdMu, self._Q, self.W)
        self._fit_signature = self._signature()
        self._belief_on_device = on_device

    def _required_parameters_initialized(self):
        return not (self.repr_points is None or self.repr_points_log is None or self.logP is None)

    def _refresh(self, on_device):
        """The belief of the current fit, on the device when the scoring call will look for it there."""
        if on_device:
            self.model.model._ensure_fit()
        if (not self._required_parameters_initialized() or self._fit_signature != self._signature()
                or (on_device and not self._belief_on_device)):
            self._update_parameters()

    def _check_dim(self, x):
        if x.shape[1] != self.input_dim:
            raise ValueError("Dimensionality mismatch: x should be of size {}, but is of size {}".format(self.input_dim, x.shape[1]))

    # ---- the contract ----------------------------------------------------------------------------------------------------
    def _device_block(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=float))
        self._check_dim(x)
        self._refresh(True)
        gp = self.model.model
        gp._stage(x)
        return gp, _normaliser(gp)[1]

    def acquisition_function(self, x):
        if self._es_device_ok():
            x = np.atleast_2d(np.asarray(x, dtype=float))
            if x.shape[0] <= _FEW_ROWS:      # the optimiser's calls: ONE gp_es_acq_rows, locations by value
                self._check_dim(x)
                self._refresh(True)
                return self.model.model._h.es_acq_rows(x, _normaliser(self.model.model)[1])
            gp, scale = self._device_block(x)
            return gp._h.es_acq(scale)
        return super().acquisition_function(np.atleast_2d(np.asarray(x, dtype=float)))

    def acquisition_function_withGradients(self, x):
        return self._compute_acq_withGradients(x)

    def argbest(self, x, sense=-1, devices=None):
        if devices is not None:
            raise NotImplementedError("entropy search scores its table on one device")
        if self._es_device_ok():
            gp, scale = self._device_block(x)
            return gp._h.es_acq_argbest(sense, scale)
        return _pick(self.acquisition_function(x)[:, 0], sense)

    def topk(self, x, k, sense=-1, devices=None):
        if devices is not None:
            raise NotImplementedError("entropy search scores its table on one device")
        return _host_topk(self.acquisition_function(x)[:, 0], k, sense)

    def _compute_acq(self, x):
        """The host route: ES.py:124-170 candidate by candidate over the model's own predictions."""
        from . import entropy_search as _es
        x = np.atleast_2d(np.asarray(x, dtype=float))
        self._check_dim(x)
        self._refresh(False)
        out = np.zeros((x.shape[0], 1))
        if getattr(self.model, "sparse", False) and x.shape[0] > 0:
            # a sparse model: the whole block in two device calls (gp_sparse_predict, gp_sparse_cov_between over the resident
            # representers), then the same arithmetic per candidate
            _, sd = self.model.predict(x, with_noise=False)
            cov = self.model.get_covariance_between_points(self.repr_points, x)
            for j in range(x.shape[0]):
                out[j, 0] = _es.score(cov[:, [j]] / sd[j], self.logP, self.repr_points_log, self.dlogPdMu, self._Q, self.W)
            return out
        for j in range(x.shape[0]):
            row = x[[j], :]
            _, sd = self.model.predict(row, with_noise=False)
            m = self.model.get_covariance_between_points(self.repr_points, row) / sd
            out[j, 0] = _es.score(m, self.logP, self.repr_points_log, self.dlogPdMu, self._Q, self.W)
        return out

    def _compute_acq_withGradients(self, x):
        raise NotImplementedError("Analytic derivatives are not supported.")
