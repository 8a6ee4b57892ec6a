"""The discrete knowledge gradient (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011): the expected decrease of the
MINIMUM OF THE POSTERIOR MEAN after one more observation at x,

    KG(x) = min_i mu(a_i)  -  E_y[ min_i mu_{+ (x, y)}(a_i) ],      a_i over a discretisation set X_A and x itself,

the acquisition of choice under noisy observations (it never reads f_min over the observations) and when the recommendation is
the posterior-mean minimiser.  After an observation at x the means move along lines in one standard normal Z, so KG is the lower
envelope of A + 1 lines in closed form, and it has a closed-form gradient (include/gphip.h spells both out).  Values over tables,
arg-best, top-k and the one-location calls with gradients all run on the device (``gp_kg_*``; csrc/kg.hip, csrc/api_kg.hip).
GPyOpt has nothing of the kind.

``AcquisitionKG`` rebuilds the discretisation set whenever the model's fit has changed, deterministically from its seed: the
ceil(A / 4) lowest-posterior-mean locations of a uniform table (ranked on the device: top-k of LCB with exploration weight 0), the
training input with the lowest posterior mean, and uniform draws for the rest.
"""
import numpy as np

from . import _lib
from .acquisitions import AcquisitionBase, AcquisitionLCB, _host_topk, _normaliser, _pick
from .cost import constant_cost_withGradients
from .gpmodel import GPModel

_FEW_ROWS = 8       # up to this many locations go down as ONE gp_kg_rows call (the fused rows path, gradients included)


def _refuse(what):
    return NotImplementedError("the knowledge gradient scores our exact GPModel with one output: %s" % what)


class AcquisitionKG(AcquisitionBase):
    """Discrete knowledge gradient over ``num_points`` discretisation points (1 .. 256), rebuilt at every model update from
    ``kg_table_size`` uniform draws and ``sampler_seed``.  ``acquisition_function`` returns -KG, to be minimised, and
    ``acquisition_function_withGradients`` its gradient for up to 8 rows a call (what L-BFGS-B and the lockstep anchor optimiser
    ask).  Only the exact HIP ``GPModel`` with one output, a Euclidean kernel and no mean function is scored; a foreign, sparse,
    MCMC, warped or input-warped model, a Gower kernel, a cost model, black-box constraints, local penalisation and replica
    groups raise ``NotImplementedError``."""
    analytical_gradient_prediction = True
    _takes_no_penaliser = ("the knowledge gradient is not penalised: a batch of KG points is batch KG, which is not implemented "
                           "(use the 'sequential' evaluator)")

    def __init__(self, model, space, optimizer=None, num_points=64, kg_table_size=10000, sampler_seed=None,
                 cost_withGradients=None, feasibility=None):
        if type(model) is not GPModel:
            raise _refuse("a foreign, MCMC, warped or input-warped model has no knowledge gradient on the device")
        if getattr(model, "sparse", False):
            raise _refuse("not available with sparse=True")
        if model._gower():
            raise _refuse("not available with the Gower kernel")
        if getattr(model, "mean_function", None) is not None:
            raise _refuse("not available with a mean function")
        if cost_withGradients is not None and cost_withGradients is not constant_cost_withGradients:
            raise NotImplementedError("the knowledge gradient takes no cost model: KG per unit of cost is not implemented")
        if feasibility is not None:
            raise NotImplementedError("the knowledge gradient takes no black-box constraints: feasibility= weights EI and MPI")
        if not 1 <= int(num_points) <= _lib.GP_KG_MAX_A:
            raise ValueError("between 1 and %d discretisation points, got %r" % (_lib.GP_KG_MAX_A, num_points))
        if int(kg_table_size) < 1:
            raise ValueError("kg_table_size must be at least 1, got %r" % (kg_table_size,))
        super().__init__(model, space, optimizer)
        self.num_points, self.kg_table_size, self.sampler_seed = int(num_points), int(kg_table_size), sampler_seed
        self._mean = AcquisitionLCB(model, space, optimizer, None, exploration_weight=0)      # acquisition_function = +mu(x): sense -1 ranks the lowest means on the device
        self.points = None              # the discretisation set of the current fit [A, D]
        self.points_mean = None         # ... and its posterior means [A], un-normalised
        self.builds = 0                 # how often the set was built (the handle's staleness key; tests)
        self.uploads = 0                # how often it went to a handle
        self._fit_signature = None

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        return AcquisitionKG(model, space, optimizer, num_points=config.get('num_kg_points', 64),
                             kg_table_size=config.get('kg_table_size', 10000), sampler_seed=config.get('sampler_seed', None),
                             cost_withGradients=cost_withGradients)

    def _set_feasibility(self, feasibility):
        if feasibility is not None:
            raise NotImplementedError("the knowledge gradient takes no black-box constraints: feasibility= weights EI and MPI")

    # ---- the discretisation set --------------------------------------------------------------------------------------------
    def _signature(self):
        """What the set was built for: the GP object, its data and its parameters (AcquisitionMES._signature)."""
        gp = getattr(self.model, "model", None)
        return (id(gp), getattr(gp, "_data_epoch", None), np.asarray(getattr(gp, "param_array", ()), dtype=float).tobytes())

    def discretisation(self):
        """[A, D]: the ceil(A / 4) lowest-posterior-mean rows of ``kg_table_size`` uniform draws, the training input with the lowest
        posterior mean, uniform draws for the rest -- all from ``numpy.random.RandomState(sampler_seed)``, so the same fit gives
        the same set."""
        A = self.num_points
        rng = np.random.RandomState(self.sampler_seed)
        table = np.atleast_2d(np.asarray(self.space.samples_uniform(self.kg_table_size, rng), dtype=float))
        n_low = min((A + 3) // 4, table.shape[0])
        idx, _ = self._mean.topk(table, n_low, sense=-1)
        idx = np.asarray(idx)
        rows = [table[idx[idx >= 0]]]
        X = np.atleast_2d(np.asarray(self.model.model.X, dtype=float))
        if A > n_low:
            rows.append(X[[self._mean.argbest(X, sense=-1)[0]]])
        have = sum(r.shape[0] for r in rows)
        if A > have:
            rows.append(np.atleast_2d(np.asarray(self.space.samples_uniform(A - have, rng), dtype=float)))
        return np.ascontiguousarray(np.vstack(rows)[:A])

    def _handle(self):
        """The model's handle with a current fit and the discretisation set of that fit resident."""
        gp = self.model.model
        if gp is None:
            raise RuntimeError("the model has no data yet: updateModel first")
        if gp.output_dim != 1:
            raise _refuse("the model has %d outputs" % gp.output_dim)
        if getattr(gp.kern, "Gower", False):
            raise _refuse("not available with the Gower kernel")
        gp._ensure_fit()
        sig = self._signature()
        if self.points is None or self._fit_signature != sig:
            self.points = self.discretisation()
            self.points.setflags(write=False)
            self._fit_signature = self._signature()
            self.builds += 1
        h = gp._h
        key = (id(self), self.builds)
        # the library drops the points with every new factor, which the key does not see: kg.info() tells
        if getattr(h, "kg_key", None) != key or h.kg.info() != self.points.shape[0]:
            gp._ensure_fit()
            shift, scale = _normaliser(gp)
            self.points_mean = h.kg.set_points(self.points, shift, scale, key=key)
            self.uploads += 1
        return gp, h

    # ---- the contract ------------------------------------------------------------------------------------------------------
    def _indicator(self, x):
        constrained = getattr(self.space, "has_constraints", None)
        if constrained is None or not constrained():
            return 1.0
        return self.space.indicator_constraints(x)

    def _table(self, x):
        """``x`` as the handle's resident candidates, with the points resident: (handle, y_std)."""
        gp, h = self._handle()
        gp._stage(x)
        if h.kg.info() != self.points.shape[0]:      # staging refitted after all
            gp, h = self._handle()
        return h, _normaliser(gp)[1]

    def acquisition_function(self, x):
        """-KG of every row of ``x``, [M, 1]: up to 8 rows as ONE gp_kg_rows call, more through the table."""
        x = np.atleast_2d(np.asarray(x, dtype=float))
        if x.shape[0] <= _FEW_ROWS:
            gp, h = self._handle()
            return h.kg.rows(x, _normaliser(gp)[1]) * self._indicator(x)
        h, scale = self._table(x)
        return -h.kg.acq(scale) * self._indicator(x)

    def acquisition_function_withGradients(self, x):
        """The same and its gradient [M, D]; groups of up to 8 rows, one gp_kg_rows call each."""
        x = np.atleast_2d(np.asarray(x, dtype=float))
        gp, h = self._handle()
        scale = _normaliser(gp)[1]
        f, df = np.empty((x.shape[0], 1)), np.empty(x.shape)
        for k in range(0, x.shape[0], _FEW_ROWS):
            f[k:k + _FEW_ROWS], df[k:k + _FEW_ROWS] = h.kg.rows(x[k:k + _FEW_ROWS], scale, grad=True)
        ind = self._indicator(x)
        return f * ind, df * ind

    def _unconstrained(self):
        constrained = getattr(self.space, "has_constraints", None)
        return constrained is None or not constrained()

    def argbest(self, x, sense=-1, devices=None):
        """Row index and value of the best entry of ``acquisition_function(x)`` (sense -1: the smallest, i.e. the largest KG)."""
        if devices is not None:
            raise NotImplementedError("replica groups hold no discretisation points: the knowledge gradient scores its table on one device")
        x = np.atleast_2d(np.asarray(x, dtype=float))
        if not self._unconstrained():
            return _pick(self.acquisition_function(x)[:, 0], sense)
        h, scale = self._table(x)
        i, v = h.kg.acq_argbest(-sense, scale)       # the device's vector is +KG: the smallest -KG is its largest entry
        return i, -v

    def topk(self, x, k, sense=-1, devices=None):
        """The ``k`` best rows of ``acquisition_function(x)`` in order, (indices, values); equal scores lowest index first."""
        if devices is not None:
            raise NotImplementedError("replica groups hold no discretisation points: the knowledge gradient scores its table on one device")
        x = np.atleast_2d(np.asarray(x, dtype=float))
        if k > 64 or not self._unconstrained():
            return _host_topk(self.acquisition_function(x)[:, 0], k, sense)
        h, scale = self._table(x)
        idx, val = h.kg.acq_topk(-sense, k, scale)
        return idx, np.where(idx >= 0, -val, val)
