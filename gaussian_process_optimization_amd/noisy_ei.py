"""Noisy expected improvement (Letham, Karrer, Ottoni & Bakshy, "Constrained Bayesian optimization with noisy experiments",
2019): EI done right under noise.  With ``exact_feval=False`` the observations are noisy, and EI plugs the lowest posterior mean
at the data in as if it were a known incumbent.  NEI averages EI over S draws ("fantasies") of what the noiseless function values
at the observed points could have been,

    NEI(x) = (1 / S) sum_s EI(x | the GP conditioned on fantasy s, incumbent min_i F_is),

each draw with its own incumbent and its own conditioned posterior mean.  The draws are exact (Matheron's rule through the
model's factor and the factor of a near-noiseless TWIN of the same kernel), the S conditioned posteriors share one variance, and
the S fantasies collapse into one weight vector before the gradient's backward pass -- include/gphip.h spells all of it out.  Values
over tables, arg-best, top-k and the one-location calls with gradients run on the device (``gp_nei_*``; csrc/nei.hip,
csrc/api_nei.hip).  GPyOpt has nothing of the kind.

``AcquisitionNEI`` owns the twin handle.  Whenever the model's fit has changed it copies the inputs and the fitted kernel
parameters into the twin, fits it at noise ``twin_noise`` and draws the fantasies from standard normals of a generator seeded
once: column i of the draws belongs to observation i, so a model that grows keeps the numbers of the observations it had (common
random numbers across the iterations of a BO loop).
"""
import numpy as np

from . import _lib
from .acquisitions import AcquisitionBase, _host_topk, _normaliser, _pick
from .cost import constant_cost_withGradients
from .gpmodel import GPModel

_FEW_ROWS = _lib.GP_NEI_MAX_ROWS       # up to this many locations go down as ONE gp_nei_rows call (the fused rows path, gradients included)


def _refuse(what):
    return NotImplementedError("noisy expected improvement scores our exact GPModel with one output: %s" % what)


class FantasyDraws(object):
    """The standard normals behind the fantasies: ``Z``, ``E`` [S, N] from ONE generator, drawn a column (an observation) at a
    time -- ``take(N)`` with a larger N appends columns and redraws none, whatever the steps N grew in."""

    def __init__(self, num_fantasies, seed=None):
        self.S = int(num_fantasies)
        self.rng = np.random.RandomState(seed)
        self.Z = np.empty((self.S, 0))
        self.E = np.empty((self.S, 0))

    def take(self, N):
        have = self.Z.shape[1]
        if N > have:
            new = np.stack([self.rng.standard_normal((2, self.S)) for _ in range(N - have)], axis=2)      # [2, S, N - have]
            self.Z = np.concatenate([self.Z, new[0]], axis=1)
            self.E = np.concatenate([self.E, new[1]], axis=1)
        return np.ascontiguousarray(self.Z[:, :N]), np.ascontiguousarray(self.E[:, :N])


class AcquisitionNEI(AcquisitionBase):
    """Noisy expected improvement over ``num_fantasies`` (1 .. 64) draws of the noiseless values at the observations, through a
    twin fit at noise ``twin_noise`` (the value ``exact_feval=True`` uses).  ``acquisition_function`` returns -NEI, to be minimised,
    and ``acquisition_function_withGradients`` its gradient for up to 8 rows a call (what L-BFGS-B and the lockstep anchor
    optimiser ask).  Only the exact HIP ``GPModel`` with one output, a Euclidean kernel, no mean function and a noise above
    ``twin_noise`` is scored: ``exact_feval=True`` has no noise to integrate over (``ValueError``); a foreign, sparse, MCMC, warped
    or input-warped model, a Gower kernel, a mean function, a cost model, black-box constraints, local penalisation and replica
    groups raise ``NotImplementedError``."""
    analytical_gradient_prediction = True
    _takes_no_penaliser = ("noisy expected improvement is not penalised: the penaliser's Lipschitz constant and radii read one "
                           "incumbent, NEI has one per fantasy (use the 'sequential', 'random' or 'thompson_sampling' evaluator)")

    def __init__(self, model, space, optimizer=None, jitter=0.01, num_fantasies=16, twin_noise=1e-6, sampler_seed=None,
                 cost_withGradients=None, feasibility=None):
        if type(model) is not GPModel:
            raise _refuse("a foreign, MCMC, warped or input-warped model has no noisy expected improvement on the device")
        if getattr(model, "sparse", False):
            raise _refuse("not available with sparse=True")
        if model._gower():
            raise _refuse("not available with the Gower kernel")
        if getattr(model, "mean_function", None) is not None:
            raise _refuse("not available with a mean function")
        if getattr(model, "exact_feval", False):
            raise ValueError("noisy expected improvement integrates over the observation noise: exact_feval=True leaves none "
                             "(use acquisition_type 'EI')")
        if cost_withGradients is not None and cost_withGradients is not constant_cost_withGradients:
            raise NotImplementedError("noisy expected improvement takes no cost model: NEI per unit of cost is not implemented")
        if feasibility is not None:
            raise NotImplementedError("noisy expected improvement takes no black-box constraints: feasibility= weights EI and MPI")
        if not 1 <= int(num_fantasies) <= _lib.GP_NEI_MAX_S:
            raise ValueError("between 1 and %d fantasies, got %r" % (_lib.GP_NEI_MAX_S, num_fantasies))
        if not (float(twin_noise) > 0.0 and np.isfinite(twin_noise)):
            raise ValueError("twin_noise must be positive and finite, got %r" % (twin_noise,))
        super().__init__(model, space, optimizer)
        self.jitter, self.num_fantasies, self.twin_noise = float(jitter), int(num_fantasies), float(twin_noise)
        self.sampler_seed = sampler_seed
        self.draws = FantasyDraws(self.num_fantasies, sampler_seed)
        self.twin = None                # the twin's _lib.Handle, made at the first use (the model's device)
        self.refreshes = 0              # how often the twin was refitted and the fantasies redrawn through new factors (tests)
        self._fit_signature = None

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        return AcquisitionNEI(model, space, optimizer, jitter=config.get('jitter', 0.01),
                              num_fantasies=config.get('num_fantasies', 16), twin_noise=config.get('twin_noise', 1e-6),
                              sampler_seed=config.get('sampler_seed', None), cost_withGradients=cost_withGradients)

    def _set_feasibility(self, feasibility):
        if feasibility is not None:
            raise NotImplementedError("noisy expected improvement takes no black-box constraints: feasibility= weights EI and MPI")

    # ---- the twin ----------------------------------------------------------------------------------------------------------
    def _signature(self):
        """What the fantasies were drawn for: the GP object, its data and its parameters (AcquisitionKG._signature)."""
        gp = getattr(self.model, "model", None)
        return (id(gp), getattr(gp, "_data_epoch", None), np.asarray(getattr(gp, "param_array", ()), dtype=float).tobytes())

    def _resident(self):
        """The twin holds this acquisition's fantasies of the model's current fit (the library tells: it drops them with either
        factor)."""
        if self.twin is None:
            return False
        try:
            return self.twin.nei.info()[0] == self.num_fantasies
        except RuntimeError:            # GP_ERR_STATE: the model was refitted since
            return False

    def _handle(self):
        """(the model's GP, the twin's handle) with the fantasies of the model's current fit resident on the twin."""
        gp = self.model.model
        if gp is None:
            raise RuntimeError("the model has no data yet: updateModel first")
        if gp.output_dim != 1:
            raise _refuse("the model has %d outputs" % gp.output_dim)
        if getattr(gp.kern, "Gower", False):
            raise _refuse("not available with the Gower kernel")
        gp._ensure_fit()
        sig = self._signature()
        if self._fit_signature != sig or not self._resident():
            noise = float(gp.likelihood.variance)
            if not noise > self.twin_noise:
                raise ValueError("noisy expected improvement needs a model noise above twin_noise: %.3e against %.3e (a model "
                                 "this clean is scored by 'EI')" % (noise, self.twin_noise))
            if self.twin is None:
                self.twin = _lib.Handle(gp._h.device)
            k = gp.kern
            self.twin.set_data(gp.X, gp.Y_normalized)            # (the twin's targets are not read)
            self.twin.set_gower()
            self.twin.set_params(k._kernel_id, k.ARD, float(k.variance), k.lengthscale.values, self.twin_noise)
            self.twin.fit(gp.max_jitter_tries)
            gp._ensure_fit()
            Z, E = self.draws.take(gp.X.shape[0])
            self.twin.nei.set(gp._h, Z, E)
            self._fit_signature = self._signature()
            self.refreshes += 1
        return gp, self.twin

    def fantasies(self):
        """(F [S, N], fstar [S]): the fantasies of the noiseless values at the observations and their minima, un-normalised."""
        gp, h = self._handle()
        F, fstar = h.nei.get()
        shift, scale = _normaliser(gp)
        return F * scale + shift, fstar * scale + shift

    # ---- the contract ------------------------------------------------------------------------------------------------------
    def _indicator(self, x):
        constrained = getattr(self.space, "has_constraints", None)
        if constrained is None or not constrained():
            return 1.0
        return self.space.indicator_constraints(x)

    def _unconstrained(self):
        constrained = getattr(self.space, "has_constraints", None)
        return constrained is None or not constrained()

    def _table(self, x):
        """``x`` as the twin's resident candidates: (twin handle, (jitter, y_mean, y_std))."""
        gp, h = self._handle()
        h.set_candidates(x)
        return h, (self.jitter,) + _normaliser(gp)

    def acquisition_function(self, x):
        """-NEI of every row of ``x``, [M, 1]: up to 8 rows as ONE gp_nei_rows call, more through the table."""
        x = np.atleast_2d(np.asarray(x, dtype=float))
        if x.shape[0] <= _FEW_ROWS:
            gp, h = self._handle()
            return h.nei.rows(x, self.jitter, *_normaliser(gp)) * self._indicator(x)
        h, args = self._table(x)
        return -h.nei.table(*args) * self._indicator(x)

    def acquisition_function_withGradients(self, x):
        """The same and its gradient [M, D]; groups of up to 8 rows, one gp_nei_rows call each."""
        x = np.atleast_2d(np.asarray(x, dtype=float))
        gp, h = self._handle()
        shift, scale = _normaliser(gp)
        f, df = np.empty((x.shape[0], 1)), np.empty(x.shape)
        for k in range(0, x.shape[0], _FEW_ROWS):
            f[k:k + _FEW_ROWS], df[k:k + _FEW_ROWS] = h.nei.rows(x[k:k + _FEW_ROWS], self.jitter, shift, scale, grad=True)
        ind = self._indicator(x)
        return f * ind, df * ind

    def argbest(self, x, sense=-1, devices=None):
        """Row index and value of the best entry of ``acquisition_function(x)`` (sense -1: the smallest, i.e. the largest NEI)."""
        if devices is not None:
            raise NotImplementedError("replica groups hold no fantasies: noisy expected improvement scores its table on one device")
        x = np.atleast_2d(np.asarray(x, dtype=float))
        if not self._unconstrained():
            return _pick(self.acquisition_function(x)[:, 0], sense)
        h, args = self._table(x)
        i, v = h.nei.argbest(-sense, *args)       # the device's vector is +NEI: the smallest -NEI is its largest entry
        return i, -v

    def topk(self, x, k, sense=-1, devices=None):
        """The ``k`` best rows of ``acquisition_function(x)`` in order, (indices, values); equal scores lowest index first."""
        if devices is not None:
            raise NotImplementedError("replica groups hold no fantasies: noisy expected improvement scores its table on one device")
        x = np.atleast_2d(np.asarray(x, dtype=float))
        if k > 64 or not self._unconstrained():
            return _host_topk(self.acquisition_function(x)[:, 0], k, sense)
        h, args = self._table(x)
        idx, val = h.nei.topk(-sense, k, *args)
        return idx, np.where(idx >= 0, -val, val)
