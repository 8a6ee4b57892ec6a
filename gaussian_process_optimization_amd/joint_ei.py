"""The joint (batch) expected improvement qEI: a batch of q points scored as a whole.

    qEI(x_1 .. x_q) = E[max(0, max_j (f_min - jitter - y_j))]

over the JOINT posterior of the q locations, estimated by Monte Carlo with fixed base samples (sample-average approximation;
Ginsbourger, Le Riche & Carraro 2010; Wang, Clark, Liu & Frazier 2016; Wilson, Hutter & Deisenroth 2018).  With the samples fixed
the estimate is a deterministic, differentiable function of the q D coordinates, which L-BFGS-B optimises.  Value and gradient are
ONE ``gp_qei_rows`` call (csrc/qei.hip, csrc/api_qei.hip): the fused rows path's passes over the inverse factor for all q locations
at once, the q x q factorisation with the reduction over the samples and its adjoint in one workgroup, a closing pass over the
training points.  GPyOpt has nothing of the kind: its batch evaluators build a batch one point at a time.

``AcquisitionQEI`` is an acquisition over BATCHES: ``acquisition_function(X)`` takes rows of q D flattened coordinates (row-major,
location by location).  ``optimize()`` returns the batch ``[q, D]``; ``JointBatch`` is the evaluator whose ``compute_batch`` is that
call (``BayesianOptimization(acquisition_type='qEI', batch_size=q)``).
"""
import numpy as np
from scipy import optimize as _sopt

from . import _lib
from .acquisitions import AcquisitionBase, AcquisitionEI, _normaliser
from .cost import constant_cost_withGradients
from .gpmodel import GPModel

NUM_CANDIDATES = 1000     # random candidates scored by marginal EI for the starts (anchor_points_generator.py:19-63)
NUM_RANDOM_STARTS = 4     # random q-subsets of the best 5 q candidates, besides the q best


def _refuse(what):
    return NotImplementedError("joint expected improvement scores batches over our exact GPModel with one output: %s" % what)


class AcquisitionQEI(AcquisitionBase):
    """Joint expected improvement of ``batch_size`` points over ``num_samples`` base samples, drawn once per object from ``seed``
    and resident on the model's handle (re-sent only when the handle changes: common random numbers across refits).  ``jitter`` is
    the improvement margin, noise, f_min and the output normaliser are taken as ``AcquisitionEI`` takes them.  Only the exact HIP
    ``GPModel`` with one output, a Euclidean kernel and no mean function is scored; a sparse, MCMC, warped, input-warped, Gower,
    mean-function or foreign model, a cost model and black-box constraints raise ``NotImplementedError``."""
    analytical_gradient_prediction = True

    def __init__(self, model, space, optimizer=None, batch_size=2, num_samples=256, jitter=0.01, seed=None,
                 cost_withGradients=None, feasibility=None):
        if type(model) is not GPModel:
            raise _refuse("a foreign, MCMC, warped or input-warped model has no joint posterior on the device")
        if getattr(model, "sparse", False):
            raise _refuse("not available with sparse=True")
        if model._gower():
            raise _refuse("not available with the Gower kernel")
        if getattr(model, "mean_function", None) is not None:
            raise _refuse("not available with a mean function")
        if cost_withGradients is not None and cost_withGradients is not constant_cost_withGradients:
            raise NotImplementedError("joint expected improvement takes no cost model: the batch has no single cost to divide by")
        if feasibility is not None:
            raise NotImplementedError("joint expected improvement takes no black-box constraints: feasibility= weights EI and MPI")
        if not 1 <= int(batch_size) <= _lib.GP_QEI_MAX_Q:
            raise ValueError("between 1 and %d points in a batch, got %r" % (_lib.GP_QEI_MAX_Q, batch_size))
        if not 1 <= int(num_samples) <= _lib.GP_QEI_MAX_S:
            raise ValueError("between 1 and %d base samples, got %r" % (_lib.GP_QEI_MAX_S, num_samples))
        super().__init__(model, space, optimizer)
        self.batch_size, self.num_samples, self.jitter, self.seed = int(batch_size), int(num_samples), jitter, seed
        self.Z = np.random.default_rng(seed).standard_normal((self.num_samples, self.batch_size))
        self.Z.setflags(write=False)
        self._key = (id(self), self.num_samples, self.batch_size)
        self._starts_rng = np.random.RandomState(seed)      # candidates and start subsets: reproducible from ``seed``
        self._ei = AcquisitionEI(model, space, optimizer, jitter=jitter)      # marginal EI: scores the candidates of the starts
        self.uploads = 0                # how often the base samples went to a handle (tests)
        self.last_starts = None         # [n_starts, q, D] of the last optimize(), and their (negated) values
        self.last_start_values = None

    @staticmethod
    def fromConfig(model, space, optimizer, cost_withGradients, config):
        return AcquisitionQEI(model, space, optimizer, batch_size=config.get('batch_size', 2),
                              num_samples=config.get('num_qei_samples', 256), jitter=config.get('jitter', 0.01),
                              seed=config.get('sampler_seed', None), cost_withGradients=cost_withGradients)

    def _set_feasibility(self, feasibility):
        if feasibility is not None:
            raise NotImplementedError("joint expected improvement takes no black-box constraints: feasibility= weights EI and MPI")

    # ---- the call ------------------------------------------------------------------------------------------------------------
    def _handle(self):
        """The model's handle with a current fit and this object's base samples resident."""
        gp = self.model.model
        if gp is None:
            raise RuntimeError("the model has no data yet: updateModel first")
        if gp.output_dim != 1:
            raise _refuse("the model has %d outputs" % gp.output_dim)
        if getattr(gp.kern, "Gower", False):
            raise _refuse("not available with the Gower kernel")
        gp._ensure_fit()
        h = gp._h
        if getattr(h, "qei_key", None) != self._key:
            h.qei_set(self.Z, key=self._key)
            self.uploads += 1
        return gp, h

    def batches(self, X):
        """Rows of q D flattened coordinates -> [rows, q, D]."""
        X = np.asarray(X, dtype=float)
        X = X[None, :] if X.ndim == 1 else X
        D = self.space.dimensionality if hasattr(self.space, "dimensionality") else X.shape[1] // self.batch_size
        if X.ndim != 2 or X.shape[1] != self.batch_size * D:
            raise ValueError("expected rows of q * D = %d * %d flattened coordinates, got shape %s" % (self.batch_size, D, X.shape))
        return X.reshape(X.shape[0], self.batch_size, D)

    def _indicator(self, B):
        constrained = getattr(self.space, "has_constraints", None)
        if constrained is None or not constrained():
            return 1.0
        return float(np.all(self.space.indicator_constraints(B) > 0))

    def _score(self, X, grad):
        B = self.batches(X)
        gp, h = self._handle()
        shift, scale = _normaliser(gp)
        fmin = self.model.get_fmin()
        f = np.empty((B.shape[0], 1))
        df = np.empty((B.shape[0], B.shape[1] * B.shape[2])) if grad else None
        for r in range(B.shape[0]):
            ind = self._indicator(B[r])
            res = h.qei_rows(B[r], self.jitter, fmin, shift, scale, include_noise=True, grad=grad)      # LinAlgError: a pivot
            if grad:
                f[r, 0], df[r] = res[0] * ind, res[1].ravel() * ind
            else:
                f[r, 0] = res * ind
        return (f, df) if grad else f

    def acquisition_function(self, x):
        """-qEI of every row of ``x`` (q D flattened coordinates each), [rows, 1]: one gp_qei_rows call per row."""
        return self._score(x, False)

    def acquisition_function_withGradients(self, x):
        """The same and its gradient [rows, q D]."""
        return self._score(x, True)

    def argbest(self, x, sense=-1, devices=None):
        v = self.acquisition_function(x)[:, 0]
        i = int(np.argmin(v) if sense < 0 else np.argmax(v))
        return i, float(v[i])

    def topk(self, x, k, sense=-1, devices=None):
        raise NotImplementedError("joint expected improvement scores batches: there is no table of single locations to rank")

    # ---- the optimiser ---------------------------------------------------------------------------------------------------------
    def tiled_bounds(self):
        """The space's bounds, once per point of the batch: the box of the q D variables."""
        return list(self.space.get_bounds()) * self.batch_size

    def starts(self):
        """[1 + NUM_RANDOM_STARTS, q, D]: the q best of NUM_CANDIDATES uniform candidates under marginal EI (ranked on the device,
        gp_acq_topk), then random q-subsets of the best 5 q."""
        q = self.batch_size
        n = getattr(self.optimizer, "num_samples", None) or NUM_CANDIDATES
        X = self.space.samples_uniform(max(int(n), 5 * q), self._starts_rng)
        idx, _ = self._ei.topk(X, 5 * q, sense=-1)
        idx = np.asarray(idx)[np.asarray(idx) >= 0]
        best = X[idx]
        out = [best[:q]]
        for _ in range(NUM_RANDOM_STARTS):
            out.append(best[np.sort(self._starts_rng.choice(best.shape[0], q, replace=False))])
        return np.stack(out)

    def optimize(self, duplicate_manager=None):
        """L-BFGS-B over the q D variables from every start; the best batch, rounded row by row: (x [q, D], -qEI of it)."""
        if duplicate_manager is not None:
            raise NotImplementedError("duplicate managers are outside the accelerated path")
        S = self.starts()
        q, D = S.shape[1], S.shape[2]
        bounds = self.tiled_bounds()
        maxiter = getattr(self.optimizer, "maxiter", None) or 1000

        def f_df(x):
            f, df = self.acquisition_function_withGradients(x[None, :])
            return float(f[0, 0]), df[0]

        self.last_starts, self.last_start_values = S, np.array([f_df(s.ravel())[0] for s in S])
        best_x, best_f = None, np.inf
        for s in S:
            res = _sopt.fmin_l_bfgs_b(f_df, x0=s.ravel(), bounds=bounds, maxiter=maxiter)
            x, fx = res[0], float(res[1])
            if res[2].get('task', b'') in (b'ABNORMAL_TERMINATION_IN_LNSRCH', 'ABNORMAL_TERMINATION_IN_LNSRCH'):
                x, fx = s.ravel(), f_df(s.ravel())[0]
            if fx < best_f:
                best_x, best_f = x, fx
        x = np.vstack([self.space.round_optimum(row) for row in best_x.reshape(q, D)])      # optimizer.py:130-168, row by row
        if not np.array_equal(x.ravel(), best_x):
            best_f = float(self.acquisition_function(x.ravel())[0, 0])                     # the value of what is returned
        return x, np.array([[best_f]])


class JointBatch(object):
    """The evaluator of ``AcquisitionQEI``: the batch is the optimum of the joint acquisition itself."""

    def __init__(self, acquisition, batch_size):
        if not isinstance(acquisition, AcquisitionQEI):
            raise TypeError("JointBatch returns the batch an AcquisitionQEI optimises")
        if int(batch_size) != acquisition.batch_size:
            raise ValueError("the acquisition scores batches of %d, the evaluator was asked for %d" % (acquisition.batch_size, batch_size))
        self.acquisition, self.batch_size, self.space = acquisition, int(batch_size), acquisition.space

    def compute_batch(self, duplicate_manager=None, context_manager=None):
        if duplicate_manager is not None or context_manager is not None:
            raise NotImplementedError("duplicate / context managers are outside the accelerated path")
        return self.acquisition.optimize()[0]
