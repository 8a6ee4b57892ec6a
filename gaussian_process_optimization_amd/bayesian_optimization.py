"""``BayesianOptimization`` facade mirroring GPyOpt's entry point for the GP path.

Reference: GPyOpt/GPyOpt/methods/bayesian_optimization.py:76-170 (constructor keywords),
GPyOpt/GPyOpt/util/arguments_manager.py:42-147 (kwargs -> objects: kernel, ARD, noise_var,
model_optimizer_type, max_iters, optimize_restarts, acquisition_jitter=0.01,
acquisition_weight=2), GPyOpt/GPyOpt/core/bo.py:55-71 (suggest_next_locations), :73-168
(run_optimization), :216-254 (_compute_next_evaluations / _update_model, Y normalised with
util/general.py:203-234), GPyOpt/GPyOpt/optimization/acquisition_optimizer.py:46-77 and
anchor_points_generator.py:19-98 (1000 random candidates scored in ONE batched call, best 5
anchors, L-BFGS-B from each), optimizer.py:28-61 (scipy fmin_l_bfgs_b).

Only the GP model type and the EI / LCB / MPI acquisitions with the sequential evaluator are
on the accelerated path; the design space here covers continuous and discrete variables
(bounds, rounding).  Everything numeric -- fit, batched scoring, arg-best -- runs on the GPU.
"""
import time

import numpy as np
from scipy import optimize as _sopt

from . import kern as _kern
from .acquisitions import (AcquisitionEI, AcquisitionLCB, AcquisitionMPI, AcquisitionLP, LocalPenalization, AcquisitionEI_MCMC,
                           AcquisitionMPI_MCMC, AcquisitionLCB_MCMC, AcquisitionEntropySearch, AcquisitionMES, AcquisitionTS)
from .cost import CostModel
from .feasibility import FeasibilityModel
from .entropy_search import AffineInvariantEnsembleSampler
from .gpmodel import GPModel
from .input_warped_gp import InputWarpedGPModel
from .joint_ei import AcquisitionQEI, JointBatch
from .knowledge_gradient import AcquisitionKG
from .noisy_ei import AcquisitionNEI
from .parameterization import lbfgsb_lockstep, SCIPY_DEFAULT


class InvalidConfigError(Exception):
    """GPyOpt/GPyOpt/core/errors.py: a combination of options the loop cannot run."""


def normalize(Y, normalization_type='stats'):
    """GPyOpt/GPyOpt/util/general.py:203-234."""
    Y = np.asarray(Y, dtype=float)
    if np.max(Y.shape) != Y.size:
        raise NotImplementedError('Only 1-dimensional arrays are supported.')
    if normalization_type == 'stats':
        Y_norm = Y - Y.mean()
        std = Y.std()
        if std > 0:
            Y_norm /= std
    elif normalization_type == 'maxmin':
        Y_norm = Y - Y.min()
        y_range = np.ptp(Y)
        if y_range > 0:
            Y_norm /= y_range
            Y_norm = 2 * (Y_norm - 0.5)
    else:
        raise ValueError('Unknown normalization type: {}'.format(normalization_type))
    return Y_norm


class Design_space(object):
    """Continuous / discrete box domain (subset of GPyOpt/GPyOpt/core/task/space.py:13-532)."""

    def __init__(self, space, constraints=None):
        # space.py:303-318: every constraint is the body of ``lambda x: ...`` over the 2-D array of locations; a
        # location is feasible where the expression is < 0.  Compiled once here (the reference re-execs per call).
        self.constraints = constraints
        self._constraint_fns = []
        for d in (constraints or []):
            try:
                self._constraint_fns.append(eval('lambda x: ' + d['constraint'], {'np': np, 'numpy': np}))
            except Exception:
                print('Fail to compile the constraint: ' + str(d))
                raise
        self.config_space = space
        self.names, self.types, self.domains = [], [], []
        for i, v in enumerate(space):
            n = int(v.get('dimensionality', 1))
            for k in range(n):
                self.names.append(v.get('name', 'var_%d' % i) + ('_%d' % k if n > 1 else ''))
                self.types.append(v.get('type', 'continuous'))
                self.domains.append(tuple(v['domain']))
        for t in self.types:
            if t not in ('continuous', 'discrete'):
                raise NotImplementedError("variable type %r is outside the accelerated path" % t)
        self.dimensionality = len(self.names)
        self.model_dimensionality = self.dimensionality

    def has_constraints(self):
        """space.py:226-230."""
        return self.constraints is not None

    def indicator_constraints(self, x):
        """space.py:303-318: ones / zeros [M, 1]."""
        x = np.atleast_2d(x)
        I_x = np.ones((x.shape[0], 1))
        for fn, d in zip(self._constraint_fns, self.constraints or []):
            try:
                ind_x = (np.asarray(fn(x)) < 0) * 1
                I_x *= ind_x.reshape(x.shape[0], 1)
            except Exception:
                print('Fail to compile the constraint: ' + str(d))
                raise
        return I_x

    def get_bounds(self):
        return [(min(d), max(d)) for d in self.domains]

    def round_optimum(self, x):
        """space.py:328-349: discrete variables snap to the closest admissible value."""
        x = np.array(x, dtype=float).reshape(-1)
        for i, (t, d) in enumerate(zip(self.types, self.domains)):
            if t == 'discrete':
                dom = np.asarray(d, dtype=float)
                x[i] = dom[np.argmin(np.abs(dom - x[i]))]
            else:
                x[i] = min(max(x[i], d[0]), d[1])
        return x[None, :]

    # -- the fork's additions for the Gower kernel (space.py:351-362,436-445,483-492) -------------------
    def get_continuous_dims(self):
        return [i for i, t in enumerate(self.types) if t == 'continuous']

    def get_discrete_dims(self):
        return [i for i, t in enumerate(self.types) if t == 'discrete']

    def lengthscales(self):
        """Ranges of the continuous variables, in order (space.py:351-362)."""
        return [d[-1] - d[0] for t, d in zip(self.types, self.domains) if t == 'continuous']

    def samples_uniform(self, n, rng=np.random):
        """experiment_design/random_design.py:15-35: rejection sampling when the space has constraints."""
        if not self.has_constraints():
            return self._samples_box(n, rng)
        samples = np.empty((0, self.dimensionality))
        while samples.shape[0] < n:
            Z = self._samples_box(n, rng)
            ok = (self.indicator_constraints(Z) == 1).flatten()
            if ok.sum() > 0:
                samples = np.vstack((samples, Z[ok, :]))
        return samples[0:n, :]

    def _samples_box(self, n, rng=np.random):
        """experiment_design/random_design.py:37-65: every discrete variable first (one ``choice`` call each, in order), then
        every continuous one (one ``uniform`` call each, in order) -- the reference's consumption of the generator, so that a
        seeded run draws the reference's design whatever the order of the variables."""
        Z = np.empty((n, self.dimensionality))
        for i, (t, d) in enumerate(zip(self.types, self.domains)):
            if t == 'discrete':
                Z[:, i] = rng.choice(np.asarray(d, dtype=float), n)
        for i, (t, d) in enumerate(zip(self.types, self.domains)):
            if t != 'discrete':
                Z[:, i] = rng.uniform(d[0], d[1], n)
        return Z


class AcquisitionOptimizer(object):
    """optimization/acquisition_optimizer.py:46-77 with ObjectiveAnchorPointsGenerator (:85-98)."""

    def __init__(self, space, optimizer='lbfgs', num_samples=1000, num_anchor=5, maxiter=1000, parallel=False):
        """``parallel``: the L-BFGS runs from the anchors advance in lockstep (``_lbfgs_from_anchors``) instead of one after
        the other -- with ``f_df`` and the 'lbfgs' optimiser; anything else runs the serial loop."""
        self.space = space
        self.parallel = parallel
        self.optimizer_name = optimizer
        self.num_samples = num_samples
        self.num_anchor = num_anchor
        self.maxiter = maxiter

    def optimize(self, f=None, df=None, f_df=None, duplicate_manager=None):
        X = self.space.samples_uniform(self.num_samples)
        scores = f(X).flatten()                       # ONE batched call (anchor_points_generator.py:59)
        anchors = X[np.argsort(scores)[:min(len(scores), self.num_anchor)], :]
        bounds = self.space.get_bounds()
        best_x, best_fx = None, np.inf
        if self.lockstep(f_df):
            xs = _lbfgs_from_anchors(self.space, anchors, f_df, self.maxiter)
            for k in range(0, len(xs), LOCKSTEP_GROUP):          # the rounded optima of a group scored in ONE call
                fxs = np.asarray(f(np.vstack(xs[k:k + LOCKSTEP_GROUP])), dtype=float).ravel()
                for x, fx in zip(xs[k:k + LOCKSTEP_GROUP], fxs):
                    if float(fx) < best_fx:
                        best_x, best_fx = x, float(fx)
            return best_x, best_fx
        for a in anchors:
            if f_df is not None and self.optimizer_name == 'lbfgs':
                def _f_df(x):                        # optimizer.py:45-47
                    fx, dfx = f_df(np.atleast_2d(x))
                    return float(np.asarray(fx).ravel()[0]), np.asarray(dfx, dtype=float).ravel()
                res = _sopt.fmin_l_bfgs_b(_f_df, x0=a, bounds=bounds, maxiter=self.maxiter)
            else:
                res = _sopt.fmin_l_bfgs_b(lambda x: float(f(np.atleast_2d(x)).ravel()[0]), x0=a, bounds=bounds,
                                          approx_grad=True, maxiter=self.maxiter)
            x = np.atleast_2d(res[0])
            if res[2].get('task', b'') in (b'ABNORMAL_TERMINATION_IN_LNSRCH', 'ABNORMAL_TERMINATION_IN_LNSRCH'):
                x = np.atleast_2d(a)                  # optimizer.py:53-59
            x = self.space.round_optimum(x)           # optimizer.py:130-168 (apply_optimizer)
            fx = float(f(x).ravel()[0])
            if fx < best_fx:
                best_x, best_fx = x, fx
        return best_x, best_fx

    def lockstep(self, f_df):
        """True when the anchors are refined in lockstep: asked for, gradients at hand, L-BFGS."""
        return bool(self.parallel) and f_df is not None and self.optimizer_name == 'lbfgs'


LOCKSTEP_GROUP = 8      # anchors per lockstep group: what ONE gp_acq_rows call takes (acquisitions._FEW_ROWS)


def _lbfgs_from_anchors(space, anchors, f_df, maxiter=1000, indexed=False):
    """``_lbfgs_from_anchor`` for every anchor, the runs of a group of up to ``LOCKSTEP_GROUP`` anchors advancing in lockstep
    (parameterization.lbfgsb_lockstep): each round's posted points go to ``f_df`` as the rows of ONE call.  A row's value and
    gradient do not depend on its company (include/gphip.h, gp_*_rows), so every run takes the steps its serial run takes;
    the abnormal-line-search fallback and ``round_optimum`` are applied per anchor.  Returns the [1, D] optima in anchor order.
    ``indexed``: every anchor has an objective of its own -- ``f_df(xs, which)`` also gets the anchors the rows belong to."""
    bounds = space.get_bounds()
    anchors = [np.asarray(a, dtype=float) for a in anchors]
    out = []
    for k in range(0, len(anchors), LOCKSTEP_GROUP):
        def fbatch(xs, idx=None, k=k):
            fx, dfx = f_df(xs, k + np.asarray(idx)) if indexed else f_df(xs)
            return np.asarray(fx, dtype=float).reshape(-1), np.asarray(dfx, dtype=float).reshape(xs.shape[0], -1)

        group = anchors[k:k + LOCKSTEP_GROUP]
        for a, res in zip(group, lbfgsb_lockstep(fbatch, group, max_iters=maxiter, bounds=bounds, maxfun=SCIPY_DEFAULT,
                                                 with_index=indexed)):
            if isinstance(res, BaseException):
                raise res
            x = np.atleast_2d(res[0])
            if res[2].get('task', b'') in (b'ABNORMAL_TERMINATION_IN_LNSRCH', 'ABNORMAL_TERMINATION_IN_LNSRCH'):
                x = np.atleast_2d(a)
            out.append(space.round_optimum(x))
    return out


def _lbfgs_from_anchor(space, a, f, f_df, maxiter=1000):
    """optimizer.py:36-59 + apply_optimizer :130-168: one bounded L-BFGS run from anchor ``a``."""
    def _f_df(x):
        fx, dfx = f_df(np.atleast_2d(x))
        return float(np.asarray(fx).ravel()[0]), np.asarray(dfx, dtype=float).ravel()
    res = _sopt.fmin_l_bfgs_b(_f_df, x0=a, bounds=space.get_bounds(), maxiter=maxiter)
    x = np.atleast_2d(res[0])
    if res[2].get('task', b'') in (b'ABNORMAL_TERMINATION_IN_LNSRCH', 'ABNORMAL_TERMINATION_IN_LNSRCH'):
        x = np.atleast_2d(a)
    return space.round_optimum(x)


class ThompsonSamplingAnchorPointsGenerator(object):
    """optimization/anchor_points_generator.py:66-82: marginal Thompson sampling.  ONE batched device
    predict over ``num_samples`` random locations, one normal draw per location from its own (mean, sd),
    the ``num_anchor`` lowest draws are the anchors (:19-63)."""

    def __init__(self, space, design_type, model, num_samples=25000):
        self.space, self.design_type, self.model, self.num_samples = space, design_type, model, num_samples

    def get_anchor_point_scores(self, X):
        m, s = self.model.predict(X)
        return np.random.normal(m.ravel(), s.ravel())

    def get(self, num_anchor=5, duplicate_manager=None, unique=False, context_manager=None):
        X = self.space.samples_uniform(self.num_samples)
        scores = self.get_anchor_point_scores(X)
        return X[np.argsort(scores)[:min(len(scores), num_anchor)], :]


class RandomAnchorPointsGenerator(object):
    """anchor_points_generator.py:100-113: every sample scores the same, i.e. the first ``num_anchor`` rows."""

    def __init__(self, space, design_type, num_samples=10000):
        self.space, self.num_samples = space, num_samples

    def get(self, num_anchor=5, duplicate_manager=None, unique=False, context_manager=None):
        X = self.space.samples_uniform(self.num_samples)
        return X[np.argsort(np.arange(X.shape[0]), kind='stable')[:num_anchor], :]


class SamplingBasedBatchEvaluator(object):
    """core/evaluators/base.py:21-92 without the duplicate manager (de_duplication is host bookkeeping)."""

    def __init__(self, acquisition, batch_size):
        self.acquisition, self.batch_size, self.space = acquisition, batch_size, acquisition.space
        self.num_anchor = 5 * batch_size

    def compute_batch(self, duplicate_manager=None, context_manager=None):
        if duplicate_manager is not None or context_manager is not None:
            raise NotImplementedError("duplicate / context managers are outside the accelerated path")
        return self.compute_batch_without_duplicate_logic()


class ThompsonBatch(SamplingBasedBatchEvaluator):
    """core/evaluators/batch_thompson.py:9-55: anchors by marginal Thompson sampling on the model, each of
    the first ``batch_size`` anchors refined by L-BFGS on the acquisition."""

    def __init__(self, acquisition, batch_size):
        super(ThompsonBatch, self).__init__(acquisition, batch_size)
        self.model = acquisition.model
        self.f, self.f_df = acquisition.acquisition_function, acquisition.acquisition_function_withGradients

    def get_anchor_points(self):
        return ThompsonSamplingAnchorPointsGenerator(self.space, "random", self.model).get(num_anchor=self.num_anchor)

    def optimize_anchor_point(self, a):
        return _lbfgs_from_anchor(self.space, a, self.f, self.f_df)

    def compute_batch_without_duplicate_logic(self):
        anchors = self.get_anchor_points()[:self.batch_size]
        optimizer = self.acquisition.optimizer
        if optimizer is not None and optimizer.lockstep(self.f_df):
            return np.vstack(_lbfgs_from_anchors(self.space, anchors, self.f_df))
        return np.vstack([self.optimize_anchor_point(a) for a in anchors])


class ThompsonPathsBatch(SamplingBasedBatchEvaluator):
    """The batch of ``AcquisitionTS`` (no counterpart in the reference): ``batch_size`` posterior paths are drawn, element b is
    the minimiser of path b -- its anchor the best of ``num_samples`` uniform locations under ITS path (its own column of one
    anchor table), refined by L-BFGS on that path.  Distinct joint samples spread the batch by themselves: no penaliser.  With the
    optimiser in lockstep mode the B runs advance together, each round's points going down as ONE gp_paths_rows call per group
    of eight, row i on path i."""

    def __init__(self, acquisition, batch_size, num_samples=1000):
        if not isinstance(acquisition, AcquisitionTS):
            raise TypeError("ThompsonPathsBatch spreads a batch over the paths of an AcquisitionTS")
        super(ThompsonPathsBatch, self).__init__(acquisition, batch_size)
        self.num_samples = num_samples

    def get_anchor_points(self):
        """[batch_size, D]: per path the lowest row of one table of uniform locations (reduced on the device)."""
        acq = self.acquisition
        X = self.space.samples_uniform(self.num_samples)
        if acq._indicator(X) is not None:
            rows = np.argmin(acq.table_on_paths(X), axis=0)
        else:
            h, shift, scale = acq._table(X)
            rows = h.paths_argbest(-1, shift, scale)[0]
        return X[rows, :]

    def compute_batch_without_duplicate_logic(self):
        acq, B = self.acquisition, self.batch_size
        acq.redraw(num_paths=B)
        anchors = self.get_anchor_points()
        optimizer = acq.optimizer
        if optimizer is not None and optimizer.lockstep(acq.acquisition_function_withGradients):
            # a round's rows are the runs still going: each on the path of its own anchor
            return np.vstack(_lbfgs_from_anchors(self.space, anchors, lambda xs, which: acq.values_on_paths(xs, which, grad=True),
                                                 indexed=True))
        out = []
        for b in range(B):
            out.append(_lbfgs_from_anchor(self.space, anchors[b], None, lambda x, p=b: acq.values_on_paths(x, p, grad=True)))
        return np.vstack(out)


class RandomBatch(SamplingBasedBatchEvaluator):
    """core/evaluators/batch_random.py:9-48: first element = the optimised acquisition, the rest uniform."""

    def compute_batch_without_duplicate_logic(self):
        x, _ = self.acquisition.optimize()
        k = self.batch_size - 1
        anchors = RandomAnchorPointsGenerator(self.space, "random").get(num_anchor=self.num_anchor)
        return np.vstack([x] + [a for a, _ in zip(anchors, range(k))])


KERNEL_NAMES = {'RBF': _kern.RBF, 'ExpQuad': _kern.ExpQuad, 'Matern52': _kern.Matern52, 'Matern32': _kern.Matern32,
                'Exponential': _kern.Exponential, 'OU': _kern.OU}


def kernel_from_name(name, input_dim, ARD=False):
    """The kernel object behind ``BayesianOptimization(kernel='<name>')``."""
    if name not in KERNEL_NAMES:
        raise ValueError("unknown kernel %r: choose one of %s" % (name, ", ".join(sorted(KERNEL_NAMES))))
    return KERNEL_NAMES[name](input_dim, ARD=ARD)


def _clock():
    """Wall-clock seconds: what the evaluation times of ``cost_withGradients='evaluation_time'`` are differences of."""
    return time.time()


class BayesianOptimization(object):
    """GPyOpt.methods.BayesianOptimization for model_type='GP' and 'input_warped_GP' (bayesian_optimization.py:76-170).

    Black-box constraints (an addition): ``constraint_function(X) -> [n, K]`` is evaluated wherever ``f`` is (``C`` holds the
    values of the initial design, for ``f=None`` use), a location is feasible where every column is ``<= constraint_bounds``
    (a scalar or one bound per column); ``constraint_kinds`` names each column ``'value'`` (the default) or ``'binary'`` -- a
    yes / no outcome, 1 where the constraint was violated and 0 where it was satisfied, modelled by a GP classifier
    (``FeasibilityModel(kinds=...)``).  A ``FeasibilityModel`` -- one exact GP per constraint -- is refitted with the surrogate
    and EI / MPI score ``a(x) F(x)`` with the incumbent over the feasible observations (``feasibility.py``).  ``x_opt`` /
    ``fx_opt`` are then the best FEASIBLE observation; while there is none they are the LEAST VIOLATING one: the observation
    with the smallest total violation ``sum_k max(c_k - bound_k, 0) / std_k`` (``std_k`` the standard deviation of column k over
    the observations), the lowest objective among equals.  The evaluators 'sequential', 'random' and 'thompson_sampling' work;
    'local_penalization' raises ``InvalidConfigError`` (its optimiser needs penalised rows, which take no constraints).

    Max-value entropy search (an addition): ``acquisition_type='MES'`` with the keywords ``num_min_samples`` (10 samples of the
    minimum's value), ``mes_grid_size`` (10000 uniform locations under the sampler, besides X) and ``sampler_seed``
    (``AcquisitionMES``).  It has gradients, so every evaluator works with it, 'local_penalization' and ``parallel_anchors=True``
    included, and so does ``cost_withGradients='evaluation_time'``; with ``constraint_function`` it raises
    ``NotImplementedError``.

    Thompson sampling proper (an addition): ``acquisition_type='TS'`` with the keywords ``num_features`` (1024 random Fourier
    features of the prior term) and ``sampler_seed`` minimises a sample of the posterior FUNCTION (``AcquisitionTS``, posterior
    paths).  'sequential' draws one fresh path per suggestion; 'thompson_sampling' with ``batch_size`` B draws B paths and
    returns the minimiser of each (``ThompsonPathsBatch``); 'local_penalization', a cost model and ``constraint_function`` raise
    ``NotImplementedError``.

    Joint expected improvement (an addition): ``acquisition_type='qEI'`` with ``batch_size`` q (1 .. 8; more raises ``ValueError``)
    and the keywords ``num_qei_samples`` (256 base samples) and ``sampler_seed`` scores and optimises the batch AS A WHOLE
    (``AcquisitionQEI``; the evaluator is ``JointBatch``, whatever ``evaluator_type`` of 'sequential', None or 'joint' was given).
    'local_penalization', 'thompson_sampling' and 'random' raise ``InvalidConfigError``: they build a batch point by point.
    ``parallel_anchors=True`` is ignored for it: a batch already fills the wide pass over the inverse factor, and the starts'
    L-BFGS runs go one after the other.  A cost model and ``constraint_function`` raise ``NotImplementedError``.

    Knowledge gradient (an addition): ``acquisition_type='KG'`` with the keywords ``num_kg_points`` (64 discretisation points, at most
    256), ``kg_table_size`` (10000 uniform locations the lowest posterior means are taken from) and ``sampler_seed`` scores the
    expected decrease of the minimum of the posterior mean (``AcquisitionKG``): the acquisition for noisy observations, which reads
    no f_min.  It has gradients, and ``parallel_anchors=True`` works.  Sequential evaluator only: a batch (``batch_size`` > 1 with
    any other evaluator) raises ``InvalidConfigError``; a cost model and ``constraint_function`` raise ``NotImplementedError``.

    Noisy expected improvement (an addition): ``acquisition_type='NEI'`` with the keywords ``num_fantasies`` (16 draws, at most 64),
    ``twin_noise`` (1e-6, the noise of the near-noiseless twin fit) and ``sampler_seed`` scores EI averaged over draws of the
    noiseless function values at the observations, each with its own incumbent (``AcquisitionNEI``): EI for noisy observations,
    where plain EI plugs in the lowest posterior mean as if it were known.  It has gradients, and ``parallel_anchors=True`` works;
    the 'sequential', 'random' and 'thompson_sampling' evaluators take it.  ``exact_feval=True`` (no noise to integrate over) and
    'local_penalization' raise ``InvalidConfigError``; a cost model, ``constraint_function``, and an MCMC, sparse, warped or Gower
    model or a mean function raise ``NotImplementedError``."""

    def __init__(self, f, domain=None, constraints=None, cost_withGradients=None, model_type='GP', X=None, Y=None,
                 initial_design_numdata=5, initial_design_type='random', acquisition_type='EI', normalize_Y=True,
                 exact_feval=False, acquisition_optimizer_type='lbfgs', model_update_interval=1,
                 evaluator_type='sequential', batch_size=1, num_cores=1, verbosity=False, verbosity_model=False,
                 maximize=False, de_duplication=False, model=None, acquisition=None, device=0, parallel_anchors=False,
                 constraint_function=None, C=None, constraint_bounds=0.0, constraint_kinds=None, **kwargs):
        if model_type not in ('GP', 'input_warped_GP') and model is None:
            raise NotImplementedError("model_type %r is outside the accelerated path" % model_type)
        if model_type == 'input_warped_GP' and evaluator_type == 'local_penalization' and batch_size > 1:
            # arguments_manager.py:32-34 (the penaliser's distances live in un-warped space)
            raise InvalidConfigError('local_penalization evaluator can only be used with GP models')
        if evaluator_type not in ('sequential', 'local_penalization', 'thompson_sampling', 'random', 'joint', None):
            raise NotImplementedError("evaluator %r is outside the accelerated path" % evaluator_type)
        joint = isinstance(acquisition, AcquisitionQEI) or (acquisition is None and acquisition_type == 'qEI')
        if joint and evaluator_type not in ('sequential', 'joint', None):
            raise InvalidConfigError("joint expected improvement optimises the batch as a whole: evaluator %r builds one point by "
                                     "point (use 'sequential', None or 'joint')" % evaluator_type)
        if evaluator_type == 'joint' and not joint:
            raise InvalidConfigError("the 'joint' evaluator returns the batch acquisition_type='qEI' optimises")
        if joint and not 1 <= int(batch_size) <= 8:
            raise ValueError("joint expected improvement takes batches of 1 to 8 points, got batch_size=%r" % (batch_size,))
        constrained = constraint_function is not None or C is not None
        if constraint_kinds is not None and not constrained:
            raise ValueError("constraint_kinds without constraint_function or C: there are no constraint columns to name")
        if constraint_kinds is not None and not isinstance(constraint_kinds, str) and \
                any(k not in ('value', 'binary') for k in constraint_kinds):
            raise ValueError("constraint_kinds takes 'value' or 'binary' per constraint column, got %r" % (constraint_kinds,))
        if isinstance(constraint_kinds, str) and constraint_kinds not in ('value', 'binary'):
            raise ValueError("constraint_kinds takes 'value' or 'binary', got %r" % (constraint_kinds,))
        kg = isinstance(acquisition, AcquisitionKG) or (acquisition is None and acquisition_type == 'KG')
        if kg and batch_size > 1 and evaluator_type != 'sequential':
            raise InvalidConfigError("the knowledge gradient suggests one point at a time: evaluator %r builds a batch (batch KG is "
                                     "not implemented; use 'sequential')" % evaluator_type)
        if kg and constrained:
            raise NotImplementedError("the knowledge gradient (KG) takes no black-box constraints: use acquisition_type 'EI' or "
                                      "'MPI' with constraint_function")
        nei = isinstance(acquisition, AcquisitionNEI) or (acquisition is None and acquisition_type == 'NEI')
        if nei and exact_feval:
            raise InvalidConfigError("noisy expected improvement (NEI) integrates over the observation noise: exact_feval=True "
                                     "leaves none (use acquisition_type 'EI')")
        if nei and evaluator_type == 'local_penalization' and batch_size > 1:
            raise InvalidConfigError("noisy expected improvement (NEI) is not penalised: use the 'sequential', 'random' or "
                                     "'thompson_sampling' evaluator")
        if nei and constrained:
            raise NotImplementedError("noisy expected improvement (NEI) takes no black-box constraints: use acquisition_type 'EI' "
                                      "or 'MPI' with constraint_function")
        if joint and constrained:
            raise NotImplementedError("joint expected improvement (qEI) takes no black-box constraints: use acquisition_type 'EI' "
                                      "or 'MPI' with constraint_function")
        if constrained and evaluator_type == 'local_penalization' and batch_size > 1:
            raise InvalidConfigError("local_penalization optimises penalised rows, which take no black-box constraints: use the "
                                     "'sequential', 'random' or 'thompson_sampling' evaluator with constraint_function")
        self.constraint_function = constraint_function
        self.feasibility = None
        self.C = None
        self.evaluator_type = evaluator_type
        self.batch_size = batch_size
        self.f = f
        self.maximize = maximize
        self.space = Design_space(domain, constraints)
        self.normalize_Y = normalize_Y
        self.model_update_interval = model_update_interval
        self.verbosity = verbosity
        self.kwargs = kwargs
        # arguments_manager.py:78-147
        kernel = kwargs.get('kernel', None)
        if isinstance(kernel, str):
            kernel = kernel_from_name(kernel, self.space.dimensionality, ARD=kwargs.get('ARD', False))
        if model is None and model_type == 'input_warped_GP':
            # arguments_manager.py:137-147: only the Kumaraswamy warping exists (None selects it)
            if kwargs.get('input_warping_function_type', "kumar_warping") != "kumar_warping":
                print("Only support kumar_warping for input!")
            model = InputWarpedGPModel(self.space, None, kernel, kwargs.get('noise_var', None), exact_feval,
                                       kwargs.get('model_optimizer_type', 'lbfgs'), kwargs.get('max_iters', 1000),
                                       kwargs.get('optimize_restarts', 5), verbosity_model, kwargs.get('ARD', False),
                                       device=device, parallel_restarts=kwargs.get('parallel_restarts', False))
        self.model = model if model is not None else GPModel(
            kernel=kernel, noise_var=kwargs.get('noise_var', None), exact_feval=exact_feval,
            optimizer=kwargs.get('model_optimizer_type', 'lbfgs'), max_iters=kwargs.get('max_iters', 1000),
            optimize_restarts=kwargs.get('optimize_restarts', 5), verbose=verbosity_model,
            ARD=kwargs.get('ARD', False), Gower=kwargs.get('Gower', False), space=self.space, device=device,
            parallel_restarts=kwargs.get('parallel_restarts', False), incremental=kwargs.get('incremental', False),
            mean_function=kwargs.get('mean_function', None))
        self.acquisition_optimizer = AcquisitionOptimizer(self.space, acquisition_optimizer_type, parallel=parallel_anchors)
        # core/bo.py:31: the cost the acquisitions divide by; 'evaluation_time' fits a GP to the logarithm of the evaluation times
        self.cost = CostModel(cost_withGradients, device=device)
        cost_withGradients = self.cost.cost_withGradients
        # arguments_manager.py:42-75
        jitter = kwargs.get('acquisition_jitter', 0.01)
        weight = kwargs.get('acquisition_weight', 2)
        # arguments_manager.py:50-75 and the acquisitions' own asserts: the integrated acquisitions need the model's
        # hyper-parameter samples, and a model that integrates them out is scored by nothing else
        mcmc_model = bool(getattr(self.model, 'MCMC_sampler', False))
        integrated = {'EI_MCMC': AcquisitionEI_MCMC, 'MPI_MCMC': AcquisitionMPI_MCMC, 'LCB_MCMC': AcquisitionLCB_MCMC}
        if acquisition is None and acquisition_type in integrated and not mcmc_model:
            raise InvalidConfigError("acquisition %r needs a model with MCMC_sampler (GPModel_MCMC)" % acquisition_type)
        if acquisition is None and mcmc_model and acquisition_type not in integrated:
            raise InvalidConfigError("a model with MCMC_sampler is scored by 'EI_MCMC', 'MPI_MCMC' or 'LCB_MCMC', not %r"
                                     % acquisition_type)
        if mcmc_model and batch_size > 1 and evaluator_type not in ('sequential', 'random', None):
            raise NotImplementedError("evaluator %r is not available with a model that samples its hyper-parameters"
                                      % evaluator_type)
        entropy = isinstance(acquisition, AcquisitionEntropySearch) or (acquisition is None and acquisition_type == 'ES')
        if entropy and evaluator_type == 'local_penalization':
            raise InvalidConfigError("local_penalization needs the acquisition's gradients, which entropy search does not have")
        if acquisition is not None:
            self.acquisition = acquisition
        elif acquisition_type == 'ES':
            # the sampler of the representer points and ES.py's keywords (acquisitions/ES.py:12-14)
            self.acquisition = AcquisitionEntropySearch(
                self.model, self.space, AffineInvariantEnsembleSampler(self.space, seed=kwargs.get('sampler_seed', None)),
                self.acquisition_optimizer, cost_withGradients, num_samples=kwargs.get('num_samples', 100),
                num_representer_points=kwargs.get('num_representer_points', 50), burn_in_steps=kwargs.get('burn_in_steps', 50))
        elif acquisition_type == 'MES':
            self.acquisition = AcquisitionMES(self.model, self.space, self.acquisition_optimizer, cost_withGradients,
                                              num_samples=kwargs.get('num_min_samples', 10),
                                              grid_size=kwargs.get('mes_grid_size', 10000), seed=kwargs.get('sampler_seed', None))
        elif acquisition_type == 'TS':
            self.acquisition = AcquisitionTS(self.model, self.space, self.acquisition_optimizer, cost_withGradients,
                                             num_features=kwargs.get('num_features', 1024), seed=kwargs.get('sampler_seed', None))
        elif acquisition_type == 'qEI':
            self.acquisition = AcquisitionQEI(self.model, self.space, self.acquisition_optimizer, batch_size=batch_size,
                                              num_samples=kwargs.get('num_qei_samples', 256), jitter=jitter,
                                              seed=kwargs.get('sampler_seed', None), cost_withGradients=cost_withGradients)
        elif acquisition_type == 'KG':
            self.acquisition = AcquisitionKG(self.model, self.space, self.acquisition_optimizer,
                                             num_points=kwargs.get('num_kg_points', 64),
                                             kg_table_size=kwargs.get('kg_table_size', 10000),
                                             sampler_seed=kwargs.get('sampler_seed', None), cost_withGradients=cost_withGradients)
        elif acquisition_type == 'NEI':
            self.acquisition = AcquisitionNEI(self.model, self.space, self.acquisition_optimizer, jitter=jitter,
                                              num_fantasies=kwargs.get('num_fantasies', 16),
                                              twin_noise=kwargs.get('twin_noise', 1e-6),
                                              sampler_seed=kwargs.get('sampler_seed', None), cost_withGradients=cost_withGradients)
        elif acquisition_type == 'EI_MCMC':
            self.acquisition = AcquisitionEI_MCMC(self.model, self.space, self.acquisition_optimizer, cost_withGradients, jitter)
        elif acquisition_type == 'MPI_MCMC':
            self.acquisition = AcquisitionMPI_MCMC(self.model, self.space, self.acquisition_optimizer, cost_withGradients, jitter)
        elif acquisition_type == 'LCB_MCMC':
            self.acquisition = AcquisitionLCB_MCMC(self.model, self.space, self.acquisition_optimizer, None, weight)
        elif acquisition_type in (None, 'EI'):
            self.acquisition = AcquisitionEI(self.model, self.space, self.acquisition_optimizer, cost_withGradients, jitter)
        elif acquisition_type == 'LCB':
            self.acquisition = AcquisitionLCB(self.model, self.space, self.acquisition_optimizer, None, weight)
        elif acquisition_type == 'MPI':
            self.acquisition = AcquisitionMPI(self.model, self.space, self.acquisition_optimizer, cost_withGradients, jitter)
        else:
            raise NotImplementedError("acquisition %r is outside the accelerated path" % acquisition_type)
        # arguments_manager.py:17-38 (evaluator_creator): local penalisation wraps the acquisition (LP.py)
        if joint:
            self.evaluator = JointBatch(self.acquisition, batch_size)      # the acquisition's rows ARE batches: always its own evaluator
        elif batch_size == 1 or evaluator_type == 'sequential':
            self.evaluator = None                      # Sequential: one optimised point (arguments_manager.py:23-24)
        elif evaluator_type in ('random', None):
            self.evaluator = RandomBatch(self.acquisition, batch_size)
        elif evaluator_type == 'thompson_sampling':
            # Thompson sampling proper draws one posterior path per batch element; every other acquisition keeps the reference's
            # marginal draws for the anchors
            self.evaluator = (ThompsonPathsBatch if isinstance(self.acquisition, AcquisitionTS) else ThompsonBatch)(
                self.acquisition, batch_size)
        elif evaluator_type == 'local_penalization':
            if isinstance(self.acquisition, AcquisitionTS):
                raise NotImplementedError("Thompson sampling spreads a batch by drawing one path per element: use the "
                                          "'thompson_sampling' evaluator, not 'local_penalization'")
            if not isinstance(self.acquisition, AcquisitionLP):
                self.acquisition = AcquisitionLP(self.model, self.space, self.acquisition_optimizer, self.acquisition,
                                                 transform=kwargs.get('acquisition_transformation', 'none'))
            self.evaluator = LocalPenalization(self.acquisition, batch_size)
        else:
            self.evaluator = None
        # initial data
        if X is None:
            X = self.space.samples_uniform(initial_design_numdata)
        self.X = np.asarray(X, dtype=float)
        if Y is None:
            if f is None:
                raise ValueError("f=None requires X and Y")
            Y = self._evaluate(self.X, record_cost=True)
        self.Y = np.asarray(Y, dtype=float).reshape(-1, 1)
        if constrained:
            if C is None:
                C = self._evaluate_constraints(self.X)
            self.C = np.asarray(C, dtype=float).reshape(self.X.shape[0], -1)
            self.feasibility = FeasibilityModel(self.C.shape[1], constraint_bounds, kinds=constraint_kinds, device=device,
                                                exact_feval=exact_feval,
                                                optimizer=kwargs.get('model_optimizer_type', 'lbfgs'),
                                                max_iters=kwargs.get('max_iters', 1000),
                                                optimize_restarts=kwargs.get('optimize_restarts', 5), verbose=verbosity_model,
                                                ARD=kwargs.get('ARD', False))
            scored = self.acquisition.acq if isinstance(self.acquisition, AcquisitionLP) else self.acquisition
            if isinstance(scored, AcquisitionLCB):
                raise ValueError("LCB takes no black-box constraints: use acquisition_type 'EI' or 'MPI' with constraint_function")
            if isinstance(scored, AcquisitionMES):
                raise NotImplementedError("MES takes no black-box constraints: use acquisition_type 'EI' or 'MPI' with "
                                          "constraint_function")
            if not isinstance(scored, (AcquisitionEI, AcquisitionMPI)) or scored._rule is None or \
                    isinstance(scored, (AcquisitionEI_MCMC, AcquisitionMPI_MCMC)):
                raise NotImplementedError("black-box constraints weight EI and MPI over the exact GPModel")
            scored._set_feasibility(self.feasibility)
        self.num_acquisitions = 0
        self.suggested_sample = None
        self.cum_time = 0.0

    def _evaluate(self, X, record_cost=False):
        """The objective at the rows of ``X``.  Under ``cost_withGradients='evaluation_time'`` one row at a time, each call
        timed (core/task/objective.py:64-77); with ``record_cost`` the times then go to the cost model (bo.py:120-122,195-196)."""
        if self.cost.cost_type != 'evaluation_time':
            Y = np.asarray(self.f(X), dtype=float).reshape(-1, 1)
            return -Y if self.maximize else Y
        X = np.atleast_2d(X)
        values, costs = [], []
        for row in X:
            started = _clock()
            values.append(np.asarray(self.f(np.atleast_2d(row)), dtype=float).reshape(-1, 1))
            costs.append(_clock() - started)
        if record_cost:
            self.cost.update_cost_model(X, costs)
        Y = np.vstack(values)
        return -Y if self.maximize else Y

    def _evaluate_constraints(self, X):
        """The constraint values [n, K] at the rows of ``X``."""
        if self.constraint_function is None:
            raise ValueError("constraint values C without a constraint_function cover the initial design only")
        X = np.atleast_2d(X)
        return np.asarray(self.constraint_function(X), dtype=float).reshape(X.shape[0], -1)

    # -- core/bo.py:236-254 ----------------------------------------------------------------
    def _update_model(self, normalization_type='stats'):
        if self.num_acquisitions % self.model_update_interval == 0:
            Y_inmodel = normalize(self.Y, normalization_type) if self.normalize_Y else self.Y
            self.model.updateModel(self.X, Y_inmodel, None, None)
            if self.feasibility is not None:      # the constraint GPs are refitted with the surrogate, on the same rows
                self.feasibility.update(self.X, self.C)

    def _best_observation(self):
        """Row of the reported optimum: the lowest objective; under black-box constraints among the feasible observations, or
        the least violating one while there is none (see the class)."""
        if self.feasibility is None:
            return int(np.argmin(self.Y))
        ok = self.feasibility.feasible(self.C)
        if ok.any():
            rows = np.flatnonzero(ok)
            return int(rows[np.argmin(self.Y[rows, 0])])
        viol = self.feasibility.violation(self.C)
        rows = np.flatnonzero(viol == viol.min())
        return int(rows[np.argmin(self.Y[rows, 0])])

    # -- core/bo.py:216-234 ----------------------------------------------------------------
    def _compute_next_evaluations(self, pending_zipped_X=None, ignored_zipped_X=None):
        if self.evaluator is not None:
            return self.evaluator.compute_batch()
        x, _ = self.acquisition.optimize()
        return x

    def suggest_next_locations(self, context=None, pending_X=None, ignored_X=None):
        """core/bo.py:55-71."""
        if context is not None:
            raise NotImplementedError("context variables are host-side bookkeeping outside the accelerated path")
        self._update_model()
        self.suggested_sample = self._compute_next_evaluations(pending_X, ignored_X)
        return self.suggested_sample

    def run_optimization(self, max_iter=0, max_time=np.inf, eps=1e-8, context=None, verbosity=False, **kw):
        """core/bo.py:73-168 (sequential evaluator)."""
        if self.f is None:
            raise ValueError("Cannot run the optimization loop without the objective function")
        t0 = time.time()
        it = 0
        while (time.time() - t0) < max_time:
            try:
                self._update_model()
            except np.linalg.LinAlgError:
                break                                  # bo.py:134-137
            # bo.py:139-141: the model is refreshed first, then the budget and the distance between the LAST TWO
            # evaluated points decide (the point that triggers the rule has been evaluated and is kept)
            if it >= max_iter or (self.X.shape[0] > 1 and
                                  np.sqrt(np.sum((self.X[-1, :] - self.X[-2, :]) ** 2)) <= eps):
                break
            x = self._compute_next_evaluations()
            y = self._evaluate(x, record_cost=True)
            if self.feasibility is not None:
                self.C = np.vstack((self.C, self._evaluate_constraints(x)))
            self.X = np.vstack((self.X, x))
            self.Y = np.vstack((self.Y, y))
            self.num_acquisitions += 1
            it += 1
            if verbosity or self.verbosity:
                print("num acquisition: %d, time elapsed: %.2fs" % (self.num_acquisitions, time.time() - t0))
        self.cum_time = time.time() - t0
        i = self._best_observation()
        self.x_opt, self.fx_opt = self.X[i], float(self.Y[i, 0])
        return self.x_opt, self.fx_opt
