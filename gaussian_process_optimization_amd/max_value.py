"""Samples of the VALUE of the global minimum, y*, for max-value entropy search (Wang & Jegelka, ICML 2017, section 3.1: the
Gumbel approximation, mirrored for a minimum).

Over a table of M locations with independent marginals N(m_i, s_i^2) the minimum's survival function is

    log S(y) = log Pr[y* > y] ~ sum_i log Phi((m_i - y) / s_i),

a Gumbel law for the minimum,  Pr[y* <= y] = 1 - exp(-exp((y - a) / b)),  is put through its three quartiles

    b = (y75 - y25) / (log log 4 - log log(4/3)),   a = y50 - b log log 2,

and the samples are  y*_k = a + b log(-log U_k),  U_k uniform on (0, 1), clipped at the incumbent ``model.get_fmin()``: the
minimum cannot lie above the best posterior mean at an observation.

Where the work runs.  For our exact ``GPModel`` (one output) the table -- ``grid_size`` uniform draws of the space plus the model's
X -- becomes the handle's resident candidates and stays on the device: ``gp_mes_bracket`` (8 sigma) gives a bracket that holds
every quantile, and rounds of ``gp_mes_logsurv`` narrow it, 64 trial values a call, over the LATENT posterior (y* is the minimum
of f).  Any other model does the same sums on the host, with the same rounds, from ``model.predict(table, with_noise=False)`` --
the latent posterior as well -- where ``predict`` takes that argument (``GPModel``'s contract), else from ``model.predict(table)``,
which for a foreign ``BOModel`` is whatever that model predicts, the likelihood noise usually included: its y* is then the minimum
of a noisy observation over the table, a more spread law.  The host sums run over blocks of rows (64 x 65536 doubles at a time).

The rounds.  Every quantile keeps a bracket [lo, hi] with S(lo) >= 1 - q > S(hi).  A round cuts each distinct bracket into 65
equal parts by 64 trial values (quantiles that still share a bracket share the call) and keeps the part where log S crosses
log(1 - q); the rounds end when every bracket is at most 1e-9 of the first one -- five rounds, 65^5 > 1e9.  A quantile is the
midpoint of its last bracket.
"""
import inspect

import numpy as np
from scipy.special import log_ndtr

QUANTILES = (0.25, 0.5, 0.75)
_LOGLOG = {0.25: np.log(np.log(4.0 / 3.0)), 0.5: np.log(np.log(2.0)), 0.75: np.log(np.log(4.0))}
TRIALS = 64          # trial values per call (GP_MES_MAX_G)
NSIG = 8.0           # the first bracket: [min(m - 8 s), min(m + 8 s)]
REL_WIDTH = 1e-9     # a quantile's bracket is narrowed to this share of the first one
_MAX_ROUNDS = 12
_HOST_ROWS = 65536   # rows per block of the host sums


def gumbel_fit(y25, y50, y75):
    """(a, b) of the Gumbel law of the minimum through the three quartiles."""
    b = (y75 - y25) / (_LOGLOG[0.75] - _LOGLOG[0.25])
    return y50 - b * _LOGLOG[0.5], b


def narrow(logsurv, lo, hi, quantiles=QUANTILES, trials=TRIALS, rel_width=REL_WIDTH):
    """Brackets {q: (lo_q, hi_q)} of the y with 1 - S(y) = q from the first bracket [lo, hi], ``logsurv(y [G]) -> log S [G]``
    being called with at most ``trials`` values at a time (see the module's docstring for the rounds)."""
    width0 = hi - lo
    brackets = {q: (lo, hi) for q in quantiles}
    targets = {q: np.log1p(-q) for q in quantiles}
    frac = np.arange(1, trials + 1) / (trials + 1.0)
    for _ in range(_MAX_ROUNDS):
        wide = [q for q in quantiles if brackets[q][1] - brackets[q][0] > rel_width * width0]
        if not wide:
            break
        for b in sorted({brackets[q] for q in wide}):
            y = b[0] + (b[1] - b[0]) * frac
            ls = np.asarray(logsurv(y), dtype=float).reshape(-1)
            edges = np.concatenate(([b[0]], y, [b[1]]))
            for q in wide:
                if brackets[q] != b:
                    continue
                below = ls < targets[q]      # log S falls with y: the first trial value below 1 - q ends the part that holds the quantile
                j = int(np.argmax(below)) if below.any() else trials
                brackets[q] = (float(edges[j]), float(edges[j + 1]))
    return brackets


class MinValueSampler(object):
    """Draws ``num_samples`` values of the global minimum under ``model``'s posterior (see the module's docstring).

    ``table()`` builds the locations, ``brackets()`` narrows the three quartiles over them, ``sample()`` fits the Gumbel law,
    draws from ``numpy.random.RandomState(seed)`` and clips at ``model.get_fmin()``.  After ``sample()``: ``last_brackets``
    {q: (lo, hi)}, ``last_quantiles`` {q: y_q}, ``last_fit`` (a, b), ``last_first`` (the first bracket), ``last_on_device``, ``last_latent``."""

    def __init__(self, model, space, num_samples=10, grid_size=10000, seed=None, sampler='gumbel', num_features=1024):
        if sampler not in ('gumbel', 'paths'):
            raise ValueError("sampler must be 'gumbel' or 'paths', got %r" % (sampler,))
        self.sampler = sampler
        self.num_features = int(num_features)
        if not 1 <= int(num_samples) <= 64:
            raise ValueError("num_samples must be between 1 and 64 (GP_MES_MAX_K), got %r" % (num_samples,))
        if int(grid_size) < 1:
            raise ValueError("grid_size must be at least 1, got %r" % (grid_size,))
        self.model = model
        self.space = space
        self.num_samples = int(num_samples)
        self.grid_size = int(grid_size)
        self.seed = seed
        self.last_brackets = self.last_quantiles = self.last_fit = self.last_first = None
        self.last_on_device = False
        self.last_latent = True         # the last sums ran over the latent posterior (the device's always do)

    # ---- where the sums run --------------------------------------------------------------------------------------------------
    def _device_gp(self):
        """The exact GP whose handle takes the table, or None (the host sums)."""
        from .gpmodel import GPModel
        m = self.model
        if type(m) is not GPModel or getattr(m, "sparse", False) or m.model is None:
            return None
        gp = m.model
        if gp.output_dim != 1 or not hasattr(gp, "_h") or not hasattr(gp._h, "mes_logsurv"):
            return None
        return gp

    def table(self):
        """``grid_size`` uniform draws of the space, then the model's inputs."""
        grid = np.atleast_2d(np.asarray(self.space.samples_uniform(self.grid_size), dtype=float))
        X = getattr(getattr(self.model, "model", None), "X", None)
        return grid if X is None else np.vstack([grid, np.atleast_2d(np.asarray(X, dtype=float))])

    def brackets(self, table=None):
        """{q: (lo, hi)} for the three quartiles over ``table`` (default: ``table()``)."""
        table = self.table() if table is None else np.atleast_2d(np.asarray(table, dtype=float))
        gp = self._device_gp()
        self.last_on_device = gp is not None
        if gp is not None:
            from .acquisitions import _normaliser
            gp._stage(table)                       # the table becomes the resident candidates; nothing table-sized comes back
            shift, scale = _normaliser(gp)
            h = gp._h
            lo, hi = h.mes_bracket(NSIG, include_noise=False, y_mean=shift, y_std=scale)
            self.last_first, self.last_latent = (lo, hi), True
            return narrow(lambda y: h.mes_logsurv(y, include_noise=False, y_mean=shift, y_std=scale), lo, hi)
        mu, sd = self._host_posterior(table)
        mu, sd = np.ravel(np.asarray(mu, dtype=float)), np.maximum(np.ravel(np.asarray(sd, dtype=float)), 1e-5)
        lo, hi = float(np.min(mu - NSIG * sd)), float(np.min(mu + NSIG * sd))
        self.last_first = (lo, hi)

        def logsurv(y):
            y = np.asarray(y, dtype=float).reshape(-1, 1)
            total = np.zeros(y.shape[0])
            for i in range(0, mu.size, _HOST_ROWS):      # blocks of rows in order: no [G, M] array is ever formed
                total += log_ndtr((mu[None, i:i + _HOST_ROWS] - y) / sd[None, i:i + _HOST_ROWS]).sum(axis=1)
            return total
        return narrow(logsurv, lo, hi)

    def _host_posterior(self, table):
        """(mean, sd) over the table for the host sums: the latent posterior where ``predict`` takes ``with_noise``."""
        predict = self.model.predict
        try:
            latent = "with_noise" in inspect.signature(predict).parameters
        except (TypeError, ValueError):
            latent = False
        self.last_latent = latent
        return predict(table, with_noise=False) if latent else predict(table)

    def sample(self, table=None):
        """``num_samples`` values of y*, all at most ``model.get_fmin()``."""
        if self.sampler == 'paths':
            return self._sample_paths(table)
        br = self.brackets(table)
        quant = {q: 0.5 * (br[q][0] + br[q][1]) for q in QUANTILES}
        a, b = gumbel_fit(quant[0.25], quant[0.5], quant[0.75])
        u = np.random.RandomState(self.seed).uniform(size=self.num_samples)
        fmin = float(np.min(self.model.get_fmin()))
        self.last_brackets, self.last_quantiles, self.last_fit = br, quant, (a, b)
        return np.minimum(a + b * np.log(-np.log(u)), fmin)

    def _sample_paths(self, table=None):
        """The sampler the MES paper itself uses: ``num_samples`` posterior paths (posterior_paths.py), each minimised over the
        table on the device (gp_paths_argbest: 2 K numbers come back), clipped at the incumbent as the Gumbel draws are."""
        gp = self._device_gp()
        if gp is None:
            raise NotImplementedError("sampler='paths' draws posterior paths of our exact GPModel: a foreign, sparse or warped "
                                      "model keeps sampler='gumbel'")
        from .posterior_paths import PosteriorPaths, draw
        table = self.table() if table is None else np.atleast_2d(np.asarray(table, dtype=float))
        gp._ensure_fit()
        paths = PosteriorPaths(gp, draws=draw(gp.kern, gp.num_data, gp.input_dim, self.num_samples, self.num_features, self.seed))
        self.last_on_device, self.last_latent = True, True
        self.last_argmin, values = paths.argmin(table)
        return np.minimum(values, float(np.min(self.model.get_fmin())))
