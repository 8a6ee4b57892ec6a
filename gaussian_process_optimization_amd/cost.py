"""The cost of evaluating the objective: ``CostModel`` (GPyOpt/GPyOpt/core/task/cost.py).

``cost_withGradients`` is what the acquisitions divide by: a function of the locations ``x`` [M, D] returning
``(cost [M, 1], d cost / dx [M, D])``.

* ``None``: constant cost, ``constant_cost_withGradients``.
* a callable: kept as given.
* ``'evaluation_time'``: a second GP (``cost_model``, an exact ``GPModel`` with its default Matern-5/2 kernel, on ``device``) is
  fitted to the LOGARITHM of the evaluation times handed to ``update_cost_model``; the cost is ``exp`` of its posterior mean.

EI and MPI over our exact, sparse or MCMC models score this last kind on the device: the routes of ``acquisitions.py`` upload
a snapshot of the cost GP's posterior mean to the scored model's handle (``gp_cost_set``) and ask for the quotient with
``GP_ACQ_PER_COST``; ``generation`` tells them when the snapshot is stale.

Two deliberate departures from the reference:

* before the first ``update_cost_model`` the cost is the constant cost (the reference would call ``predict`` on a cost model
  that does not exist yet);
* ``BayesianOptimization`` records the evaluation times of the initial design when it evaluates it, so that the first step
  already divides by a fitted cost (the reference's ``methods/bayesian_optimization.py`` throws those times away, and its first
  step under ``'evaluation_time'`` fails).
"""
import numpy as np

from .gpmodel import GPModel


def constant_cost_withGradients(x):
    """Unit cost and zero cost gradient (core/task/cost.py:76)."""
    rows = x.shape[0]
    return np.ones((rows, 1)), np.zeros(x.shape)


class CostModel(object):
    """cost.py:8-72.  ``cost_type`` names the kind as the reference does; ``num_updates`` counts the calls of
    ``update_cost_model`` that reached the cost GP, ``generation`` moves with each of them."""

    def __init__(self, cost_withGradients=None, device=0):
        self.cost_type = cost_withGradients
        self.generation = 0
        if cost_withGradients is None:
            self.cost_withGradients = constant_cost_withGradients
            self.cost_type = 'Constant cost'
        elif isinstance(cost_withGradients, str) and cost_withGradients == 'evaluation_time':
            self.cost_model = GPModel(device=device)
            self.cost_withGradients = self._cost_gp_withGradients
            self.num_updates = 0
        else:
            self.cost_withGradients = cost_withGradients
            self.cost_type = 'Used defined cost'

    def _fitted(self):
        return getattr(self, "num_updates", 0) > 0

    def _cost_gp(self, x):
        """The predicted evaluation time at the rows of ``x`` [M, 1]."""
        return self._cost_gp_withGradients(x)[0]

    def _cost_gp_withGradients(self, x):
        """``(exp(m), exp(m) dm/dx)`` with ``m`` the cost GP's posterior mean; the constant cost before the first update."""
        x = np.atleast_2d(x)
        if not self._fitted():
            return constant_cost_withGradients(x)
        m, _, dmdx, _ = self.cost_model.predict_withGradients(x)
        price = np.exp(m)
        return price, price * dmdx

    def update_cost_model(self, x, cost_x):
        """New locations ``x`` [n, D] and their evaluation times ``cost_x`` [n]: their logarithms go under what the cost GP
        holds, and the cost GP is refitted.  A no-op for the other kinds of cost."""
        if self.cost_type != 'evaluation_time':
            return
        x = np.atleast_2d(np.asarray(x, dtype=float))
        log_cost = np.log(np.atleast_2d(np.asarray(cost_x, dtype=float)).T)
        if self.num_updates == 0:
            X_all, costs_all = x, log_cost
        else:
            X_all = np.vstack((self.cost_model.model.X, x))
            costs_all = np.vstack((self.cost_model.model.Y, log_cost))
        self.num_updates += 1
        self.cost_model.updateModel(X_all, costs_all, None, None)
        self.generation += 1
