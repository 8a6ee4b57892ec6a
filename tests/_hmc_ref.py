"""Hybrid Monte Carlo restated from the algorithm (Duane et al. 1987; Neal 2011, "MCMC using Hamiltonian dynamics", sec. 5.3.2-3),
independently of gaussian_process_optimization_amd/mcmc.py: plain functions over (U, grad U) of a position vector, unit or
general mass matrix, and the order of random draws of the sampler it is compared with -- per sample ONE
``np.random.multivariate_normal(0, M)`` for the momentum, then ONE ``np.random.rand()`` for the Metropolis test.

Also here: the pure-Python models of tests/test_mcmc_host.py (a quadratic potential behind the interface HMC asks of a model).
"""
import numpy as np


def leapfrog(q, p, grad_U, eps, steps, Minv):
    """``steps`` leapfrog steps of size ``eps``: p -= eps/2 grad U(q); q += eps Minv p; p -= eps/2 grad U(q)."""
    q, p = np.array(q, dtype=float), np.array(p, dtype=float)
    for _ in range(steps):
        p = p + (-eps / 2. * grad_U(q))
        q = q + eps * np.dot(Minv, p)
        p = p + (-eps / 2. * grad_U(q))
    return q, p


def hamiltonian(q, p, U, M, Minv):
    """U(q) + the negative log density of p ~ N(0, M), normaliser included."""
    return U(q) + p.size * np.log(2 * np.pi) / 2. + np.log(np.linalg.det(M)) / 2. + float(np.dot(p, np.dot(Minv, p[:, None]))[0]) / 2.


def chain(q0, U, grad_U, num_samples, eps, steps, M=None, record=None):
    """The chain the sampler under test must reproduce bit for bit.  Row i holds the state BEFORE trajectory i and is replaced by
    the proposal when it is accepted -- so a rejected proposal repeats the state the trajectory started from.  ``record`` maps a
    position to what is stored (default: the position itself).  Returns (rows, accept decisions)."""
    q = np.array(q0, dtype=float)
    M = np.eye(q.size) if M is None else M
    Minv = np.linalg.inv(M)
    record = (lambda x: x) if record is None else record
    rows, accepts = np.empty((num_samples, q.size)), []
    for i in range(num_samples):
        p = np.random.multivariate_normal(np.zeros(q.size), M)
        H_old = hamiltonian(q, p, U, M, Minv)
        rows[i] = record(q)
        q_new, p_new = leapfrog(q, p, grad_U, eps, steps, Minv)
        H_new = hamiltonian(q_new, p_new, U, M, Minv)
        k = 1. if H_old > H_new else np.exp(H_old - H_new)
        ok = bool(np.random.rand() < k)
        accepts.append(ok)
        if ok:
            q = q_new
            rows[i] = record(q)
    return rows, accepts


class Quadratic(object):
    """U(x) = 0.5 sum x_i^2 / var_i behind the model interface of the sampler: the target is N(0, diag(var))."""

    def __init__(self, x0, var):
        self.var = np.asarray(var, dtype=float)
        self._x = np.array(x0, dtype=float)
        self.gradient_calls = 0

    @property
    def optimizer_array(self):
        return self._x

    @optimizer_array.setter
    def optimizer_array(self, x):
        self._x = np.array(x, dtype=float)

    @property
    def unfixed_param_array(self):
        return self._x.copy()

    def U(self, x):
        return float(0.5 * np.sum(np.square(x) / self.var))

    def grad_U(self, x):
        return np.asarray(x, dtype=float) / self.var

    def objective_function(self):
        return self.U(self._x)

    def objective_function_gradients(self):
        self.gradient_calls += 1
        return self.grad_U(self._x)
