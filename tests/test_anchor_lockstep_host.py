"""CPU: the acquisition optimiser's anchors in lockstep (bayesian_optimization.AcquisitionOptimizer(parallel=True),
_lbfgs_from_anchors) and the bounded lockstep driver under it (parameterization.lbfgsb_lockstep(bounds=, maxfun=)) over NumPy
stand-ins whose rows do not notice their company: every anchor follows its serial run bit for bit."""
import ctypes
import re
import os

import numpy as np
from scipy import optimize as sopt

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import bayesian_optimization as bo
from gaussian_process_optimization_amd.parameterization import lbfgsb_lockstep, SCIPY_DEFAULT

CENTRE = np.array([0.2, 1.3, -0.4])      # the bowl's minimum lies outside the box in two coordinates: bounds become active
BOX = [(0.0, 1.0), (0.0, 1.0), (0.0, 1.0)]


def _row(x):
    """One row's value and gradient, from that row alone (plain Python floats in a fixed order)."""
    f, g = 0.0, []
    for d in range(3):
        u = float(x[d]) - float(CENTRE[d])
        f += u * u + 0.3 * np.sin(5.0 * float(x[d]))
        g.append(2.0 * u + 1.5 * np.cos(5.0 * float(x[d])))
    return f, np.array(g)


def _f(X):
    return np.array([[_row(x)[0]] for x in np.atleast_2d(X)])


def _f_df(X):
    rows = [_row(x) for x in np.atleast_2d(X)]
    return np.array([[r[0]] for r in rows]), np.stack([r[1] for r in rows])


def _fbatch(xs):
    f, g = _f_df(xs)
    return f.ravel(), g


def _space():
    return gpo.Design_space([{'name': 'x%d' % d, 'type': 'continuous', 'domain': BOX[d]} for d in range(3)])


def test_lockstep_with_bounds_equals_serial_bitwise():
    rng = np.random.default_rng(4)
    x0s = [rng.uniform(0, 1, 3) for _ in range(4)] + [np.array([0.0, 1.0, 0.5])]       # the last start lies ON two bounds
    got = lbfgsb_lockstep(_fbatch, x0s, max_iters=40, bounds=BOX)
    active = 0
    for x0, (x, fv, d) in zip(x0s, got):
        ref = sopt.fmin_l_bfgs_b(lambda z: (_row(z)[0], _row(z)[1]), x0, bounds=BOX, maxiter=40, maxfun=40)
        assert np.array_equal(x, ref[0]) and fv == ref[1]
        assert d["nit"] == ref[2]["nit"] and d["funcalls"] == ref[2]["funcalls"]
        active += int(np.any(x == 0.0) or np.any(x == 1.0))
    assert active == len(x0s)           # every run ended on the box's boundary


def _rosen(z):
    return float(sopt.rosen(z)), sopt.rosen_der(z)


def test_maxfun_default_and_scipy_default():
    """maxfun = None stays maxfun = max_iters (what every call before had); SCIPY_DEFAULT leaves the limit to scipy, as a serial
    call that passes maxiter alone: the run then ends on its iteration limit, not on its evaluations."""
    x0s = [np.array([-1.2, 1.0, -0.5, 0.8]), np.array([2.0, -1.0, 1.5, 0.3])]
    fb = lambda xs: (np.array([_rosen(x)[0] for x in xs]), np.stack([_rosen(x)[1] for x in xs]))
    as_before = lbfgsb_lockstep(fb, x0s, max_iters=20)
    free = lbfgsb_lockstep(fb, x0s, max_iters=20, maxfun=SCIPY_DEFAULT)
    six = lbfgsb_lockstep(fb, x0s, max_iters=20, maxfun=6)
    for x0, a, b, c in zip(x0s, as_before, free, six):
        ra = sopt.fmin_l_bfgs_b(_rosen, x0, maxiter=20, maxfun=20)
        rb = sopt.fmin_l_bfgs_b(_rosen, x0, maxiter=20)
        rc = sopt.fmin_l_bfgs_b(_rosen, x0, maxiter=20, maxfun=6)
        for got, ref in ((a, ra), (b, rb), (c, rc)):
            assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and got[2]["funcalls"] == ref[2]["funcalls"]
        # (scipy stops after the iteration in which the evaluations pass maxfun)
        assert b[2]["nit"] == 20 > a[2]["nit"] > c[2]["nit"] and b[2]["funcalls"] > a[2]["funcalls"] > c[2]["funcalls"]


def _serial_and_lockstep(num_anchor, seed):
    space = _space()
    out = []
    for parallel in (False, True):
        opt = bo.AcquisitionOptimizer(space, num_samples=60, num_anchor=num_anchor, parallel=parallel)
        np.random.seed(seed)
        out.append(opt.optimize(f=_f, f_df=_f_df))
    return out


def test_anchors_in_lockstep_return_the_serial_winner():
    for num_anchor in (5, 11):              # one group, and two (8 + 3)
        (xs, fs), (xp, fp) = _serial_and_lockstep(num_anchor, seed=num_anchor)
        assert xs.shape == (1, 3) and np.array_equal(xs, xp) and fs == fp


def test_each_round_is_one_call_of_at_most_eight_rows():
    rows = []

    def f_df(X):
        rows.append(np.atleast_2d(X).shape[0])
        return _f_df(X)

    space = _space()
    np.random.seed(2)
    bo.AcquisitionOptimizer(space, num_samples=60, num_anchor=11, parallel=True).optimize(f=_f, f_df=f_df)
    assert rows[0] == 8 and max(rows) == 8 and 3 in rows
    per_anchor = []
    np.random.seed(2)
    X = space.samples_uniform(60)
    for a in X[np.argsort(_f(X).flatten())[:11]]:
        n0 = len(rows)
        bo._lbfgs_from_anchor(space, a, _f, f_df)
        per_anchor.append(len(rows) - n0)
        assert set(rows[n0:]) == {1}
    n_lock = len(rows) - sum(per_anchor)
    assert n_lock == max(per_anchor[:8]) + max(per_anchor[8:])      # a group takes as many rounds as its longest run


def test_abnormal_line_search_falls_back_to_the_anchor():
    """Gradients that contradict the values around one start: its line search terminates abnormally and the anchor itself is
    kept, as in the serial code; the other anchors are not disturbed."""
    def f_df(X):
        f, g = _f_df(X)
        for j, x in enumerate(np.atleast_2d(X)):
            if x[0] > 0.8:
                g[j] = -g[j] - 1.0
        return f, g

    space = _space()
    anchors = np.array([[0.3, 0.4, 0.5], [0.9, 0.5, 0.5], [0.6, 0.9, 0.1]])
    got = bo._lbfgs_from_anchors(space, anchors, f_df)
    for a, x in zip(anchors, got):
        assert np.array_equal(x, bo._lbfgs_from_anchor(space, a, _f, f_df))
    bad = sopt.fmin_l_bfgs_b(lambda z: tuple(q.ravel() if q.size > 1 else float(q.ravel()[0]) for q in f_df(z)), anchors[1],
                             bounds=BOX, maxiter=1000)
    assert bad[2]["task"] in (b'ABNORMAL_TERMINATION_IN_LNSRCH', 'ABNORMAL_TERMINATION_IN_LNSRCH') or "ABNORMAL" in str(bad[2]["task"])
    assert np.array_equal(got[1], anchors[1:2]) and not np.array_equal(got[0], anchors[0:1])


def test_parallel_without_gradients_or_lbfgs_runs_the_serial_code(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the lockstep routine must not run")

    monkeypatch.setattr(bo, "_lbfgs_from_anchors", boom)
    space = _space()
    res = []
    for kw, parallel in ((dict(f=_f), True), (dict(f=_f), False)):
        np.random.seed(9)
        res.append(bo.AcquisitionOptimizer(space, num_samples=40, num_anchor=3, maxiter=15, parallel=parallel).optimize(**kw))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    np.random.seed(9)
    other = bo.AcquisitionOptimizer(space, optimizer='sgd', num_samples=40, num_anchor=3, maxiter=15, parallel=True)
    assert not other.lockstep(_f_df)
    x, fx = other.optimize(f=_f, f_df=_f_df)
    assert np.array_equal(x, res[1][0])
    assert bo.BayesianOptimization(f=None, domain=[{'name': 'x', 'type': 'continuous', 'domain': (0, 1)}], X=np.zeros((2, 1)),
                                   Y=np.zeros((2, 1))).acquisition_optimizer.parallel is False


def test_rows_pass_stats_is_bound_as_the_header_declares_it():
    from gaussian_process_optimization_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gphip.h")).read()
    m = re.search(r"int\s+gp_rows_pass_stats\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["gp_t *gp", "int64_t *narrow", "int64_t *wide"]
    spec = [s for s in _lib.SIGNATURES if s[0] == "gp_rows_pass_stats"]
    lib = _lib.load_library()
    fn = lib.gp_rows_pass_stats
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 3
    assert fn.argtypes[0] is ctypes.c_void_p and fn.argtypes[1] is fn.argtypes[2] is ctypes.POINTER(ctypes.c_int64)
    assert len(spec) == 1
    assert hasattr(_lib.Handle, "rows_pass_stats")
