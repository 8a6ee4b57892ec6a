"""The knowledge gradient's entries off the unit cube: the two relations of tests/_domain_cases.py (its docstring states them)
for the entries of ``_lib.KgEntries``, with that module's own transforms (``scaled``, ``shifted``, ``rounded``), exponents and
offsets, over two existing cases of tests/_kg_truth.py -- b (ARD, N = 300, D = 3, the narrow pass) and f (one lengthscale,
N = 130, D = 2, noise 1e-6, the wide pass).  tests/test_gpu_kg_domains.py runs the device; tests/test_kg_domains_host.py holds
2 Delta to ten times the existing tolerance, as tests/test_domains_host.py does for that module's table.

Results: the points' means, +KG over the table, -KG and its gradient of the leading rows by value.  Existing tolerances: those of
tests/test_gpu_kg.py -- the mean's, the value's first-order allowance per row, the gradient's max(4 x the float64 restatement's
own error, the relative tolerance of the largest entry)."""
import collections
import functools

import numpy as np

import _domain_cases as DC
import _kg_truth as KT

T = KT.T
CASES = ("b", "f")
ROLES = {"X": DC.COORD, "Xa": DC.COORD, "Xs": DC.COORD, "ls": DC.LENGTH}
RESULTS = collections.OrderedDict([("mu", DC.EXACT), ("table", DC.EXACT), ("rows", DC.EXACT), ("gradient", DC.grad(1))])


@functools.lru_cache(maxsize=None)
def problem(cid):
    p = KT.problem(cid)
    return dict(X=p.X, Y=p.Y, ls=p.ls_arg, Xa=p.Xa, Xs=p.Xs)


def lengthscales(cid, p):
    c = KT.CASES[cid]
    ls = np.asarray(p["ls"], dtype=float).reshape(-1)
    return ls if ls.size == c.D else np.full(c.D, ls[0])


def exponent_sets(cid):
    c = KT.CASES[cid]
    return [DC.exponents(c.D)] if c.ard else [DC.exponents(c.D, u) for u in DC.UNIFORM]


def offset(cid):
    return DC.offsets(KT.CASES[cid].D)


def _solve(cid, p, dtype):
    c = KT.CASES[cid]
    q = KT.Problem(c, p["X"], p["Y"], lengthscales(cid, p), p["ls"], p["Xa"], p["Xs"])
    return KT.solve_case(c, q, 0.0, dtype)


def truth(cid, p):
    sv = _solve(cid, p, T)
    c, tr = sv.p.case, sv.truth
    return collections.OrderedDict([("mu", tr.mu), ("table", tr.value), ("rows", -tr.value[:c.Mr]), ("gradient", -tr.grad)])


def tolerance(cid, p):
    c = KT.CASES[cid]
    sv = _solve(cid, p, T)
    with DC._pinned():
        f64 = _solve(cid, {k: np.asarray(v, dtype=float) for k, v in p.items()}, np.float64)
    tol_m, _ = KT.tolerances(c.noise, sv.truth.mean_norm, KT.VARIANCE, c.y_std)
    g = sv.truth.grad
    return dict(mu=tol_m, table=sv.allowance, rows=sv.allowance[:c.Mr],
                gradient=max(4 * DC.maxnorm(f64.truth.grad, g), KT.rel_tol(c.noise) * float(np.max(np.abs(g)))))


def device(h, cid, p):
    c = KT.CASES[cid]
    h.set_data(p["X"], p["Y"])
    h.set_params(KT.FAMILY_ID[c.fam], int(c.ard), KT.VARIANCE, p["ls"], c.noise)
    assert h.fit()[2] == 0.0
    mu = h.kg.set_points(p["Xa"], KT.Y_MEAN, c.y_std)
    h.set_candidates(p["Xs"])
    table = h.kg.acq(c.y_std)[:, 0]
    rows, g = h.kg.rows(p["Xs"][:c.Mr], c.y_std, grad=True)
    return collections.OrderedDict([("mu", mu), ("table", table), ("rows", rows[:, 0]), ("gradient", g)])


@functools.lru_cache(maxsize=None)
def shifted_problem(cid):
    return DC.shifted(problem(cid), ROLES, offset(cid))


@functools.lru_cache(maxsize=None)
def shifted_truth(cid):
    """(truth, existing tolerance, Delta) per result of the shifted problem (tests/_domain_cases.shifted_truth's computation)."""
    p = shifted_problem(cid)
    t = truth(cid, p)
    tol = tolerance(cid, p)
    dl = {n: 0.0 for n in t}
    for how in ("div", "mul"):
        t2 = truth(cid, DC.rounded(p, ROLES, lengthscales(cid, p), how))
        for n in t:
            dl[n] = max(dl[n], DC.maxnorm(t[n], t2[n]))
    return t, tol, dl


def condition(cid):
    """{result: (2 Delta, 10 x the existing tolerance's largest entry)}: the first must not exceed the second."""
    t, tol, dl = shifted_truth(cid)
    return {n: (2 * dl[n], 10 * float(np.max(tol[n]))) for n in t}


def part2_report(cid, dev):
    """Per result: (device error, existing tolerance at its largest, Delta, the largest |device - truth| / (existing + 2 Delta))."""
    t, tol, dl = shifted_truth(cid)
    rep = collections.OrderedDict()
    for n in RESULTS:
        got, ref = np.asarray(dev[n], dtype=T), np.asarray(t[n], dtype=T)
        assert got.shape == ref.shape and np.all(np.isfinite(got)), n
        err = np.abs(got - ref)
        allow = np.asarray(tol[n], dtype=T) + 2 * T(dl[n])
        rep[n] = (float(np.max(err)), float(np.max(tol[n])), dl[n], float(np.max(err / allow)))
    return rep
