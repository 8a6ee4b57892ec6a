"""GPU: the cost surface of cost-aware EI / MPI (csrc/cost.hip, api_cost.hip) and GP_ACQ_PER_COST through every scoring entry.

1. ``gp_cost_rows`` against the long-double truth of tests/_cost_truth.py at the bound derived there (the module's docstring walks
   through csrc/cost.hip operation by operation).  gamma, in the form |logc - truth| <= gamma eps sum_j |alpha_j k_j| |scale|: a
   term's value passes at most COST_CB = 32 fma of its chunk and then at most nchunk = ceil(Nc / 32) additions of the chunks'
   partial sums (both kernels run this one order); the covariance adds 13 + |arg| roundings (exp within 4 ulp, the polynomial, the
   products, the exponent's own rounding); the distance adds |k'(r)| delta r / k with delta r <= |e|_2 + (D / 2 + 1) u r, e_d the
   rounding of the scaled difference -- so gamma = (32 + nchunk + 13 + |arg|) / 2 + the distance's share, evaluated term by term.
   The same per component of dlogc over sum_j |alpha_j g_j df_jd|, with |g'| and two more roundings of the term.
2. The bits of one location do not depend on its company: alone, in tables of 9, 130, 1025 rows, in few-rows calls of 1..8.
3. The flagged scores against the same entry without the flag, divided on the host by exp(truth): the bound is that of logc (a
   relative error of the quotient) plus 8 eps (the device's exp, the host's, the division and the product), for the gradient per
   component (|dneg| bound(logc) + |neg| bound(dlogc_d)) / c + 8 eps (|dneg_d| + |neg dlogc_d|) / c; both plus four spacings of
   the subnormal numbers, where the tail's scores live (a relative bound means nothing below 2.2e-308) -- for the gradient the
   numerator's spacings are divided by c as well.
4. Error codes.  5. The cached logc of a table.  6. The classes.
Measured error-to-bound ratios: profiles/cost_errors.txt (tools/cost_errors.py prints them from these same functions)."""
import ctypes

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd import acquisitions as A
from oracle import cpu_ref as O

import _cost_truth as CT

pytestmark = pytest.mark.gpu

EI, LCB, MPI, F = _lib.GP_ACQ_EI, _lib.GP_ACQ_LCB, _lib.GP_ACQ_MPI, _lib.GP_ACQ_PER_COST
ARG = _lib.GP_ERR_ARG
EPS = np.finfo(float).eps
T = np.longdouble


def _bits(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


@pytest.fixture(scope="module")
def h():
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", 0)
    yield hd
    hd.close()


def set_surface(h, cid):
    """The handle with data of the case's width (the surface has the handle's D columns) and the case's surface."""
    p = CT.problem(cid)
    c = p.case
    if getattr(h, "D", None) != c.D:
        rng = np.random.default_rng(3)
        h.set_data(rng.uniform(0, 1, (8, c.D)), rng.standard_normal((8, 1)))
    h.cost_set(p.Xc, p.alpha, CT.KERNEL_IDS[c.fam], c.ard, p.variance, p.ls_arg, c.shift, c.scale)
    assert h.cost_info() == c.Nc
    return p


def surface_ratios(h, cid):
    """(largest |logc - truth| / bound, largest |dlogc - truth| / bound, logc, dlogc) of a case."""
    p = set_surface(h, cid)
    logc, dlogc = h.cost_rows(p.Xs, grad=True)
    t_logc, t_dlogc, b_logc, b_dlogc, _ = CT.truth(cid)
    r0 = np.max(np.abs(logc.astype(T) - t_logc) / b_logc)
    r1 = np.max(np.abs(dlogc.astype(T) - t_dlogc) / b_dlogc)
    return float(r0), float(r1), logc, dlogc


# ---- 1. the surface against the truth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in CT.TABLE])
def test_surface_against_the_truth(h, cid):
    r0, r1, logc, dlogc = surface_ratios(h, cid)
    print("case %s: logc error / bound %.3f, dlogc error / bound %.3f" % (cid, r0, r1))
    assert np.all(np.isfinite(logc)) and np.all(np.isfinite(dlogc))
    assert r0 <= 1.0 and r1 <= 1.0
    p = CT.problem(cid)
    assert _bits(h.cost_rows(p.Xs)) == _bits(logc)                       # values alone: the same bits
    if p.case.fam == "Exponential":                                       # r = 0 adds exactly 0: the row is finite and within the bound
        assert np.all(np.isfinite(dlogc[list(p.case.same)]))


# ---- 2. the bits of a location do not depend on its company ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid,row", [("f", 3), ("d", 2), ("e", 17), ("i", 5), ("g", 0), ("m", 4), ("j", 0)])
def test_bits_do_not_depend_on_the_company(h, cid, row):
    p = set_surface(h, cid)
    D = p.case.D
    x = p.Xs[row]
    alone = _bits(*h.cost_rows(x[None, :], grad=True))
    assert _bits(h.cost_rows(x[None, :])) == alone[:1]
    rng = np.random.default_rng(11)
    for M in (9, 130, 1025):
        for at in (0, 7, M - 1):
            tab = rng.uniform(0, 1, (M, D))
            tab[at] = x
            logc, dlogc = h.cost_rows(tab, grad=True)
            assert _bits(logc[[at]], dlogc[[at]]) == alone, (M, at)
            assert _bits(h.cost_rows(tab)[[at]]) == alone[:1], (M, at)
    for M in range(1, 9):
        few = rng.uniform(0, 1, (M, D))
        at = M - 1 - M // 3
        few[at] = x
        logc, dlogc = h.cost_rows(few, grad=True)
        assert _bits(logc[[at]], dlogc[[at]]) == alone, (M, at)


# ---- 3. the flagged scores, isolated from the base acquisition's own error ------------------------------------------------------------
N, D, M, MZ, S = 300, 3, 600, 40, 3
FEW_EPS = 8 * EPS
TINY = 4 * np.finfo(float).smallest_subnormal      # far in the tail the scores are subnormal: a quotient there is good to the spacing


class _Scored(object):
    """One context with an exact fit, a sparse fit and an ensemble over the same data, the table in both table slots, and a cost
    surface (Matern-5/2, ARD, 65 points, a normaliser) with its truth at the table's rows."""

    def __init__(self):
        self.X, self.Y, self.Xs = O.synthetic_problem(N, D, M, seed=5)
        rng = np.random.default_rng(21)
        self.Xc, self.alpha = rng.uniform(0, 1, (65, D)), 0.3 * rng.standard_normal(65)
        self.ls = np.array([0.5, 0.8, 0.65])
        self.surf = dict(kernel=_lib.GP_KERNEL_MATERN52, ard=1, variance=1.2, lengthscale=self.ls, shift=-0.4, scale=0.8)
        self.Xs[5], self.Xs[400] = self.Xc[2], self.Xc[40]            # two table rows on points of the surface
        h = self.h = _lib.Handle(0)
        h.set_option("emulate_fp64", 0)
        h.set_data(self.X, self.Y)
        h.set_params(_lib.GP_KERNEL_RBF, 0, 1.1, [0.4], 1e-2)
        h.fit()
        self.fmin = h.fmin()
        h.sparse_set_inducing(rng.uniform(0, 1, (MZ, D)))
        h.sparse_fit()
        self.smin = h.sparse_fmin()
        h.ens_fit(np.linspace(1.0, 1.4, S), np.linspace(0.4, 0.6, S)[:, None], np.linspace(1e-2, 2e-2, S))
        h.set_candidates(self.Xs)
        h.sparse_set_candidates(self.Xs)
        self.set()

    def set(self, alpha=None):
        s = self.surf
        self.h.cost_set(self.Xc, self.alpha if alpha is None else alpha, s["kernel"], s["ard"], s["variance"], s["lengthscale"],
                        s["shift"], s["scale"])

    def truth(self, X, alpha=None):
        s = self.surf
        return CT.surface("Mat52", s["variance"], self.ls, self.Xc, self.alpha if alpha is None else alpha, s["shift"], s["scale"], X)


@pytest.fixture(scope="module")
def sc():
    c = _Scored()
    yield c
    c.h.close()


def _check_quotient(tag, flagged, plain, truth, grad):
    """flagged = plain / exp(truth logc) (and the quotient rule for the gradient) within the bound of the docstring's item 3."""
    logc, dlogc, b_logc, b_dlogc, _ = truth
    c = np.exp(logc)
    neg = np.asarray(plain[0] if grad else plain, dtype=float).reshape(-1).astype(T)
    got = np.asarray(flagged[0] if grad else flagged, dtype=float).reshape(-1).astype(T)
    want = neg / c
    bound = np.abs(want) * (b_logc + FEW_EPS) + TINY
    ratio = float(np.max(np.abs(got - want) / bound))
    worst = [ratio]
    assert np.all(np.abs(got - want) <= bound), (tag, ratio)
    if grad:
        dneg, dgot = plain[1].astype(T), flagged[1].astype(T)
        dwant = (dneg - neg[:, None] * dlogc) / c[:, None]
        dbound = ((np.abs(dneg) * b_logc[:, None] + np.abs(neg)[:, None] * b_dlogc)
                  + FEW_EPS * (np.abs(dneg) + np.abs(neg[:, None] * dlogc))) / c[:, None] + TINY * (1 + 1 / c[:, None])
        dratio = float(np.max(np.abs(dgot - dwant) / dbound))
        worst.append(dratio)
        assert np.all(np.abs(dgot - dwant) <= dbound), (tag, dratio)
    print("%-40s error / bound %s" % (tag, " ".join("%.3f" % w for w in worst)))
    return worst


def _best(v, sense):
    v = np.asarray(v, dtype=float).ravel()
    i = int(np.argmax(v) if sense > 0 else np.argmin(v))
    return i, v[i]


def _topk(v, sense, k):
    v = np.asarray(v, dtype=float).ravel()
    order = np.argsort(v if sense < 0 else -v, kind="stable")[:k]
    return order.astype(np.int64), v[order]


@pytest.mark.parametrize("acq,par", [(EI, 0.01), (MPI, 0.05)])
def test_exact_table_entries(sc, acq, par):
    h = sc.h
    h.set_candidates(sc.Xs)
    truth = sc.truth(sc.Xs)
    plain, plain_g = h.acq(acq, par, sc.fmin), h.acq_grad(acq, par, sc.fmin)
    flagged, flagged_g = h.acq(acq | F, par, sc.fmin), h.acq_grad(acq | F, par, sc.fmin)
    _check_quotient("gp_acq %d" % acq, flagged, plain, truth, False)
    _check_quotient("gp_acq_grad %d" % acq, flagged_g, plain_g, truth, True)
    assert _bits(flagged_g[0]) == _bits(flagged)
    for sense in (-1, +1):
        i, v = h.acq_argbest(acq | F, par, sc.fmin, sense)
        wi, wv = _best(flagged, sense)
        assert (i, np.float64(v).tobytes()) == (wi, np.float64(wv).tobytes())
        idx, val = h.acq_topk(acq | F, par, sc.fmin, sense, 7)
        widx, wval = _topk(flagged, sense, 7)
        assert np.array_equal(idx, widx) and _bits(val) == _bits(wval)
    assert _bits(h.acq(acq, par, sc.fmin)) == _bits(plain)                # without the flag: as before, after flagged calls


@pytest.mark.parametrize("acq,par", [(EI, 0.01), (MPI, 0.05)])
@pytest.mark.parametrize("M1", [1, 5])
def test_exact_rows(sc, acq, par, M1):
    h = sc.h
    x = np.ascontiguousarray(sc.Xs[3:3 + M1])
    truth = sc.truth(x)
    fused0 = h.rows_stats()["fused"]
    _check_quotient("gp_acq_rows %d M=%d" % (acq, M1), h.acq_rows(x, acq | F, par, sc.fmin), h.acq_rows(x, acq, par, sc.fmin), truth, False)
    _check_quotient("gp_acq_rows %d M=%d grad" % (acq, M1), h.acq_rows(x, acq | F, par, sc.fmin, grad=True),
                    h.acq_rows(x, acq, par, sc.fmin, grad=True), truth, True)
    assert h.rows_stats()["fused"] == fused0 + 4                           # the fused passes, the quotient behind them


def test_exact_rows_through_the_table_arithmetic(sc):
    """More than eight locations leave the fused path: gp_set_candidates + the table entries, the quotient included."""
    h = sc.h
    x = np.ascontiguousarray(sc.Xs[100:111])
    _check_quotient("gp_acq_rows M=11 grad", h.acq_rows(x, EI | F, 0.01, sc.fmin, grad=True), h.acq_rows(x, EI, 0.01, sc.fmin, grad=True),
                    sc.truth(x), True)
    h.set_candidates(sc.Xs)


@pytest.mark.parametrize("acq,par", [(EI, 0.01), (MPI, 0.05)])
def test_sparse_entries(sc, acq, par):
    h = sc.h
    truth = sc.truth(sc.Xs)
    plain_g, flagged_g = h.sparse_acq(acq, par, sc.smin, grad=True), h.sparse_acq(acq | F, par, sc.smin, grad=True)
    flagged = h.sparse_acq(acq | F, par, sc.smin)
    _check_quotient("gp_sparse_acq %d" % acq, flagged, h.sparse_acq(acq, par, sc.smin), truth, False)
    _check_quotient("gp_sparse_acq %d grad" % acq, flagged_g, plain_g, truth, True)
    for sense in (-1, +1):
        i, v = h.sparse_acq_argbest(acq | F, par, sc.smin, sense)
        wi, wv = _best(flagged, sense)
        assert (i, np.float64(v).tobytes()) == (wi, np.float64(wv).tobytes())
        idx, val = h.sparse_acq_topk(acq | F, par, sc.smin, sense, 5)
        widx, wval = _topk(flagged, sense, 5)
        assert np.array_equal(idx, widx) and _bits(val) == _bits(wval)
    for M1 in (1, 5, 11):                                                  # fused rows, fused rows, the table arithmetic on scratch
        x = np.ascontiguousarray(sc.Xs[20:20 + M1])
        _check_quotient("gp_sparse_acq_rows %d M=%d grad" % (acq, M1), h.sparse_acq_rows(x, acq | F, par, sc.smin, grad=True),
                        h.sparse_acq_rows(x, acq, par, sc.smin, grad=True), sc.truth(x), True)
        _check_quotient("gp_sparse_acq_rows %d M=%d" % (acq, M1), h.sparse_acq_rows(x, acq | F, par, sc.smin),
                        h.sparse_acq_rows(x, acq, par, sc.smin), sc.truth(x), False)


@pytest.mark.parametrize("acq,par", [(EI, 0.01), (MPI, 0.05)])
def test_ensemble_entries(sc, acq, par):
    h = sc.h
    h.set_candidates(sc.Xs)
    flagged = h.ens_acq(acq | F, par)
    _check_quotient("gp_ens_acq %d" % acq, flagged, h.ens_acq(acq, par), sc.truth(sc.Xs), False)
    for sense in (-1, +1):
        i, v = h.ens_acq_argbest(acq | F, par, sense)
        wi, wv = _best(flagged, sense)
        assert (i, np.float64(v).tobytes()) == (wi, np.float64(wv).tobytes())
    for M1 in (1, 5, 8):
        x = np.ascontiguousarray(sc.Xs[40:40 + M1])
        _check_quotient("gp_ens_acq_rows %d M=%d" % (acq, M1), h.ens_acq_rows(x, acq | F, par), h.ens_acq_rows(x, acq, par), sc.truth(x), False)
        _check_quotient("gp_ens_acq_rows %d M=%d grad" % (acq, M1), h.ens_acq_rows(x, acq | F, par, grad=True),
                        h.ens_acq_rows(x, acq, par, grad=True), sc.truth(x), True)


# ---- 4. error codes -------------------------------------------------------------------------------------------------------------------
def test_error_codes(sc):
    h, lib = sc.h, sc.h.lib
    h.set_candidates(sc.Xs)
    out = np.empty(M)
    dout = np.empty((M, D))
    idx, val = ctypes.c_int64(), ctypes.c_double()
    idx3, val3 = np.empty(3, dtype=np.int64), np.empty(3)
    x = np.ascontiguousarray(sc.Xs[:2])
    Xb, r0, s0 = np.ascontiguousarray(sc.Xs[:2]), np.array([0.1, 0.2]), np.array([0.05, 0.05])

    def calls(t, lp=0):
        """every entry that takes the flag, as (name, return code) under type ``t``"""
        p = _lib.dptr
        if not lp:      # (the entries without a penaliser argument; gp_acq_lp is called by itself below)
            yield "gp_acq", lib.gp_acq(h.h, t, 0.01, sc.fmin, 0.0, 1.0, p(out))
            yield "gp_acq_grad", lib.gp_acq_grad(h.h, t, 0.01, sc.fmin, 0.0, 1.0, p(out), p(dout))
            yield "gp_acq_argbest", lib.gp_acq_argbest(h.h, t, 0.01, sc.fmin, 0.0, 1.0, -1, ctypes.byref(idx), ctypes.byref(val))
            yield "gp_acq_topk", lib.gp_acq_topk(h.h, t, 0.01, sc.fmin, 0.0, 1.0, -1, 3, idx3.ctypes.data_as(_lib.c_int64_p), p(val3))
            yield "gp_sparse_acq_topk", lib.gp_sparse_acq_topk(h.h, t, 0.01, sc.smin, 0.0, 1.0, -1, 3, idx3.ctypes.data_as(_lib.c_int64_p), p(val3))
            yield "gp_ens_acq_argbest", lib.gp_ens_acq_argbest(h.h, t, 0.01, -1, ctypes.byref(idx), ctypes.byref(val))
        yield "gp_acq_rows", lib.gp_acq_rows(h.h, x.ctypes.data, 2, t, 0.01, sc.fmin, 0.0, 1.0, lp, 0, Xb.ctypes.data if lp else None,
                                             2 if lp else 0, r0.ctypes.data if lp else None, s0.ctypes.data if lp else None,
                                             out.ctypes.data, None)
        yield "gp_sparse_acq", lib.gp_sparse_acq(h.h, t, 0.01, sc.smin, 0.0, 1.0, lp, 0, p(Xb) if lp else None, 2 if lp else 0,
                                                 p(r0) if lp else None, p(s0) if lp else None, p(out), None)
        yield "gp_sparse_acq_rows", lib.gp_sparse_acq_rows(h.h, x.ctypes.data, 2, t, 0.01, sc.smin, 0.0, 1.0, lp, 0,
                                                           Xb.ctypes.data if lp else None, 2 if lp else 0, r0.ctypes.data if lp else None,
                                                           s0.ctypes.data if lp else None, out.ctypes.data, None)
        if not lp:
            yield "gp_ens_acq", lib.gp_ens_acq(h.h, t, 0.01, p(out))
            yield "gp_ens_acq_rows", lib.gp_ens_acq_rows(h.h, x.ctypes.data, 2, t, 0.01, out.ctypes.data, None)

    assert all(rc == 0 for _, rc in calls(EI | F)), list(calls(EI | F))
    assert all(rc == ARG for _, rc in calls(LCB | F)), list(calls(LCB | F))             # LCB takes no cost
    assert all(rc == ARG for _, rc in calls(EI | F, lp=1)), list(calls(EI | F, lp=1))   # the penalised acquisition takes no cost
    assert lib.gp_acq_lp(h.h, EI | F, 0.01, sc.fmin, 0.0, 1.0, 0, _lib.dptr(Xb), 2, _lib.dptr(r0), _lib.dptr(s0), _lib.dptr(out)) == ARG
    assert all(rc == 0 for _, rc in calls(EI, lp=1)) and all(rc == 0 for _, rc in calls(LCB))
    assert all(rc == ARG for _, rc in calls(EI | F | 0x200)) and all(rc == ARG for _, rc in calls(3 | F))
    with pytest.raises(ValueError, match="columns"):                                  # a surface of the wrong width
        h.cost_set(np.zeros((4, D + 1)), np.zeros(4), _lib.GP_KERNEL_RBF, 0, 1.0, [1.0])
    assert h.cost_info() == 65
    for bad in (dict(kernel=7), dict(variance=-1.0), dict(lengthscale=[0.5, 0.0, 0.5]), dict(shift=np.inf)):
        kw = dict(sc.surf)
        kw.update(bad)
        with pytest.raises(ValueError):
            h.cost_set(sc.Xc, sc.alpha, kw["kernel"], kw["ard"], kw["variance"], kw["lengthscale"], kw["shift"], kw["scale"])
        assert h.cost_info() == 65
    h.cost_set(None, None, 0, 0, 1.0, None)                                            # the flag without a surface
    assert h.cost_info() == 0
    assert all(rc == ARG for _, rc in calls(EI | F)), list(calls(EI | F))
    assert b"cost surface" in lib.gp_last_error()
    assert all(rc == 0 for _, rc in calls(EI))
    with pytest.raises(RuntimeError):
        h.cost_rows(x)
    sc.set()
    h.set_candidates(sc.Xs)


# ---- 5. the cached logc of a table ----------------------------------------------------------------------------------------------------
def test_table_cache_follows_the_surface_and_the_table(sc):
    h = sc.h
    h.set_candidates(sc.Xs)
    plain = h.acq(EI, 0.01, sc.fmin)
    first = h.acq(EI | F, 0.01, sc.fmin)
    assert _bits(h.acq(EI | F, 0.01, sc.fmin)) == _bits(first)            # served from the cache: the same bits
    alpha2 = sc.alpha[::-1].copy()
    sc.set(alpha2)                                                        # another surface: the next call divides by it
    second = h.acq(EI | F, 0.01, sc.fmin)
    _check_quotient("after gp_cost_set", second, plain, sc.truth(sc.Xs, alpha2), False)
    assert _bits(second) != _bits(first)
    i, v = h.acq_argbest(EI | F, 0.01, sc.fmin, -1)
    wi, wv = _best(second, -1)
    assert (i, np.float64(v).tobytes()) == (wi, np.float64(wv).tobytes())
    table2 = np.ascontiguousarray(sc.Xs[::-1])                            # another table of the same size: the next call scores it
    h.set_candidates(table2)
    _check_quotient("after gp_set_candidates", h.acq(EI | F, 0.01, sc.fmin), h.acq(EI, 0.01, sc.fmin), sc.truth(table2, alpha2), False)
    # one cache, two tables: exact, sparse, exact -- each call finds the logc of its own table
    sp = h.sparse_acq(EI | F, 0.01, sc.smin)
    _check_quotient("sparse after exact", sp, h.sparse_acq(EI, 0.01, sc.smin), sc.truth(sc.Xs, alpha2), False)
    _check_quotient("exact after sparse", h.acq(EI | F, 0.01, sc.fmin), h.acq(EI, 0.01, sc.fmin), sc.truth(table2, alpha2), False)
    h.sparse_set_candidates(table2)
    _check_quotient("after gp_sparse_set_candidates", h.sparse_acq(EI | F, 0.01, sc.smin), h.sparse_acq(EI, 0.01, sc.smin),
                    sc.truth(table2, alpha2), False)
    h.cost_set(None, None, 0, 0, 1.0, None)                               # cleared: flagged calls fail again
    with pytest.raises(ValueError, match="cost surface"):
        h.acq(EI | F, 0.01, sc.fmin)
    sc.set()
    h.set_candidates(sc.Xs)
    h.sparse_set_candidates(sc.Xs)
    assert _bits(h.acq(EI | F, 0.01, sc.fmin)) == _bits(first)


# ---- 6. the classes -------------------------------------------------------------------------------------------------------------------
def _objective(x):
    x = np.atleast_2d(x)
    return (np.sin(5 * x[:, 0]) + (x[:, 1] - 0.4) ** 2)[:, None]


def _costs(x):
    x = np.atleast_2d(x)
    return 0.2 + x[:, 0] + 0.5 * np.sin(3 * x[:, 1]) ** 2


@pytest.fixture(scope="module")
def world():
    """A fitted exact model, a fitted cost model over other points, and a table."""
    rng = np.random.RandomState(4)
    X = rng.uniform(0, 1, (60, 2))
    Y = _objective(X) + 0.05 * rng.standard_normal((60, 1))
    gm = gpo.GPModel(kernel=gpo.kern.RBF(2, 0.9, 0.35), noise_var=0.03, max_iters=0, verbose=False)
    gm.updateModel(X, Y, None, None)
    cm = gpo.CostModel('evaluation_time')
    cm.cost_model.max_iters, cm.cost_model.verbose = 0, False      # (keep the default hyper-parameters: the test is about the route)
    Xc = rng.uniform(0, 1, (25, 2))
    cm.update_cost_model(Xc, _costs(Xc))
    table = rng.uniform(0, 1, (300, 2))
    yield gm, cm, X, Y, table
    gm.model.close()
    cm.cost_model.model.close()


def _route_pair(cls, model, cm, **kw):
    """The acquisition on the device route and its twin on the host rule: the same cost behind a plain function, which the
    predicates refuse."""
    dev = cls(model, cost_withGradients=cm.cost_withGradients, **kw)
    host = cls(model, cost_withGradients=lambda x: cm.cost_withGradients(x), **kw)
    return dev, host


@pytest.mark.parametrize("cls", [gpo.AcquisitionEI, gpo.AcquisitionMPI])
def test_classes_take_the_device_route_and_agree_with_the_host_rule(world, cls):
    gm, cm, X, Y, table = world
    dev, host = _route_pair(cls, gm, cm)
    assert dev._device_ok() and dev._per_cost and dev._acq_id == dev._rule.device_id | F
    assert not host._device_ok() and host._route() is None and not host._per_cost
    for rows in (table[:1], table[:5], table[:64], table):                # few rows (by value), tables
        fd, dd = dev.acquisition_function_withGradients(rows)
        fh, dh = host.acquisition_function_withGradients(rows)
        np.testing.assert_allclose(fd, fh, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(dd, dh, rtol=1e-7, atol=1e-9 * np.max(np.abs(dh)))
        np.testing.assert_allclose(dev.acquisition_function(rows), host.acquisition_function(rows), rtol=1e-9, atol=1e-9)
    assert gm.model._h.cost_info() == 25
    scores = dev.acquisition_function(table)[:, 0]
    i, v = dev.argbest(table, -1)
    assert (i, v) == (int(np.argmin(scores)), scores[int(np.argmin(scores))])
    hi, hv = host.argbest(table, -1)
    assert hi == i and abs(hv - v) <= 1e-9 * max(abs(hv), 1.0)
    idx, val = dev.topk(table, 6, -1)
    order = np.argsort(scores, kind="stable")[:6]
    assert np.array_equal(idx, order) and np.array_equal(val, scores[order])
    hidx, hval = host.topk(table, 6, -1)
    assert np.array_equal(hidx, idx)
    np.testing.assert_allclose(hval, val, rtol=1e-9, atol=1e-9)


def test_lcb_and_lp_never_carry_the_flag(world):
    gm, cm, X, Y, table = world
    lcb = gpo.AcquisitionLCB(gm, cost_withGradients=cm.cost_withGradients)
    assert lcb._device_ok() and not lcb._per_cost and lcb._acq_id == LCB
    space = gpo.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}])
    base = gpo.AcquisitionEI(gm, space, cost_withGradients=cm.cost_withGradients)
    lp = gpo.AcquisitionLP(gm, space, None, base)
    lp.update_batches(table[[3, 77]], 2.2, float(Y.min()))
    assert base._per_cost and lp._lp_route() is None and not lp._lp_device_ok()      # a base with a cost: the host rule
    ref = gpo.AcquisitionLP(gm, space, None, gpo.AcquisitionEI(gm, space, cost_withGradients=lambda x: cm.cost_withGradients(x)))
    ref.update_batches(table[[3, 77]], 2.2, float(Y.min()))
    f, df = lp.acquisition_function_withGradients(table[:40])
    rf, rdf = ref.acquisition_function_withGradients(table[:40])
    np.testing.assert_allclose(f, rf, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(df, rdf, rtol=1e-7, atol=1e-9 * np.max(np.abs(rdf)))


def test_replica_groups_refuse_a_cost(world):
    gm, cm, X, Y, table = world
    dev = gpo.AcquisitionEI(gm, cost_withGradients=cm.cost_withGradients)
    with pytest.raises(NotImplementedError, match="cost"):
        dev.argbest(table, -1, devices=[0])
    with pytest.raises(NotImplementedError, match="cost"):
        dev.topk(table, 4, -1, devices=[0])


def test_sparse_model_takes_the_device_cost(world):
    gm, cm, X, Y, table = world
    sm = gpo.GPModel(kernel=gpo.kern.RBF(2, 0.9, 0.35), max_iters=0, verbose=False, sparse=True, num_inducing=20, device_acquisitions=True)
    sm.updateModel(X, Y, None, None)
    dev, host = _route_pair(gpo.AcquisitionEI, sm, cm)
    assert dev._sparse_device_ok() and dev._per_cost and not host._sparse_device_ok()
    for rows in (table[:4], table[:50]):
        fd, dd = dev.acquisition_function_withGradients(rows)
        fh, dh = host.acquisition_function_withGradients(rows)
        np.testing.assert_allclose(fd, fh, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(dd, dh, rtol=1e-7, atol=1e-9 * np.max(np.abs(dh)))
    scores = dev.acquisition_function(table)[:, 0]
    assert dev.argbest(table, -1)[0] == int(np.argmin(scores))
    sm.model.close()


def test_generation_counter_renews_the_surface(world):
    gm, cm, X, Y, table = world
    dev, host = _route_pair(gpo.AcquisitionEI, gm, cm)
    before = dev.acquisition_function(table[:30])
    key = gm.model._h.cost_key
    assert key == (id(cm), cm.generation)
    extra = np.random.RandomState(9).uniform(0, 1, (5, 2))
    cm.update_cost_model(extra, 3.0 * _costs(extra))
    after = dev.acquisition_function(table[:30])
    assert gm.model._h.cost_key == (id(cm), cm.generation) != key and gm.model._h.cost_info() == 30
    assert not np.array_equal(before, after)
    np.testing.assert_allclose(after, host.acquisition_function(table[:30]), rtol=1e-9, atol=1e-9)


def test_bayesian_optimization_with_fed_costs():
    rng = np.random.RandomState(5)
    X = rng.uniform(0, 1, (20, 2))
    Y = _objective(X)
    domain = [{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}]
    np.random.seed(3)
    bo = gpo.BayesianOptimization(f=None, domain=domain, X=X, Y=Y, cost_withGradients='evaluation_time', max_iters=0,
                                  verbosity_model=False)
    bo.cost.cost_model.max_iters, bo.cost.cost_model.verbose = 50, False
    bo.cost.cost_model.optimize_restarts = 1
    bo.cost.update_cost_model(X, _costs(X))
    x1 = bo.suggest_next_locations()
    assert x1.shape == (1, 2) and np.all((x1 >= 0) & (x1 <= 1))
    assert bo.acquisition._device_ok() and bo.acquisition._per_cost
    h = bo.model.model._h
    assert h.cost_info() == 20 and h.cost_key == (id(bo.cost), 1)
    more = rng.uniform(0, 1, (4, 2))
    bo.cost.update_cost_model(more, _costs(more))
    x2 = bo.suggest_next_locations()
    assert x2.shape == (1, 2) and np.all((x2 >= 0) & (x2 <= 1))
    assert h.cost_info() == 24 and h.cost_key == (id(bo.cost), 2)


def test_mcmc_model_with_the_device_cost():
    rng = np.random.RandomState(2)
    X = rng.uniform(0, 1, (30, 2))
    Y = _objective(X) + 0.05 * rng.standard_normal((30, 1))
    np.random.seed(7)
    mm = gpo.GPModel_MCMC(n_samples=3, n_burnin=5, subsample_interval=2, leapfrog_steps=3)
    domain = [{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}]
    bo = gpo.BayesianOptimization(f=None, domain=domain, X=X, Y=Y, model=mm, acquisition_type='EI_MCMC',
                                  cost_withGradients='evaluation_time')
    bo.cost.cost_model.max_iters, bo.cost.cost_model.verbose = 0, False
    bo.cost.update_cost_model(X, _costs(X))
    x1 = bo.suggest_next_locations()
    assert x1.shape == (1, 2) and np.all((x1 >= 0) & (x1 <= 1))
    acq = bo.acquisition
    assert isinstance(acq, gpo.AcquisitionEI_MCMC) and acq._ens_ok() and acq._per_cost
    h = mm.model._h
    assert h.cost_info() == 30 and h.cost_key == (id(bo.cost), 1)
    host = gpo.AcquisitionEI_MCMC(mm, cost_withGradients=lambda x: bo.cost.cost_withGradients(x))
    assert not host._ens_ok()
    Xs = rng.uniform(0, 1, (11, 2))
    for rows in (Xs[:3], Xs):
        fd, dd = acq.acquisition_function_withGradients(rows)
        fh, dh = host.acquisition_function_withGradients(rows)
        np.testing.assert_allclose(fd, fh, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(dd, dh, rtol=1e-7, atol=1e-9 * np.max(np.abs(dh)))
        np.testing.assert_allclose(acq.acquisition_function(rows), host.acquisition_function(rows), rtol=1e-9, atol=1e-9)
    scores = acq.acquisition_function(Xs)[:, 0]
    assert acq.argbest(Xs, -1)[0] == int(np.argmin(scores))
    more = rng.uniform(0, 1, (3, 2))
    bo.cost.update_cost_model(more, _costs(more))
    bo.suggest_next_locations()
    assert h.cost_info() == 33 and h.cost_key == (id(bo.cost), 2)
