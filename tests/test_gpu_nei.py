"""GPU: noisy expected improvement -- gp_nei_set / _info / _get / _table / _argbest / _topk / _rows (csrc/nei.hip,
csrc/api_nei.hip, csrc/api_rows.hip) against the long-double truth of tests/_nei_truth.py, and the classes on top
(``AcquisitionNEI``, ``BayesianOptimization(acquisition_type='NEI')``).

The fantasies are held to the project's relative tolerance at the model's noise, values to the first-order allowance the truth's
adjoint gives, gradients to four times the error of the same algorithm in plain float64 (floor: the twin's relative tolerance of
max |g|).  Every ratio is printed before it is asserted (tools/nei_errors.py collects them into profiles/nei_errors.txt).
"""
import collections
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib

import _nei_truth as NT

pytestmark = pytest.mark.gpu

T = NT.T
YM = NT.Y_MEAN
CASE_IDS = [c.id for c in NT.TABLE]


def _handle(p, noise, fit=True, Y=None, X=None):
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(p.X if X is None else X, p.Y if Y is None else Y)
    h.set_params(NT.FAMILY_ID[p.case.fam], int(p.case.ard), NT.VARIANCE, p.ls_arg, noise)
    if fit:
        h.fit()
    return h


def _pair(p, S=None):
    """(model, twin) of a case, both fitted, the case's fantasies resident on the twin."""
    c = p.case
    h, h0 = _handle(p, c.noise), _handle(p, c.twin_noise)
    S = c.S if S is None else S
    if S:
        h0.nei.set(h, p.Z[:S], p.E[:S])
    return h, h0


Setup = collections.namedtuple("Setup", "p h h0 sv f64 F fstar table rows grad")


@functools.lru_cache(maxsize=None)
def setup(cid):
    """The two handles of a case with the case's fantasies resident, the truth at the fits' jitters, and the device's answers --
    the fantasies, +NEI over the table, -NEI and its gradient of the table's leading rows by value: computed once, shared,
    read-only.  (Tests that change a handle's state build their own.)"""
    p = NT.problem(cid)
    c = p.case
    h, h0 = _pair(p)
    jitter, jitter0 = h.fit_state()[2], h0.fit_state()[2]
    sv, f64 = NT.truth(cid, jitter, jitter0), NT.float64_restatement(cid, jitter, jitter0)
    F, fstar = h0.nei.get()
    h0.set_candidates(p.Xs)
    table = h0.nei.table(c.par, YM, c.y_std)[:, 0]
    rows, grad = h0.nei.rows(p.Xs[:c.Mr], c.par, YM, c.y_std, grad=True)
    rows = rows[:, 0]
    for a in (F, fstar, table, rows, grad):
        a.setflags(write=False)
    return Setup(p, h, h0, sv, f64, F, fstar, table, rows, grad)


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)


# ---- 1. the fantasies ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_fantasies_against_the_truth(cid):
    s = setup(cid)
    c = s.p.case
    S, d, d0 = s.h0.nei.info()
    assert S == c.S and d == s.sv.d and d0 == s.sv.d0
    err_F = float(np.max(np.abs(np.asarray(s.F, dtype=T) - s.sv.truth.F)))
    err_f = float(np.max(np.abs(np.asarray(s.fstar, dtype=T) - s.sv.truth.fstar)))
    print("nei fantasies[%s]      F err / tol_F = %.3e   fstar err / tol_F = %.3e" % (cid, err_F / s.sv.tol_F, err_f / s.sv.tol_F))
    assert err_F <= s.sv.tol_F and err_f <= s.sv.tol_F
    assert _bits(s.fstar) == _bits(s.F.min(1))                                    # the minima are the device's own columns' minima


# ---- 2. values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_table_values_against_the_truth(cid):
    s = setup(cid)
    assert np.all(np.isfinite(s.table))
    err = np.abs(np.asarray(s.table, dtype=T) - s.sv.truth.value).astype(float)
    ratio = err / s.sv.allowance
    i = int(np.argmax(ratio))
    print("nei table[%s]          worst err / allowance = %.3e   (row %d: err %.3e, NEI %.6e; median NEI %.3e)"
          % (cid, ratio[i], i, err[i], float(s.sv.truth.value[i]), float(np.median(np.asarray(s.sv.truth.value, dtype=float)))))
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_rows_values_against_the_truth(cid):
    s = setup(cid)
    Mr = s.p.case.Mr
    assert np.all(np.isfinite(s.rows)) and np.all(np.isfinite(s.grad))           # the location ON a training input included
    err = np.abs(np.asarray(-s.rows, dtype=T) - s.sv.truth.value[:Mr]).astype(float)
    ratio = err / s.sv.allowance[:Mr]
    print("nei rows[%s]           worst err / allowance = %.3e" % (cid, float(ratio.max())))
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_rows_against_table(cid):
    s = setup(cid)
    c = s.p.case
    diff = float(np.max(np.abs(-s.rows - s.table[:c.Mr])))
    bound = NT.rel_tol(c.twin_noise) * max(1.0, float(np.max(np.abs(s.table[:c.Mr]))))
    print("nei rows against table[%s]   |diff| = %.3e   diff / bound = %.3e" % (cid, diff, diff / bound))
    assert diff <= bound


# ---- 3. gradient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gradient_against_the_float64_restatement(cid):
    s = setup(cid)
    g = s.sv.truth.grad
    dev = float(np.max(np.abs(np.asarray(-s.grad, dtype=T) - g)))
    f64 = float(np.max(np.abs(np.asarray(s.f64.truth.grad, dtype=T) - g)))
    floor = NT.rel_tol(s.p.case.twin_noise) * float(np.max(np.abs(g)))
    bound = max(4 * f64, floor)
    print("nei gradient[%s]    device err %.3e   float64 restatement err %.3e   ratio %.3e   floor %.3e   err / bound = %.3e"
          % (cid, dev, f64, dev / f64 if f64 > 0 else np.inf, floor, dev / bound))
    assert dev <= bound


def test_one_fantasy_is_ei_on_the_fantasy():
    """S = 1: gp_nei_table is gp_acq (EI) of an ordinary handle given (X, F_1) at the twin's noise with fmin = fstar_1."""
    s = setup("a")
    p, c = s.p, s.p.case
    ref = _handle(p, c.twin_noise, Y=np.ascontiguousarray(s.F[0][:, None]))
    ref.set_candidates(p.Xs)
    ei = -ref.acq(_lib.GP_ACQ_EI, c.par, float(s.fstar[0]) * c.y_std + YM, YM, c.y_std)[:, 0]
    err = float(np.max(np.abs(ei - s.table)))
    print("nei S = 1 against gp_acq: NEI %.9e   err / allowance = %.3e" % (float(s.table[0]), err / float(s.sv.allowance[0])))
    assert err <= float(s.sv.allowance[0])


# ---- 4. determinism and independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["c", "d"])
def test_rows_bits_do_not_depend_on_slot_company_or_dout(cid):
    s = setup(cid)
    p, c, h0 = s.p, s.p.case, s.h0
    a = (c.par, YM, c.y_std)
    X = p.Xs[:8]
    v8, g8 = h0.nei.rows(X, *a, grad=True)
    assert _bits(v8, g8) == _bits(s.rows, s.grad)                                # repeated calls
    assert _bits(h0.nei.rows(X, *a)) == _bits(v8)                                # the value with and without dout
    v1, g1 = h0.nei.rows(X[:1], *a, grad=True)                                   # slot 0 alone ...
    v4, g4 = h0.nei.rows(X[:4], *a, grad=True)                                   # ... among 4 ...
    assert _bits(v1, g1) == _bits(v4[:1], g4[:1]) == _bits(v8[:1], g8[:1])       # ... and among 8
    w4, k4 = h0.nei.rows(X[[3, 2, 1, 0]], *a, grad=True)                         # another slot, other company
    assert _bits(w4[3:], k4[3:]) == _bits(v1, g1)
    assert _bits(h0.nei.rows(X[:1], *a)) == _bits(v1)


@pytest.mark.parametrize("cid", ["b", "c"])
def test_leading_fantasies_of_a_larger_draw_have_the_same_bits(cid):
    s = setup(cid)
    p, c = s.p, s.p.case
    h, h0 = _pair(p, S=64)                                                       # the whole draw: the case's S are its leading rows
    F, fstar = h0.nei.get()
    assert F.shape == (64, c.N) and _bits(F[:c.S], fstar[:c.S]) == _bits(s.F, s.fstar)
    h0.nei.set(h, p.Z[:c.S], p.E[:c.S])                                           # the case's own S on ANOTHER pair of handles
    h0.set_candidates(p.Xs)
    assert _bits(h0.nei.table(c.par, YM, c.y_std)[:, 0]) == _bits(s.table)
    assert _bits(*h0.nei.rows(p.Xs[:c.Mr], c.par, YM, c.y_std, grad=True)) == _bits(s.rows, s.grad)
    # more than eight rows by value: the table route (the product's summation order is a function of (M, N), as gp_paths_table
    # documents, so a shorter table agrees to rounding, not bitwise)
    many = h0.nei.rows(p.Xs[:9], c.par, YM, c.y_std)
    h0.set_candidates(p.Xs[:9])
    assert _bits(-many[:, 0]) == _bits(h0.nei.table(c.par, YM, c.y_std)[:, 0])
    assert np.max(np.abs(-many[:, 0] - s.table[:9])) <= NT.rel_tol(c.twin_noise) * max(1.0, float(np.max(np.abs(s.table[:9]))))
    with pytest.raises(ValueError):
        h0.nei.rows(p.Xs[:9], c.par, YM, c.y_std, grad=True)                      # ... which has no gradient: GP_ERR_ARG


# ---- 5. selection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["b", "d"])
def test_argbest_and_topk_against_numpy(cid):
    s = setup(cid)
    p, c = s.p, s.p.case
    a = (c.par, YM, c.y_std)
    h, h0 = _pair(p)
    Xs = np.vstack([p.Xs, p.Xs[:5]])                                             # ties: the first five rows again at the end
    h0.set_candidates(Xs)
    v = h0.nei.table(*a)[:, 0]
    assert _bits(v[-5:]) == _bits(v[:5])
    for sense, pick in ((+1, np.argmax), (-1, np.argmin)):
        i, val = h0.nei.argbest(sense, *a)
        assert i == int(pick(v)) and _bits(val) == _bits(v[i])
        idx, vals = h0.nei.topk(sense, 7, *a)
        order = np.argsort(-v if sense > 0 else v, kind="stable")[:7]
        assert np.array_equal(idx, order) and _bits(vals) == _bits(v[order])
    best = int(np.argmax(s.table))                                               # a planted tie: the best row twice, the copy first
    h0.set_candidates(np.vstack([p.Xs[best], p.Xs]))
    v = h0.nei.table(*a)[:, 0]
    assert _bits(v[0]) == _bits(v[best + 1]) and h0.nei.argbest(+1, *a)[0] == 0


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


def _raw_rows(h, Xs, M, par=0.01, y_mean=0.0, y_std=1.0, out=True, grad=True, null_x=False):
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    o, d = np.full(max(M, 16), SENTINEL), np.full(max(M, 16) * h.D, SENTINEL)
    rc = h.lib.gp_nei_rows(h.h, None if null_x else Xs.ctypes.data, M, par, y_mean, y_std, o.ctypes.data if out else None,
                           d.ctypes.data if grad else None)
    return rc, o, d


def _untouched(res):
    return all(np.all(a == SENTINEL) for a in res[1:])


def _raw_table(h, par=0.01, y_mean=0.0, y_std=1.0):
    o = np.full(max(h.M, 1), SENTINEL)
    return h.lib.gp_nei_table(h.h, par, y_mean, y_std, o.ctypes.data_as(_lib.c_double_p)), o


def _raw_set(h0, h, S, Z, E):
    return (h0 or h).lib.gp_nei_set(h0.h if h0 is not None else None, h.h if h is not None else None, S,
                             None if Z is None else Z.ctypes.data, None if E is None else E.ctypes.data)


def _refused_everywhere(h0, Xs):
    rc, o = _raw_table(h0)
    assert rc == _lib.GP_ERR_STATE and np.all(o == SENTINEL)
    res = _raw_rows(h0, Xs, 4)
    assert res[0] == _lib.GP_ERR_STATE and _untouched(res)
    idx, val = np.zeros(4, dtype=np.int64), np.zeros(4)
    pi, pf = idx.ctypes.data_as(_lib.c_int64_p), val.ctypes.data_as(_lib.c_double_p)
    assert h0.lib.gp_nei_topk(h0.h, 0.01, 0.0, 1.0, 1, 4, pi, pf) == _lib.GP_ERR_STATE
    assert h0.lib.gp_nei_argbest(h0.h, 0.01, 0.0, 1.0, 1, pi, pf) == _lib.GP_ERR_STATE
    assert h0.lib.gp_nei_get(h0.h, None, pf) == _lib.GP_ERR_STATE


def test_fantasies_belong_to_both_fits():
    p = NT.problem("b")
    c = p.case
    Z, E = np.ascontiguousarray(p.Z[:c.S]), np.ascontiguousarray(p.E[:c.S])
    h, h0 = _pair(p, S=0)
    h0.set_candidates(p.Xs)
    assert h0.nei.info()[0] == 0
    _refused_everywhere(h0, p.Xs)                                                 # two fits, no resident fantasies
    Y2 = np.vstack([p.Y, np.zeros((2, 1))])
    for drop in (lambda: h0.fit(),
                 lambda: (h0.set_params(NT.FAMILY_ID[c.fam], int(c.ard), NT.VARIANCE, p.ls_arg, 2 * c.twin_noise), h0.fit()),
                 lambda: (h0.set_data(p.X, p.Y), h0.fit(), h0.set_candidates(p.Xs)),
                 lambda: h0.append(p.Xs[:2], Y2)):                                # whatever drops or grows the TWIN's factor
        h, h0 = _pair(p)
        h0.set_candidates(p.Xs)
        assert h0.nei.info()[0] == c.S and _raw_table(h0)[0] == 0
        drop()
        assert h0.nei.info()[0] == 0
        _refused_everywhere(h0, p.Xs)
    for change in (lambda h: h.fit(),
                   lambda h: (h.set_params(NT.FAMILY_ID[c.fam], int(c.ard), NT.VARIANCE, p.ls_arg, 2 * c.noise), h.fit()),
                   lambda h: h.append(p.Xs[:2], Y2),
                   lambda h: h.close()):                                          # ... and whatever happens to the MODEL's
        h, h0 = _pair(p)
        h0.set_candidates(p.Xs)
        assert _raw_table(h0)[0] == 0
        change(h)
        _refused_everywhere(h0, p.Xs)
        assert h0.lib.gp_nei_info(h0.h, None, None, None) == _lib.GP_ERR_STATE
    h, h0 = _pair(p)
    h0.set_candidates(p.Xs)
    h0.nei.clear()                                                                # S = 0 clears
    assert h0.nei.info() == (0, 0.0, 0.0)
    _refused_everywhere(h0, p.Xs)


def _variant(p, noise, kind):
    """A handle over the case's data at ``noise`` that gp_nei_set must refuse for one reason, and the code it must give."""
    c = p.case
    fam, ard = NT.FAMILY_ID[c.fam], int(c.ard)
    if kind == "unfitted":
        return _handle(p, noise, fit=False), _lib.GP_ERR_STATE
    if kind == "two outputs":
        return _handle(p, noise, Y=np.hstack([p.Y, -p.Y])), _lib.GP_ERR_STATE
    if kind == "another N":
        return _handle(p, noise, X=p.X[:-1], Y=p.Y[:-1]), _lib.GP_ERR_ARG
    if kind == "another D":
        h = _lib.Handle(0)
        h.set_option("emulate_fp64", 0)
        h.set_data(np.ascontiguousarray(p.X[:, :-1]), p.Y)
        h.set_params(fam, ard, NT.VARIANCE, p.ls_arg[:-1] if c.ard else p.ls_arg, noise)
        h.fit()
        return h, _lib.GP_ERR_ARG
    h = _handle(p, noise, fit=False)
    if kind == "Gower kernel":
        h.set_gower([0] * c.D, [1.0] * c.D)
    elif kind == "output warp":
        h.set_output_warp([[0.5, 1.0, 0.0]], 1.0)
    elif kind == "mean function":
        h.mean_set(np.full((c.D, 1), 0.1), [0.2])
    if kind == "Laplace fit":
        h.laplace_fit(np.where(p.Y[:, 0] > 0, 1.0, -1.0))
        return h, _lib.GP_ERR_STATE
    h.fit()
    if kind == "sparse fit":                                                      # beside the exact fit, which stays
        h.sparse_set_inducing(p.X[:20])
        h.sparse_fit()
    elif kind == "ensemble":
        h.ens_fit([NT.VARIANCE, NT.VARIANCE], np.vstack([p.ls_arg, 1.1 * p.ls_arg]), [noise, noise])
        assert h.ens_info() == 2
    return h, _lib.GP_ERR_STATE


VARIANTS = ("unfitted", "two outputs", "another N", "another D", "Gower kernel", "output warp", "mean function", "Laplace fit", "sparse fit",
            "ensemble")


def test_set_refusals_leave_the_state_untouched():
    p = NT.problem("c")                                                           # (RBF: the Gower option takes it)
    c = p.case
    Z, E = np.ascontiguousarray(p.Z[:c.S]), np.ascontiguousarray(p.E[:c.S])
    h, h0 = _pair(p)
    h0.set_candidates(p.Xs)
    before = h0.nei.table(c.par, YM, c.y_std)
    fam, ard = NT.FAMILY_ID[c.fam], int(c.ard)

    def unchanged():
        return h0.nei.info()[0] == c.S and _bits(h0.nei.table(c.par, YM, c.y_std)) == _bits(before)

    # every state the entry refuses, on either handle: as the MODEL against the resident twin, whose fantasies and table bits
    # must stay, and as the TWIN against the good model, which must be left without fantasies
    for kind in VARIANTS:
        m, code = _variant(p, c.noise, kind)
        rc = _raw_set(h0, m, c.S, Z, E)
        print("nei refusal[%s as the model]: return code %d" % (kind, rc))
        assert rc == code and unchanged()
        m.close()
        t, code = _variant(p, c.twin_noise, kind)
        rc = _raw_set(t, h, c.S, Z, E)
        print("nei refusal[%s as the twin]: return code %d" % (kind, rc))
        assert rc == code and t.lib.gp_nei_info(t.h, None, None, None) == 0 and t.nei.info()[0] == 0
        assert t.lib.gp_nei_get(t.h, None, None) == _lib.GP_ERR_STATE
        t.close()
    moved = p.X.copy()
    moved[5, 1] = np.nextafter(moved[5, 1], 2.0)
    assert _raw_set(h0, _handle(p, c.noise, X=moved), c.S, Z, E) == _lib.GP_ERR_ARG and unchanged()      # another X, by one ulp
    for kw in (dict(kernel=(fam + 1) % 4), dict(variance=np.nextafter(NT.VARIANCE, 2.0)), dict(ls=p.ls_arg * (1 + 2 ** -40)),
               dict(ard=0, ls=p.ls_arg[:1])):                                     # kernel id, variance, lengthscales, ARD flag
        m = _handle(p, c.noise, fit=False)
        m.set_params(kw.get("kernel", fam), kw.get("ard", ard), kw.get("variance", NT.VARIANCE), kw.get("ls", p.ls_arg), c.noise)
        m.fit()
        assert _raw_set(h0, m, c.S, Z, E) == _lib.GP_ERR_ARG and unchanged()
    assert _raw_set(h0, _handle(p, c.twin_noise), c.S, Z, E) == _lib.GP_ERR_ARG   # d <= d0
    assert _raw_set(h, h0, c.S, Z, E) == _lib.GP_ERR_ARG                          # ... and the roles swapped
    big = np.zeros((65, c.N))
    nan = Z.copy()
    nan[1, 3] = np.nan
    for rc in (_raw_set(h0, h, 65, big, big), _raw_set(h0, h, -1, Z, E), _raw_set(h0, h, c.S, nan, E), _raw_set(h0, h, c.S, Z, nan),
               _raw_set(h0, h, c.S, None, E), _raw_set(h0, None, c.S, Z, E), _raw_set(None, h, c.S, Z, E), _raw_set(h0, h0, c.S, Z, E)):
        assert rc == _lib.GP_ERR_ARG
    assert unchanged() and h.nei.info()[0] == 0


def test_refused_arguments_leave_results_untouched():
    p = NT.problem("b")
    c = p.case
    h, h0 = _pair(p)
    h0.set_candidates(p.Xs)
    before = h0.nei.table(c.par, YM, c.y_std)
    rows_before = h0.nei.rows(p.Xs[:4], c.par, YM, c.y_std, grad=True)
    for kw in (dict(y_std=0.0), dict(y_std=-1.0), dict(y_std=np.inf), dict(y_std=np.nan), dict(y_mean=np.inf), dict(par=np.nan)):
        rc, o = _raw_table(h0, **kw)
        assert rc == _lib.GP_ERR_ARG and np.all(o == SENTINEL)
        res = _raw_rows(h0, p.Xs, 4, **kw)
        assert res[0] == _lib.GP_ERR_ARG and _untouched(res)
    bad = p.Xs[:4].copy()
    bad[2, 1] = np.inf
    for res in (_raw_rows(h0, bad, 4), _raw_rows(h0, p.Xs, 0), _raw_rows(h0, p.Xs, 4, null_x=True), _raw_rows(h0, p.Xs, 4, out=False),
                _raw_rows(h0, p.Xs, 9)):                                          # (nine rows with a gradient: the table has none)
        assert res[0] == _lib.GP_ERR_ARG and _untouched(res)
    i64, f64 = np.zeros(4, dtype=np.int64), np.zeros(4)
    pi, pf = i64.ctypes.data_as(_lib.c_int64_p), f64.ctypes.data_as(_lib.c_double_p)
    lib = h0.lib
    assert lib.gp_nei_argbest(h0.h, 0.01, 0.0, 1.0, 0, pi, pf) == _lib.GP_ERR_ARG
    assert lib.gp_nei_topk(h0.h, 0.01, 0.0, 1.0, 1, 0, pi, pf) == _lib.GP_ERR_ARG
    assert lib.gp_nei_table(h0.h, 0.01, 0.0, 1.0, None) == _lib.GP_ERR_ARG
    assert _bits(h0.nei.table(c.par, YM, c.y_std)) == _bits(before)
    assert _bits(*h0.nei.rows(p.Xs[:4], c.par, YM, c.y_std, grad=True)) == _bits(*rows_before)


def test_route_counters_and_passes():
    """What the issue lists, counted where it happens (gp_nei_stats): the twin's inverse factor is built once for all the calls
    that follow a fit, a value pass is 3 launches of which 1 reads it, a gradient pass 6 launches of which 2 read it."""
    p = NT.problem("c")
    c = p.case
    a = (c.par, YM, c.y_std)
    h, h0 = _pair(p)
    st, ps = h0.rows_stats(), h0.rows_pass_stats()
    assert h0.nei.stats() == dict(linv_builds=0, launches=0, reads=0)            # gp_nei_set builds no inverse factor
    h0.nei.rows(p.Xs[:1], *a)                                                     # layout 1, a value call
    assert h0.nei.stats() == dict(linv_builds=1, launches=3, reads=1)
    h0.nei.rows(p.Xs[:4], *a, grad=True)                                          # layout 4, a gradient call
    assert h0.nei.stats() == dict(linv_builds=1, launches=6, reads=2)
    h0.nei.rows(p.Xs[:8], *a, grad=True)                                          # layout 8: ONE wide pass
    assert h0.nei.stats() == dict(linv_builds=1, launches=6, reads=2)
    h0.nei.rows(p.Xs[:8], *a)
    assert h0.nei.stats() == dict(linv_builds=1, launches=3, reads=1)
    st1, ps1 = h0.rows_stats(), h0.rows_pass_stats()
    assert st1["fused"] == st["fused"] + 4 and st1["fallback"] == st["fallback"]
    assert ps1["narrow"] == ps["narrow"] + 2 and ps1["wide"] == ps["wide"] + 2
    h0.profile(True)                                                              # the profiled pass: one phase per pass, named by its kind
    h0.nei.rows(p.Xs[:4], *a, grad=True)
    assert [q["name"] for q in h0.phases()] == ["rows_nei_grad"]
    h0.profile(False)
    h0.nei.rows(p.Xs[:9], *a)                                                     # beyond the fused shapes: the table route
    assert h0.rows_stats()["fallback"] == st["fallback"] + 1
    assert h0.nei.stats() == dict(linv_builds=1, launches=0, reads=0)
    h0.nei.set(h, p.Z[:c.S], p.E[:c.S])                                           # new fantasies, the same factor: nothing is rebuilt
    h0.nei.rows(p.Xs[:1], *a, grad=True)
    assert h0.nei.stats() == dict(linv_builds=1, launches=6, reads=2)
    h0.fit()                                                                      # a new factor: one more build, at the next rows call
    h0.nei.set(h, p.Z[:c.S], p.E[:c.S])
    assert h0.nei.stats()["linv_builds"] == 1
    h0.nei.rows(p.Xs[:1], *a)
    h0.nei.rows(p.Xs[:1], *a, grad=True)
    assert h0.nei.stats() == dict(linv_builds=2, launches=6, reads=2)
    assert h.rows_stats() == dict(fused=0, fallback=0) and h.nei.stats()["linv_builds"] == 0      # the model's handle answered none of them


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------
def _f2(X):
    X = np.atleast_2d(X)
    return (np.sin(3 * X[:, 0]) + (X[:, 1] - 0.4) ** 2)[:, None]


DOMAIN2 = [{"name": "x%d" % i, "type": "continuous", "domain": (0.0, 1.0)} for i in range(2)]


def _data():
    """A noisy 2-D sample with one outlying low observation in a region where the function is high: the noisy posterior does not
    believe it, EI's plug-in incumbent barely moves, NEI's fantasies of that point stay near the posterior mean."""
    rng = np.random.default_rng(11)
    X0 = rng.uniform(0, 1, (40, 2))
    Y0 = _f2(X0) + 0.1 * rng.standard_normal((40, 1))
    Y0[int(np.argmax(_f2(X0)[:, 0])), 0] -= 1.5
    return X0, Y0


def _bo(kind, parallel=False, **kw):
    X0, Y0 = _data()
    return gpo.BayesianOptimization(_f2, DOMAIN2, X=X0, Y=Y0, acquisition_type=kind, exact_feval=False, sampler_seed=0,
                                    optimize_restarts=1, verbosity_model=False, parallel_anchors=parallel, **kw)


def _suggest(kind, parallel=False, **kw):
    bo = _bo(kind, parallel, **kw)
    np.random.seed(5)                                                             # the optimiser's uniform samples
    return bo, bo.suggest_next_locations()


def test_end_to_end_suggests_a_point():
    bo, x = _suggest("NEI")
    acq = bo.acquisition
    assert isinstance(acq, gpo.AcquisitionNEI) and bo.evaluator is None
    assert x.shape == (1, 2) and np.all(x >= 0.0) and np.all(x <= 1.0)
    assert acq.twin.nei.info()[0] == 16 and acq.refreshes == 1
    F, fstar = acq.fantasies()
    assert F.shape == (16, 40) and np.array_equal(fstar, F.min(1))
    _, x_again = _suggest("NEI")
    assert np.array_equal(x_again, x)                                             # repeatable under the seed
    _, x_par = _suggest("NEI", parallel=True)
    assert x_par.shape == (1, 2) and np.all(x_par >= 0.0) and np.all(x_par <= 1.0)
    # EI on the same data from the same anchors ends elsewhere, and not by rounding: each acquisition scores its OWN suggestion
    # strictly better than the other's (the values are the negated acquisitions: lower is better), so the two surfaces have
    # different optima
    bo_ei, x_ei = _suggest("EI")
    nei_own, nei_other = float(acq.acquisition_function(x)[0, 0]), float(acq.acquisition_function(x_ei)[0, 0])
    ei_own, ei_other = (float(bo_ei.acquisition.acquisition_function(x_ei)[0, 0]), float(bo_ei.acquisition.acquisition_function(x)[0, 0]))
    print("nei end to end: NEI suggests %s, EI %s (distance %.3e); -NEI there %.9e and %.9e; -EI there %.9e and %.9e"
          % (x[0], x_ei[0], float(np.linalg.norm(x - x_ei)), nei_own, nei_other, ei_other, ei_own))
    assert nei_own < nei_other and ei_own < ei_other


def test_end_to_end_three_iterations():
    X0, Y0 = _data()
    rng = np.random.default_rng(3)

    def noisy(X):
        return _f2(X) + 0.1 * rng.standard_normal((np.atleast_2d(X).shape[0], 1))

    bo = gpo.BayesianOptimization(noisy, DOMAIN2, X=X0[:30], Y=Y0[:30], acquisition_type="NEI", exact_feval=False, sampler_seed=0,
                                  num_fantasies=8, optimize_restarts=1, verbosity_model=False)
    np.random.seed(5)
    bo.run_optimization(max_iter=3)
    assert bo.X.shape == (33, 2) and np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)
    acq = bo.acquisition
    assert acq.draws.Z.shape[1] >= 32 and acq.refreshes >= 3                     # the draws grew by columns, the twin followed every fit
