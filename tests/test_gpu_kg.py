"""GPU: the knowledge gradient -- gp_kg_set_points / _info / _acq / _acq_argbest / _acq_topk / _rows (csrc/kg.hip,
csrc/api_kg.hip) against the long-double truth of tests/_kg_truth.py, and the classes on top (``AcquisitionKG``,
``BayesianOptimization(acquisition_type='KG')``).

Values are held to the first-order allowance the truth's adjoint gives for the posterior's tolerances (tests/test_gpu_rows.py's);
gradients to four times the error of the same algorithm in plain float64 (floor: the posterior's relative tolerance of max |g|).
Every ratio is printed before it is asserted (tools/kg_errors.py collects them into profiles/kg_errors.txt).
"""
import collections
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib

import _kg_truth as KT

pytestmark = pytest.mark.gpu

T = KT.T
YM = KT.Y_MEAN
CASE_IDS = [c.id for c in KT.TABLE]


def _handle(p, fit=True, Y=None):
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(p.X, p.Y if Y is None else Y)
    h.set_params(KT.FAMILY_ID[p.case.fam], int(p.case.ard), KT.VARIANCE, p.ls_arg, p.case.noise)
    if fit:
        h.fit()
    return h


Setup = collections.namedtuple("Setup", "p h sv f64 mu table rows grad")


@functools.lru_cache(maxsize=None)
def setup(cid):
    """The handle of a case with the case's points resident, the truth at the fit's jitter, and the device's answers -- the
    points' means, +KG over the table, -KG and its gradient of the table's leading rows by value: computed once, shared,
    read-only.  (Tests that change a handle's state build their own.)"""
    p = KT.problem(cid)
    c = p.case
    h = _handle(p)
    jitter = h.fit_state()[2]
    mu = h.kg.set_points(p.Xa, YM, c.y_std)
    sv, f64 = KT.truth(cid, jitter), KT.float64_restatement(cid, jitter)
    h.set_candidates(p.Xs)
    table = h.kg.acq(c.y_std)[:, 0]
    rows, grad = h.kg.rows(p.Xs[:c.Mr], c.y_std, grad=True)
    rows = rows[:, 0]
    for a in (mu, table, rows, grad):
        a.setflags(write=False)
    return Setup(p, h, sv, f64, mu, table, rows, grad)


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)


# ---- 1. the points' means -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_points_mean_against_the_truth(cid):
    s = setup(cid)
    c = s.p.case
    assert s.h.kg.info() == c.A
    tol_m, _ = KT.tolerances(c.noise, s.sv.truth.mean_norm, KT.VARIANCE, c.y_std)
    err = float(np.max(np.abs(np.asarray(s.mu, dtype=T) - s.sv.truth.mu)))
    print("kg points' mean[%s]   err / tolerance = %.3e" % (cid, err / tol_m))
    assert err <= tol_m


# ---- 2. values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_table_values_against_the_truth(cid):
    s = setup(cid)
    err = np.abs(np.asarray(s.table, dtype=T) - s.sv.truth.value).astype(float)
    ratio = err / s.sv.allowance
    i = int(np.argmax(ratio))
    print("kg table[%s]          worst err / allowance = %.3e   (row %d: err %.3e, KG %.6e; median KG %.3e)"
          % (cid, ratio[i], i, err[i], float(s.sv.truth.value[i]), float(np.median(np.asarray(s.sv.truth.value, dtype=float)))))
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_rows_values_against_the_truth(cid):
    s = setup(cid)
    Mr = s.p.case.Mr
    err = np.abs(np.asarray(-s.rows, dtype=T) - s.sv.truth.value[:Mr]).astype(float)
    ratio = err / s.sv.allowance[:Mr]
    print("kg rows[%s]           worst err / allowance = %.3e" % (cid, float(ratio.max())))
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_rows_against_table(cid):
    s = setup(cid)
    Mr = s.p.case.Mr
    diff = float(np.max(np.abs(-s.rows - s.table[:Mr])))
    scale = max(1.0, float(np.max(np.abs(s.table[:Mr]))))
    print("kg rows against table[%s]   |diff| = %.3e" % (cid, diff))
    assert diff <= 1e-9 * scale


# ---- 3. gradient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gradient_against_the_float64_restatement(cid):
    s = setup(cid)
    g = s.sv.truth.grad
    dev = float(np.max(np.abs(np.asarray(-s.grad, dtype=T) - g)))
    f64 = float(np.max(np.abs(np.asarray(s.f64.truth.grad, dtype=T) - g)))
    floor = KT.rel_tol(s.p.case.noise) * float(np.max(np.abs(g)))
    bound = max(4 * f64, floor)
    print("kg gradient[%s]    device err %.3e   float64 restatement err %.3e   ratio %.3e   floor %.3e   err / bound = %.3e"
          % (cid, dev, f64, dev / f64 if f64 > 0 else np.inf, floor, dev / bound))
    assert dev <= bound


def test_one_point_is_the_two_line_closed_form():
    s = setup("a")
    tr = s.sv.truth
    closed = KT.two_line_closed_form(tr.atil[0], tr.b[0])
    err_t, err_r = abs(float(T(s.table[0]) - closed)), abs(float(T(-s.rows[0]) - closed))
    print("kg A = 1 closed form: KG %.9e   table err / allowance = %.3e   rows err / allowance = %.3e"
          % (float(closed), err_t / s.sv.allowance[0], err_r / s.sv.allowance[0]))
    assert err_t <= s.sv.allowance[0] and err_r <= s.sv.allowance[0]


# ---- 4. determinism and independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["c", "f"])
def test_rows_bits_do_not_depend_on_slot_company_or_dout(cid):
    s = setup(cid)
    p, c, h = s.p, s.p.case, s.h
    X = p.Xs[:8]
    v8, g8 = h.kg.rows(X, c.y_std, grad=True)
    assert _bits(v8, g8) == _bits(s.rows, s.grad)                                # repeated calls
    assert _bits(h.kg.rows(X, c.y_std)) == _bits(v8)                             # the value with and without dout
    v1, g1 = h.kg.rows(X[:1], c.y_std, grad=True)                                # slot 0 alone ...
    v4, g4 = h.kg.rows(X[:4], c.y_std, grad=True)                                # ... among 4 ...
    assert _bits(v1, g1) == _bits(v4[:1], g4[:1]) == _bits(v8[:1], g8[:1])       # ... and among 8
    w4, k4 = h.kg.rows(X[[3, 2, 1, 0]], c.y_std, grad=True)                      # another slot, other company
    assert _bits(w4[3:], k4[3:]) == _bits(v1, g1)
    assert _bits(h.kg.rows(X[:1], c.y_std)) == _bits(v1)


@pytest.mark.parametrize("cid", ["b", "d"])
def test_table_value_does_not_depend_on_length_or_row(cid):
    s = setup(cid)
    p, c = s.p, s.p.case
    h = _handle(p)
    h.kg.set_points(p.Xa, YM, c.y_std)
    h.set_candidates(p.Xs)
    assert _bits(h.kg.acq(c.y_std)) == _bits(s.table)                            # another handle, the same bits
    sub = np.ascontiguousarray(p.Xs[[7, 3, 0]])
    h.set_candidates(sub)
    assert _bits(h.kg.acq(c.y_std)[:, 0]) == _bits(s.table[[7, 3, 0]])
    h.set_candidates(p.Xs[:9])                                                   # more than eight rows by value: the table route
    many = h.kg.rows(p.Xs[:9], c.y_std)
    assert _bits(-many[:, 0]) == _bits(s.table[:9])
    with pytest.raises(ValueError):
        h.kg.rows(p.Xs[:9], c.y_std, grad=True)                                  # ... which has no gradient: GP_ERR_ARG


# ---- 5. selection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["d", "e"])
def test_argbest_and_topk_against_numpy(cid):
    s = setup(cid)
    p, c = s.p, s.p.case
    h = _handle(p)
    h.kg.set_points(p.Xa, YM, c.y_std)
    Xs = np.vstack([p.Xs, p.Xs[:5]])                                             # ties: the first five rows again at the end
    h.set_candidates(Xs)
    v = h.kg.acq(c.y_std)[:, 0]
    assert _bits(v[-5:]) == _bits(v[:5])
    for sense, pick in ((+1, np.argmax), (-1, np.argmin)):
        i, val = h.kg.acq_argbest(sense, c.y_std)
        assert i == int(pick(v)) and _bits(val) == _bits(v[i])
        idx, vals = h.kg.acq_topk(sense, 7, c.y_std)
        order = np.argsort(-v if sense > 0 else v, kind="stable")[:7]
        assert np.array_equal(idx, order) and _bits(vals) == _bits(v[order])
    # the winner of a tie is the lower index
    h.set_candidates(np.vstack([p.Xs[:3], p.Xs[:3]]))
    v = h.kg.acq(c.y_std)[:, 0]
    assert h.kg.acq_argbest(+1, c.y_std)[0] == int(np.argmax(v)) < 3


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


def _raw_rows(h, Xs, M, y_std=1.0, out=True, grad=True, null_x=False):
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    o, d = np.full(max(M, 16), SENTINEL), np.full(max(M, 16) * h.D, SENTINEL)
    rc = h.lib.gp_kg_rows(h.h, None if null_x else Xs.ctypes.data, M, y_std, o.ctypes.data if out else None,
                          d.ctypes.data if grad else None)
    return rc, o, d


def _untouched(res):
    return all(np.all(a == SENTINEL) for a in res[1:])


def _raw_acq(h, y_std=1.0):
    o = np.full(max(h.M, 1), SENTINEL)
    return h.lib.gp_kg_acq(h.h, y_std, o.ctypes.data_as(_lib.c_double_p)), o


def test_points_belong_to_the_fit():
    s = setup("b")
    p, c = s.p, s.p.case
    h = _handle(p)
    h.set_candidates(p.Xs)
    rc, o = _raw_acq(h)
    assert rc == _lib.GP_ERR_STATE and np.all(o == SENTINEL)                      # a fit, no resident points
    res = _raw_rows(h, p.Xs, 4)
    assert res[0] == _lib.GP_ERR_STATE and _untouched(res)
    for drop in (lambda: h.fit(),
                 lambda: (h.set_params(KT.FAMILY_ID[c.fam], int(c.ard), KT.VARIANCE, p.ls_arg, 2e-2), h.fit()),
                 lambda: h.append(p.Xs[:2], np.vstack([p.Y, np.zeros((2, 1))]))):
        h.kg.set_points(p.Xa, YM, c.y_std)
        assert h.kg.info() == c.A and _raw_acq(h)[0] == 0
        drop()
        assert h.kg.info() == 0
        assert _raw_acq(h)[0] == _lib.GP_ERR_STATE
        res = _raw_rows(h, p.Xs, 4)
        assert res[0] == _lib.GP_ERR_STATE and _untouched(res)
        idx, val = np.zeros(4, dtype=np.int64), np.zeros(4)
        assert h.lib.gp_kg_acq_topk(h.h, 1.0, 1, 4, idx.ctypes.data_as(_lib.c_int64_p), val.ctypes.data_as(_lib.c_double_p)) \
            == _lib.GP_ERR_STATE
    fresh = _lib.Handle(0)
    fresh.D = c.D
    assert fresh.lib.gp_kg_set_points(fresh.h, p.Xa.ctypes.data_as(_lib.c_double_p), c.A, 0.0, 1.0, None) == _lib.GP_ERR_STATE
    unfit = _handle(p, fit=False)
    assert unfit.lib.gp_kg_set_points(unfit.h, p.Xa.ctypes.data_as(_lib.c_double_p), c.A, 0.0, 1.0, None) == _lib.GP_ERR_STATE


def test_refused_states():
    s = setup("b")
    p, c = s.p, s.p.case
    h = _handle(p)
    Xa = p.Xa.ctypes.data_as(_lib.c_double_p)
    for switch_on, switch_off in ((lambda: h.set_output_warp([[0.5, 1.0, 0.0]], 1.0), lambda: h.set_output_warp(None)),
                                  (lambda: h.mean_set(np.full((c.D, 1), 0.1), [0.2]), lambda: h.mean_set(None, None)),
                                  (lambda: h.set_gower([0] * c.D, [1.0] * c.D), lambda: h.set_gower())):
        switch_on()
        h.fit()
        assert h.lib.gp_kg_set_points(h.h, Xa, c.A, 0.0, 1.0, None) == _lib.GP_ERR_STATE
        switch_off()
        h.fit()
        assert h.lib.gp_kg_set_points(h.h, Xa, c.A, 0.0, 1.0, None) == 0
    hp = _handle(p, Y=np.hstack([p.Y, -p.Y]))                                     # two outputs
    assert hp.lib.gp_kg_set_points(hp.h, Xa, c.A, 0.0, 1.0, None) == _lib.GP_ERR_STATE


def test_refused_arguments_leave_results_and_points_untouched():
    s = setup("b")
    p, c = s.p, s.p.case
    h = _handle(p)
    h.kg.set_points(p.Xa, YM, c.y_std)
    h.set_candidates(p.Xs)
    before = h.kg.acq(c.y_std)
    rows_before = h.kg.rows(p.Xs[:4], c.y_std, grad=True)
    lib, Xa = h.lib, p.Xa.ctypes.data_as(_lib.c_double_p)
    big = np.zeros((257, c.D))
    nan = p.Xa.copy()
    nan[1, 0] = np.nan
    for rc in (lib.gp_kg_set_points(h.h, Xa, 0, 0.0, 1.0, None), lib.gp_kg_set_points(h.h, big.ctypes.data_as(_lib.c_double_p), 257, 0.0, 1.0, None),
               lib.gp_kg_set_points(h.h, None, c.A, 0.0, 1.0, None), lib.gp_kg_set_points(None, Xa, c.A, 0.0, 1.0, None),
               lib.gp_kg_set_points(h.h, nan.ctypes.data_as(_lib.c_double_p), c.A, 0.0, 1.0, None),
               lib.gp_kg_set_points(h.h, Xa, c.A, np.inf, 1.0, None), lib.gp_kg_set_points(h.h, Xa, c.A, 0.0, 0.0, None),
               lib.gp_kg_set_points(h.h, Xa, c.A, 0.0, np.nan, None), lib.gp_kg_info(h.h, None)):
        assert rc == _lib.GP_ERR_ARG
    assert h.kg.info() == c.A
    for y_std in (0.0, -1.0, np.inf, np.nan):
        rc, o = _raw_acq(h, y_std)
        assert rc == _lib.GP_ERR_ARG and np.all(o == SENTINEL)
        res = _raw_rows(h, p.Xs, 4, y_std)
        assert res[0] == _lib.GP_ERR_ARG and _untouched(res)
    bad = p.Xs[:4].copy()
    bad[2, 1] = np.inf
    for res in (_raw_rows(h, bad, 4), _raw_rows(h, p.Xs, 0), _raw_rows(h, p.Xs, 4, null_x=True), _raw_rows(h, p.Xs, 4, out=False),
                _raw_rows(h, p.Xs, 9)):                                           # (nine rows with a gradient: the table has none)
        assert res[0] == _lib.GP_ERR_ARG and _untouched(res)
    i64, f64 = np.zeros(4, dtype=np.int64), np.zeros(4)
    pi, pf = i64.ctypes.data_as(_lib.c_int64_p), f64.ctypes.data_as(_lib.c_double_p)
    assert lib.gp_kg_acq_argbest(h.h, 1.0, 0, pi, pf) == _lib.GP_ERR_ARG
    assert lib.gp_kg_acq_topk(h.h, 1.0, 1, 0, pi, pf) == _lib.GP_ERR_ARG
    assert lib.gp_kg_acq(h.h, 1.0, None) == _lib.GP_ERR_ARG
    assert _bits(h.kg.acq(c.y_std)) == _bits(before)
    assert _bits(*h.kg.rows(p.Xs[:4], c.y_std, grad=True)) == _bits(*rows_before)


def test_representers_and_points_coexist():
    s = setup("b")
    p, c = s.p, s.p.case
    rng = np.random.default_rng(3)
    Xr = rng.uniform(0, 1, (12, c.D))

    def belief(h):
        mu, cov = h.es_set_representers(Xr, YM, c.y_std)
        R = Xr.shape[0]
        h.es_set_belief(np.full(R, -np.log(R)), np.zeros(R), 0.1 * np.eye(R), np.zeros((R, R, R)), np.array([-1.0, 0.0, 1.0]))
        return mu, cov

    ref = _handle(p)                                                              # entropy search alone
    belief(ref)
    ref.set_candidates(p.Xs)
    es_alone = ref.es_acq(c.y_std)
    h = _handle(p)
    belief(h)
    h.kg.set_points(p.Xa, YM, c.y_std)                                            # the points arrive: the representers stay
    h.set_candidates(p.Xs)
    assert _bits(h.es_acq(c.y_std)) == _bits(es_alone)
    assert _bits(h.kg.acq(c.y_std)[:, 0]) == _bits(s.table)
    belief(h)                                                                     # the representers again: the points stay
    assert h.kg.info() == c.A
    h.set_candidates(p.Xs)
    assert _bits(h.kg.acq(c.y_std)[:, 0]) == _bits(s.table)
    assert _bits(h.es_acq_rows(p.Xs[:4], c.y_std)) == _bits(ref.es_acq_rows(p.Xs[:4], c.y_std))
    assert _bits(*h.kg.rows(p.Xs[:c.Mr], c.y_std, grad=True)) == _bits(s.rows, s.grad)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------
def _f2(X):
    X = np.atleast_2d(X)
    return (np.sin(3 * X[:, 0]) + (X[:, 1] - 0.4) ** 2)[:, None]


DOMAIN2 = [{"name": "x%d" % i, "type": "continuous", "domain": (0.0, 1.0)} for i in range(2)]


def _suggest(parallel):
    rng = np.random.default_rng(11)
    X0 = rng.uniform(0, 1, (40, 2))
    Y0 = _f2(X0) + 0.1 * rng.standard_normal((40, 1))                            # noisy observations: KG's home ground
    bo = gpo.BayesianOptimization(_f2, DOMAIN2, X=X0, Y=Y0, acquisition_type="KG", sampler_seed=0, num_kg_points=32,
                                  kg_table_size=2000, optimize_restarts=1, verbosity_model=False, parallel_anchors=parallel)
    calls = []
    inner = bo.acquisition.acquisition_function

    def recording(x):
        v = inner(x)
        calls.append((np.array(x, dtype=float, copy=True), np.array(v, dtype=float, copy=True)))
        return v

    bo.acquisition.acquisition_function = recording
    np.random.seed(5)                                                             # the optimiser's uniform samples
    return bo, bo.suggest_next_locations(), calls


def test_end_to_end_suggests_a_point():
    bo, x, calls = _suggest(False)
    acq, gp = bo.acquisition, bo.model.model
    assert isinstance(acq, gpo.AcquisitionKG) and bo.evaluator is None
    assert x.shape == (1, 2) and np.all(x >= 0.0) and np.all(x <= 1.0)
    assert acq.points.shape == (32, 2) and gp._h.kg.info() == 32
    Xt, vt = calls[0]                                                             # the optimiser's table and its scores
    anchors = Xt[np.argsort(vt.ravel())[:5]]
    k = gp.kern
    assert type(k).__name__ == "Matern52"
    noise = float(gp.Gaussian_noise.variance)
    shift, scale = gpo.acquisitions._normaliser(gp)
    ls = np.repeat(np.asarray(k.lengthscale.values, dtype=float), 2)[:2]
    fit = KT.fit("Mat52", float(k.variance), ls, KT.sigma2(noise, gp._h.fit_state()[2]), gp.X, gp.Y_normalized)
    tr = KT.evaluate("Mat52", float(k.variance), noise, fit, acq.points, np.vstack([x, anchors]), 0, shift, scale)
    allow = KT.value_allowance(noise, tr, float(k.variance), scale)
    v = np.asarray(tr.value, dtype=float)
    print("kg end to end: truth's KG of the point %.6e, of its anchors %s (allowances up to %.1e); fitted noise %.2e"
          % (v[0], np.array2string(v[1:], precision=4), float(allow.max()), noise))
    assert np.all(v[0] >= v[1:] - (allow[0] + allow[1:]))                         # L-BFGS-B never returns worse than its start
    _, x_par, _ = _suggest(True)
    assert np.array_equal(x_par, x)                                               # lockstep anchors: the serial loop's location
