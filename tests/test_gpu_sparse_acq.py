"""GPU: acquisitions over the sparse GP on the device -- the table entries (``gp_sparse_set_candidates``, ``gp_sparse_acq``,
``gp_sparse_acq_argbest``, ``gp_sparse_acq_topk``; csrc/api_sparse.hip) and the rows entries (``gp_sparse_predict_rows``,
``gp_sparse_acq_rows``; csrc/sparse_rows.hip) of include/gphip.h, and ``GPModel(sparse=True, device_acquisitions=True)`` over them.

Inputs: the cases of tests/_sparse_ref.py with variance 1.3, noise 2e-2, mc_max = 128 -- S1 (Mz = 10, one tile), S2a (S2 with the
first column of Y: N = 300, Mz = 130 crosses a tile with padding), S3 (Mz = 128, exactly one tile), S5 (Mz = 1), all four families;
S4 (D = 17, crosses GP_GRAD_CH = 16 and makes eight locations two passes of the fused path: 7 + 1) for RBF and Exponential, iso and
ARD; and B1 (N = 256, D = 8, Mz = 2048 -- the cap --, Matern-3/2 iso, 8 rows, RandomState(4242)).  The fused kernel's boundaries
along Mz: the 128-column step of a lane's walk along a row (S1 / S3 / S2a: below, on, past), the 8-row block of a workgroup (S1: 10
rows = 1 block + 2; S5: 1 row), and the PREFETCH SPLIT: the first SR_PF 128-column groups of a row pair are requested before k
exists and multiplied out of registers, the groups from SR_PF on run in a streaming loop of their own, and SR_PF differs per
instance -- 8 groups (1024 columns) in the 1-location and the <= 4-location instance, 4 groups (512 columns) in the 8-location
instance.  Every S case has at most 2 groups, so B1 (16 groups) is the case past the largest internal boundary, for EVERY instance:
its rows-against-table checks run for the first 1, 4, 5 and 8 rows (instances 1, 4, 8, 8), and the alone / slot-3-of-4 /
slot-6-of-8 bit check runs on it too -- there the three instances split the same row at different columns and must still add it in
the same order.  Every run re-asserts cond(Kmm) <= 8.9e4 and that no jitter ladder stepped, on oracle and device.

1. Rows posterior against the long-double truth, for the first 1, 4, 5 and 8 rows of Xs with and without noise: the rule of
   tests/test_gpu_sparse_gp.py, bound = max(MULT x the float64 oracle's own error, 1e-13 x scale).  MULT from
   profiles/sparse_acq_errors.txt (tools/sparse_acq_errors.py over this file's printed figures on an MI355X):
     "640 quantities, 16 above the floor; worst ratio above the floor 2.49 (S2a rbf ard: 5 rows noise=1 dvdx); x 4 = 9.94 -> MULT = 16."
     "S2a rbf ard: 5 rows noise=1 dvdx   scale 7.017e-01  device 1.441e-12  oracle 5.797e-13  ratio 2.49"
   (under the floor the largest ratio is 24.14 -- S3 Exponential iso, 1 row, var: device 2.3e-16, oracle 9.6e-18 -- and the floor
   is the bound).  The fused kernel adds each row of woodbury_inv lane by lane and then across the wave where LAPACK's dot
   products run along the row: forward errors of the same order cond eps, other constants.
2. Rows against table (all runs and B1): ``gp_sparse_predict_rows`` against ``gp_sparse_predict`` and ``gp_sparse_acq_rows`` against
   ``gp_sparse_acq`` on the staged table, EI (0.01) / LCB (2) / MPI (0.01), values and gradients, lp = 0 and lp = 1 (both
   transforms, 3 centres from Xs, r_x0 = 0.2, s_x0 = 0.1), relative to the largest entry of the vector compared.  The plain
   logarithm of a negative LCB is NaN on both routes alike (AcquisitionLP never asks for it: it switches LCB to softplus), and
   the penaliser's gradient is infinite at a location that is itself a centre; such entries must be the same on both routes
   and the finite ones are compared.  Tolerance = worst observed x 4 rounded up to a power of ten,
   capped at 1e-9:
     "924 comparisons; worst 1.323e-11 (S2a rbf ard: LCB lp=transform 0 gradient, scale 1.051e+02); x 4 = 5.292e-11 -> tolerance 1e-10."
   (S2a RBF has cond(Kmm) = 4.9e4, the largest of the runs; B1's worst is below 1e-13.)  The model level (7.) is held to the same
   tolerance: worst there 7.3e-14.
3. The rule's arithmetic: ``gp_sparse_acq`` on the 130-row table against ``acquisitions._Rule`` (float64 NumPy / SciPy) applied to
   what ``gp_sparse_predict(include_noise=True, grad=True)`` returns, with (y_mean, y_std) = (0, 1) and (0.3, 1.7); the penalised
   scores against ``oracle.cpu_ref.lp_penalized_acquisition`` / ``lp_d_acquisition`` fed the device's own un-penalised values.
   Only the libm calls differ; above 1e-12 of the largest entry is a formula difference:
     "720 comparisons; worst 1.611e-15 (S4 rbf iso: EI y=(0.3, 1.7) value, scale 1.723e-01); x 4 = 6.444e-15 -> tolerance 1e-14."
4. Arg-best and top-k, exact.  5. Bits.  6. State, refusals, counters.  7. The model level.
Every figure is printed before it is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib, acquisitions as A
from oracle import cpu_ref as O

import _sparse_ref as R

pytestmark = pytest.mark.gpu

MULT = 16.0          # check 1 (docstring)
FLOOR = 1e-13
TOL_ROWS_TABLE = 1e-10   # check 2 (docstring)
TOL_RULE = 1e-14        # check 3 (docstring)
FAMS = ["rbf", "Mat52", "Mat32", "Exponential"]
KID = {"rbf": _lib.GP_KERNEL_RBF, "Mat52": _lib.GP_KERNEL_MATERN52, "Mat32": _lib.GP_KERNEL_MATERN32,
       "Exponential": _lib.GP_KERNEL_EXPONENTIAL}
RUNS = [("S1", f, True) for f in FAMS] + [("S2a", f, True) for f in FAMS] + [("S3", f, False) for f in FAMS] + \
       [("S5", f, False) for f in FAMS] + [("S4", f, a) for f in ("rbf", "Exponential") for a in (False, True)]
IDS = ["%s-%s-%s" % (c, f, "ard" if a else "iso") for c, f, a in RUNS]
B1 = ("B1", "Mat32", False)
PRED_Q = ["mean", "var", "dmdx", "dvdx"]
ACQS = [("EI", _lib.GP_ACQ_EI, 0.01), ("LCB", _lib.GP_ACQ_LCB, 2.0), ("MPI", _lib.GP_ACQ_MPI, 0.01)]
LDT = np.longdouble
ROWS = 8             # locations of the rows comparisons: the first ROWS of Xs


def _inputs(case):
    if case == "B1":
        rng = np.random.RandomState(4242)
        X = rng.uniform(0, 1, (256, 8))
        Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((256, 1))
        Z = rng.uniform(0, 1, (2048, 8))
        Xs = rng.uniform(0, 1, (8, 8))
        return X, Y, Z, Xs
    X, Y, Z, Xs = R.case_inputs("S2" if case == "S2a" else case)
    return X, Y[:, :1].copy(), Z, Xs


@functools.lru_cache(maxsize=None)
def _ref(case, fam, ard, truth=True):
    """Inputs and the float64 oracle of a run -- fit, fmin, the posterior of the first ROWS rows of Xs with and without noise --
    and, with ``truth``, the same in long double.  Computed once and shared; read-only."""
    X, Y, Z, Xs = _inputs(case)
    ls = R.case_lengthscale(X.shape[1], ard)
    out = dict(X=X, Y=Y, Z=Z, Xs=Xs, ls=ls)
    for tag, lin in (("f64", R.F64), ("ld", R.LD))[:2 if truth else 1]:
        f = R.inference(fam, X, Z, Y, R.VARIANCE, ls, ard, R.NOISE, lin, grads=False)
        for inc in (True, False):
            f["pred%d" % inc] = dict(zip(PRED_Q, R.predict(f, Z, Xs[:ROWS], R.NOISE, inc, lin)))
        f["fmin"] = R.fmin(f, X)
        out[tag] = f
    return out


def _handle(case, fam, ard, truth=True):
    r = _ref(case, fam, ard, truth)
    h = _lib.Handle(0)
    h.set_option("mc_max", 128)
    h.set_data(r["X"], r["Y"])
    h.set_params(KID[fam], ard, R.VARIANCE, r["ls"], R.NOISE)
    h.sparse_set_inducing(r["Z"])
    return h, r


def _fit(h, r):
    """The sparse fit, under the suite's conditions."""
    _, jk, jb = h.sparse_fit()
    cond = float(np.linalg.cond(np.asarray(r["f64"]["Kmm"], dtype=float)))
    print("cond(Kmm) %.3g  oracle jitters %g %g  device jitters %g %g" % (cond, r["f64"]["jitter_kmm"], r["f64"]["jitter_b"], jk, jb))
    assert cond <= 8.9e4
    assert r["f64"]["jitter_kmm"] == 0.0 and r["f64"]["jitter_b"] == 0.0 and (jk, jb) == (0.0, 0.0)


def _check(what, got, oracle, truth):
    """The tolerance rule of check 1."""
    truth = np.asarray(truth, dtype=LDT)
    got = np.asarray(got, dtype=float).reshape(truth.shape)
    assert np.all(np.isfinite(got)), what
    scale = float(np.max(np.abs(truth)))
    dev = float(np.max(np.abs(got.astype(LDT) - truth)))
    orc = float(np.max(np.abs(np.asarray(oracle, dtype=LDT).reshape(truth.shape) - truth)))
    bound = max(MULT * orc, FLOOR * scale)
    print("%-44s scale %.3e  device %.3e  oracle %.3e  ratio %7.2f  bound %.3e" % (what, scale, dev, orc, dev / max(orc, 1e-300), bound))
    assert dev <= bound, (what, dev, bound)


def _rel(tag, what, got, want, tol):
    """Largest difference relative to the largest entry of ``want``.  Entries that are not finite -- the logarithm of a negative
    LCB, the penaliser's gradient at a location that is itself a centre (the reference divides by the distance) -- must be the
    same on both sides; the finite ones are compared."""
    got, want = np.asarray(got, dtype=float).reshape(-1), np.asarray(want, dtype=float).reshape(-1)
    ok = np.isfinite(want)
    assert got.shape == want.shape and np.array_equal(got[~ok], want[~ok], equal_nan=True), what
    if not ok.any():
        print("%s %-58s nothing finite on either side" % (tag, what))
        return
    assert np.all(np.isfinite(got[ok])), what
    scale = float(np.max(np.abs(want[ok])))
    rel = float(np.max(np.abs(got[ok] - want[ok]))) / max(scale, 1e-300)
    print("%s %-58s scale %.3e  rel %.3e  tol %.0e" % (tag, what, scale, rel, tol))
    assert rel <= tol, (what, rel, tol)


def _lp_spec(r, transform):
    Xs = r["Xs"]
    return (transform, Xs[[1, 3, 6]].copy(), np.full(3, 0.2), np.full(3, 0.1))


# ---- 1. rows posterior against the long-double truth ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,fam,ard", RUNS, ids=IDS)
def test_rows_posterior_against_long_double(case, fam, ard):
    h, r = _handle(case, fam, ard)
    try:
        _fit(h, r)
        tag = "%s %s %s" % (case, fam, "ard" if ard else "iso")
        for inc in (True, False):
            for M in (1, 4, 5, 8):
                m, v, dm, dvx = h.sparse_predict_rows(r["Xs"][:M], include_noise=inc, grad=True)
                m0, v0 = h.sparse_predict_rows(r["Xs"][:M], include_noise=inc)
                assert np.array_equal(m0, m) and np.array_equal(v0, v)      # the value call's bits are the gradient call's
                for q, g in zip(PRED_Q, (m, v[:, 0], dm, dvx)):
                    _check("%s: %d rows noise=%d %s" % (tag, M, inc, q), g, r["f64"]["pred%d" % inc][q][:M], r["ld"]["pred%d" % inc][q][:M])
        assert np.array_equal(h.sparse_mean_grad_rows(r["Xs"][:5]), h.sparse_predict_rows(r["Xs"][:5], grad=True)[2])
        assert h.sparse_rows_stats() == dict(fused=18, fallback=0)
    finally:
        h.close()


# ---- 2. rows against table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fam,ard", RUNS + [B1], ids=IDS + ["B1-Mat32-iso"])
def test_rows_against_table(case, fam, ard):
    h, r = _handle(case, fam, ard, truth=case != "B1")
    try:
        _fit(h, r)
        tag = "ROWS-TABLE %s %s %s:" % (case, fam, "ard" if ard else "iso")
        Xs, few = r["Xs"], r["Xs"][:ROWS]
        fmin = float(r["f64"]["fmin"])
        for inc in (True, False):
            tab = h.sparse_predict(few, include_noise=inc, grad=True)
            row = h.sparse_predict_rows(few, include_noise=inc, grad=True)
            for q, a, b in zip(PRED_Q, row, tab):
                _rel(tag, "noise=%d %s" % (inc, q), a, b, TOL_ROWS_TABLE)
        h.sparse_set_candidates(Xs)
        # every instance of the fused kernel (1, <= 4, <= 8 locations), which split a row at different columns
        tab = h.sparse_predict(few, include_noise=True, grad=True)
        spec = _lp_spec(r, 0)
        tv, tg = h.sparse_acq(_lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=spec)
        for M in (1, 4, 5):
            for q, a, b in zip(PRED_Q, h.sparse_predict_rows(few[:M], include_noise=True, grad=True), tab):
                _rel(tag, "%d rows noise=1 %s" % (M, q), a, b[:M], TOL_ROWS_TABLE)
            rv, rg = h.sparse_acq_rows(few[:M], _lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=spec)
            _rel(tag, "%d rows EI lp=transform 0 value" % M, rv, tv[:M], TOL_ROWS_TABLE)
            _rel(tag, "%d rows EI lp=transform 0 gradient" % M, rg, tg[:M], TOL_ROWS_TABLE)
        for name, aid, par in ACQS:
            for lp in (None, _lp_spec(r, 0), _lp_spec(r, 1)):
                what = "%s lp=%s" % (name, "off" if lp is None else "transform %d" % lp[0])
                tv, tg = h.sparse_acq(aid, par, fmin, grad=True, lp=lp)
                assert np.array_equal(h.sparse_acq(aid, par, fmin, lp=lp), tv, equal_nan=True)
                rv, rg = h.sparse_acq_rows(few, aid, par, fmin, grad=True, lp=lp)
                assert np.array_equal(h.sparse_acq_rows(few, aid, par, fmin, lp=lp), rv, equal_nan=True)
                assert rv.shape == tv[:ROWS].shape and rg.shape == (ROWS, Xs.shape[1])
                _rel(tag, what + " value", rv, tv[:ROWS], TOL_ROWS_TABLE)
                _rel(tag, what + " gradient", rg, tg[:ROWS], TOL_ROWS_TABLE)
    finally:
        h.close()


# ---- 3. the rule's arithmetic ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fam,ard", RUNS, ids=IDS)
def test_table_scores_against_the_host_rule(case, fam, ard):
    h, r = _handle(case, fam, ard, truth=False)
    try:
        _fit(h, r)
        tag = "RULE %s %s %s:" % (case, fam, "ard" if ard else "iso")
        Xs = r["Xs"]
        fmin0 = float(r["f64"]["fmin"])
        mean, var, dm, dv = h.sparse_predict(Xs, include_noise=True, grad=True)
        h.sparse_set_candidates(Xs)
        rules = dict(EI=A._RULES["EI"], LCB=A._RULES["LCB"], MPI=A._RULES["MPI"])
        for ym, ys in ((0.0, 1.0), (0.3, 1.7)):
            fmin = fmin0 * ys + ym
            # GPModel.predict_withGradients over a Standardize normaliser (gpmodel.py:131-142, gp.py:344-352)
            mu, v = mean * ys + ym, np.maximum(var * ys ** 2, 1e-10)
            sd = np.sqrt(v)
            dmu, dsd = dm[..., 0] * ys, dv * ys ** 2 / (2 * sd)
            for name, aid, par in ACQS:
                val, grad = rules[name].gradient(par, fmin, mu, sd.copy(), dmu, dsd)
                out, dout = h.sparse_acq(aid, par, fmin, ym, ys, grad=True)
                assert out.shape == (130, 1) and dout.shape == (130, Xs.shape[1])
                what = "%s y=(%g, %g)" % (name, ym, ys)
                _rel(tag, what + " value", out, -val, TOL_RULE)
                _rel(tag, what + " gradient", dout, -grad, TOL_RULE)
                for tr, trname in ((0, "none"), (1, "softplus")):
                    lp = _lp_spec(r, tr)
                    pv, pg = h.sparse_acq(aid, par, fmin, ym, ys, grad=True, lp=lp)
                    assert pv.shape == (130,)
                    with np.errstate(all="ignore"):
                        wv = O.lp_penalized_acquisition(out, Xs, lp[1], lp[2], lp[3], trname)
                        wg = O.lp_d_acquisition(out, dout, Xs, lp[1], lp[2], lp[3], trname)
                    _rel(tag, what + " lp %s value" % trname, pv, wv, TOL_RULE)
                    _rel(tag, what + " lp %s gradient" % trname, pg, wg, TOL_RULE)
    finally:
        h.close()


# ---- 4. arg-best and top-k: exact ------------------------------------------------------------------------------------------------
def test_argbest_and_topk_are_numpys():
    h, r = _handle("S2a", "Mat52", True, truth=False)
    try:
        _fit(h, r)
        Xs, fmin = r["Xs"], float(r["f64"]["fmin"])
        aid, par = _lib.GP_ACQ_EI, 0.01
        h.sparse_set_candidates(Xs)
        for lp in (None, _lp_spec(r, 0)):
            v = np.asarray(h.sparse_acq(aid, par, fmin, lp=lp)).reshape(-1)
            for sense in (-1, +1):
                for exclude in ([], [int(np.argmin(v))], [0, 7, 40, int(np.argmin(v)), int(np.argmax(v))]):
                    masked = v.copy()
                    masked[list(set(exclude))] = np.inf if sense < 0 else -np.inf
                    want = int(np.argmin(masked) if sense < 0 else np.argmax(masked))
                    got = h.sparse_acq_argbest(aid, par, fmin, sense, lp=lp, exclude=exclude)
                    print("argbest lp=%s sense %+d exclude %s: %s, want row %d" % (lp is not None, sense, exclude, got, want))
                    assert got == (want, masked[want])
        v = h.sparse_acq(aid, par, fmin)[:, 0]
        for sense in (-1, +1):
            order = np.argsort(v if sense < 0 else -v, kind="stable")
            for k in (1, 5, 64):
                idx, val = h.sparse_acq_topk(aid, par, fmin, sense, k)
                assert np.array_equal(idx, order[:k]) and np.array_equal(val, v[order[:k]])
        # M = 3 < k: the tail is marked empty
        h.sparse_set_candidates(Xs[:3])
        idx, val = h.sparse_acq_topk(aid, par, fmin, -1, 5)
        v3 = h.sparse_acq(aid, par, fmin)[:, 0]
        assert np.array_equal(v3, v[:3])
        assert np.array_equal(idx[:3], np.argsort(v3, kind="stable")) and np.array_equal(idx[3:], [-1, -1]) and np.all(np.isinf(val[3:]))
        # a real tie: row 40 a copy of row 7, both the winner -> the lower index
        for sense in (-1, +1):
            w = int(np.argmin(v) if sense < 0 else np.argmax(v))
            T = Xs.copy()
            T[[w, 7]] = T[[7, w]]
            T[40] = T[7]
            h.sparse_set_candidates(T)
            vt = h.sparse_acq(aid, par, fmin)[:, 0]
            assert vt[7] == vt[40] == v[w]
            assert h.sparse_acq_argbest(aid, par, fmin, sense) == (7, v[w])
            assert h.sparse_acq_topk(aid, par, fmin, sense, 2)[0].tolist() == [7, 40]
    finally:
        h.close()


# ---- 5. bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fam,ard", [("S1", "rbf", True), ("S2a", "Mat52", True), ("S4", "Exponential", True), B1])
def test_bits_do_not_depend_on_company(case, fam, ard):
    h, r = _handle(case, fam, ard, truth=False)
    try:
        _fit(h, r)
        Xs, fmin = r["Xs"], float(r["f64"]["fmin"])
        x = Xs[7:8]
        lp = _lp_spec(r, 0)
        four = np.vstack([Xs[0:2], x, Xs[2:3]])             # slot 3 of 4
        eight = np.vstack([Xs[0:5], x, Xs[5:7]])            # slot 6 of 8
        alone = h.sparse_predict_rows(x, grad=True)
        assert all(np.array_equal(a, b) for a, b in zip(alone, h.sparse_predict_rows(x, grad=True)))      # the same call twice
        assert all(np.array_equal(a[0], b[2]) for a, b in zip(alone, h.sparse_predict_rows(four, grad=True)))
        assert all(np.array_equal(a[0], b[5]) for a, b in zip(alone, h.sparse_predict_rows(eight, grad=True)))
        assert np.array_equal(h.sparse_mean_grad_rows(x)[0], h.sparse_mean_grad_rows(eight)[5])
        for name, aid, par in ACQS[:1] + ACQS[2:]:
            for spec in (None, lp):
                a1 = h.sparse_acq_rows(x, aid, par, fmin, grad=True, lp=spec)
                assert all(np.array_equal(a, b) for a, b in zip(a1, h.sparse_acq_rows(x, aid, par, fmin, grad=True, lp=spec)))
                assert all(np.array_equal(a[0], b[2]) for a, b in zip(a1, h.sparse_acq_rows(four, aid, par, fmin, grad=True, lp=spec)))
                assert all(np.array_equal(a[0], b[5]) for a, b in zip(a1, h.sparse_acq_rows(eight, aid, par, fmin, grad=True, lp=spec)))
        if case == "B1":
            return
        # a row's table score: the same bits in tables of 1, 5 and 130 rows, at any position
        h.sparse_set_candidates(Xs)
        full = h.sparse_acq(_lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=lp)
        assert all(np.array_equal(a, b) for a, b in zip(full, h.sparse_acq(_lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=lp)))
        for rows in (slice(0, 1), slice(0, 5), slice(129, 130), slice(125, 130)):
            h.sparse_set_candidates(Xs[rows])
            sub = h.sparse_acq(_lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=lp)
            assert all(np.array_equal(a, b[rows]) for a, b in zip(sub, full)), rows
        # the cached posterior is gp_sparse_predict's, bit for bit: the negated LCB with weight 0 is the mean itself
        h.sparse_set_candidates(Xs)
        mean, var = h.sparse_predict(Xs, include_noise=True)
        assert np.array_equal(h.sparse_acq(_lib.GP_ACQ_LCB, 0.0, 0.0), mean)
    finally:
        h.close()


# ---- 6. state ----------------------------------------------------------------------------------------------------------------------
def test_table_and_cache_survive_interleaved_calls_and_follow_a_refit():
    h, r = _handle("S2a", "Mat32", True, truth=False)
    try:
        _fit(h, r)
        Xs, fmin = r["Xs"], float(r["f64"]["fmin"])
        spec = _lp_spec(r, 1)
        h.sparse_set_candidates(Xs)
        before = h.sparse_acq(_lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=spec)
        best = h.sparse_acq_argbest(_lib.GP_ACQ_EI, 0.01, fmin, +1, lp=spec)
        h.sparse_predict(Xs[:3], grad=True)
        h.sparse_predict(Xs[::-1].copy(), grad=True)
        h.sparse_fmin()
        h.sparse_predict_rows(Xs[:1], grad=True)
        h.sparse_predict_rows(Xs[:9], grad=True)                          # the fallback's scratch, not the table
        h.sparse_acq_rows(Xs[5:14], _lib.GP_ACQ_MPI, 0.01, fmin, grad=True, lp=_lp_spec(r, 0))
        h.sparse_acq_rows(Xs[:2], _lib.GP_ACQ_LCB, 2.0, fmin, lp=spec)
        h.sparse_mean_grad_rows(Xs[:3])
        after = h.sparse_acq(_lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=spec)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert h.sparse_acq_argbest(_lib.GP_ACQ_EI, 0.01, fmin, +1, lp=spec) == best
        # new parameters drop the cache, not the table; after the refit the scores are a fresh context's
        h.set_params(KID["Mat32"], True, R.VARIANCE, 1.3 * r["ls"], R.NOISE)
        assert h.lib.gp_sparse_acq(h.h, 0, 0.01, fmin, 0.0, 1.0, 0, 0, None, 0, None, None, _lib.dptr(np.empty(130)), None) == _lib.GP_ERR_STATE
        h.sparse_fit()
        moved = h.sparse_acq(_lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=spec)
        assert not np.array_equal(moved[0], before[0])
        fresh = _lib.Handle(0)
        try:
            fresh.set_option("mc_max", 128)
            fresh.set_data(r["X"], r["Y"])
            fresh.set_params(KID["Mat32"], True, R.VARIANCE, 1.3 * r["ls"], R.NOISE)
            fresh.sparse_set_inducing(r["Z"])
            fresh.sparse_fit()
            fresh.sparse_set_candidates(Xs)
            want = fresh.sparse_acq(_lib.GP_ACQ_EI, 0.01, fmin, grad=True, lp=spec)
        finally:
            fresh.close()
        assert all(np.array_equal(a, b) for a, b in zip(moved, want))
    finally:
        h.close()


def test_exact_model_bits_survive_the_sparse_acquisition_calls():
    """tests/test_gpu_sparse_gp.py's test_exact_model_bits_survive_interleaved_sparse_calls over the new entries: the exact model's
    fit, resident candidates, posterior, scores, fmin -- and a ``gp_acq_rows`` with an LP batch issued before and after a sparse
    LP call, which shares the batch's device scratch -- return a fresh context's bits."""
    r = _ref("S1", "Mat52", True, False)
    Xs = r["Xs"]
    batch = (0, Xs[[2, 9]].copy(), np.array([0.15, 0.25]), np.array([0.1, 0.2]))
    other = (1, Xs[[4, 5, 8]].copy(), np.full(3, 0.3), np.full(3, 0.05))

    def setup():
        h = _lib.Handle(0)
        h.set_option("mc_max", 128)
        h.set_data(r["X"], r["Y"])
        h.set_params(KID["Mat52"], True, R.VARIANCE, r["ls"], R.NOISE)
        return h

    def exact(h):
        fit = h.fit()
        rows = h.acq_rows(Xs[:3], _lib.GP_ACQ_EI, 0.01, 0.0, grad=True, lp=batch)
        h.set_candidates(Xs)
        fmin = h.fmin()
        return (fit, h.predict(include_noise=True), fmin, h.acq_grad(_lib.GP_ACQ_EI, 0.01, fmin),
                h.acq_lp(_lib.GP_ACQ_EI, 0.01, fmin, 0, *batch[1:]), rows)

    def same(a, b):
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(a, b)

    def rows(h):
        return h.acq_rows(Xs[:3], _lib.GP_ACQ_EI, 0.01, 0.0, grad=True, lp=batch)

    fresh = setup()
    want = exact(fresh)
    fresh.close()
    h = setup()
    try:
        assert same(exact(h), want)
        fmin = want[2]
        h.sparse_set_inducing(r["Z"])
        h.sparse_fit()
        sf = h.sparse_fmin()
        h.sparse_set_candidates(Xs[::2].copy())
        h.sparse_acq(_lib.GP_ACQ_EI, 0.01, sf, grad=True, lp=other)
        h.sparse_acq_argbest(_lib.GP_ACQ_LCB, 2.0, sf, -1, lp=other, exclude=[1, 2])
        h.sparse_acq_topk(_lib.GP_ACQ_EI, 0.01, sf, -1, 5)
        h.sparse_predict_rows(Xs[:8], grad=True)
        h.sparse_predict_rows(Xs[:9], grad=True)
        h.sparse_acq_rows(Xs[:4], _lib.GP_ACQ_MPI, 0.01, sf, grad=True, lp=other)
        h.sparse_acq_rows(Xs[:12], _lib.GP_ACQ_EI, 0.01, sf, grad=True, lp=other)
        # the exact model's resident candidates, their posterior and scores, read without restaging
        assert same(h.predict(include_noise=True), want[1]) and h.fmin() == want[2]
        assert same(h.acq_grad(_lib.GP_ACQ_EI, 0.01, fmin), want[3])
        assert same(h.acq_lp(_lib.GP_ACQ_EI, 0.01, fmin, 0, *batch[1:]), want[4])
        # the penaliser's batch lives in scratch both models share: an exact gp_acq_rows keeps the batch it uploaded cached, and a
        # sparse call with another batch in between must not leave it believing the scratch still holds its own
        assert same(rows(h), want[5])
        h.sparse_acq(_lib.GP_ACQ_EI, 0.01, sf, grad=True, lp=other)                   # table path: another batch into the scratch
        assert same(rows(h), want[5])
        h.sparse_acq_rows(Xs[:4], _lib.GP_ACQ_MPI, 0.01, sf, grad=True, lp=other)     # fused path with another batch
        assert same(rows(h), want[5])
        h.sparse_acq_rows(Xs[:12], _lib.GP_ACQ_MPI, 0.01, sf, grad=True, lp=other)    # the fallback with another batch
        assert same(rows(h), want[5])
        assert same(exact(h), want)
    finally:
        h.close()


def test_return_codes_and_route_counters():
    lib = _lib.load()
    r = _ref("S1", "rbf", True, False)
    D = 3
    buf = np.zeros(8192)
    p = _lib.dptr(buf)
    vp = buf.ctypes.data
    i64 = ctypes.c_int64()
    d = ctypes.c_double()
    ex = np.zeros(300, dtype=np.int64)
    pex = ex.ctypes.data_as(_lib.c_int64_p)
    ARG, STATE = _lib.GP_ERR_ARG, _lib.GP_ERR_STATE

    def acq(g, type_=0, lp=0, tr=0, nb=0, Xb=None, out=p):
        return lib.gp_sparse_acq(g, type_, 0.01, 0.0, 0.0, 1.0, lp, tr, Xb, nb, Xb, Xb, out, None)

    def argbest(g, sense=1, nex=0, e=None, idx=ctypes.byref(i64)):
        return lib.gp_sparse_acq_argbest(g, 0, 0.01, 0.0, 0.0, 1.0, 0, 0, None, 0, None, None, sense, e, nex, idx, ctypes.byref(d))

    def topk(g, k=1, sense=1):
        return lib.gp_sparse_acq_topk(g, 0, 0.01, 0.0, 0.0, 1.0, sense, k, pex, p)

    def prow(g, M=1, mean=vp, var=vp, dm=None, dv=None, Xs=vp):
        return lib.gp_sparse_predict_rows(g, Xs, M, 1, mean, var, dm, dv)

    def arow(g, M=1, type_=0, lp=0, tr=0, nb=0, Xb=None, out=vp):
        return lib.gp_sparse_acq_rows(g, vp, M, type_, 0.01, 0.0, 0.0, 1.0, lp, tr, Xb, nb, Xb, Xb, out, None)

    calls = (acq, argbest, topk, prow, arow)
    assert lib.gp_sparse_set_candidates(None, p, 1) == ARG and all(c(None) == ARG for c in calls)
    assert lib.gp_sparse_rows_stats(None, None, None) == ARG
    h = _lib.Handle(0)
    try:
        g = h.h
        assert lib.gp_sparse_set_candidates(g, p, 1) == STATE                               # no data
        assert all(c(g) == STATE for c in calls)
        h.set_data(r["X"], r["Y"])
        assert all(c(g) == STATE for c in calls)                                            # no parameters
        h.set_params(KID["rbf"], True, R.VARIANCE, r["ls"], R.NOISE)
        assert all(c(g) == STATE for c in calls)                                            # no inducing inputs
        h.sparse_set_inducing(r["Z"])
        assert all(c(g) == STATE for c in calls)                                            # no sparse fit
        assert lib.gp_sparse_set_candidates(g, None, 1) == ARG and lib.gp_sparse_set_candidates(g, p, 0) == ARG
        h.sparse_fit()
        assert acq(g) == STATE and argbest(g) == STATE and topk(g) == STATE                 # no table
        assert b"gp_sparse_set_candidates" in lib.gp_last_error()
        h.sparse_set_candidates(r["Xs"][:20])
        assert acq(g) == 0 and argbest(g) == 0 and topk(g) == 0 and prow(g) == 0 and arow(g) == 0
        assert acq(g, out=None) == ARG and argbest(g, idx=None) == ARG
        assert acq(g, type_=3) == ARG and acq(g, type_=-1) == ARG and arow(g, type_=7) == ARG
        assert acq(g, lp=1, tr=2) == ARG and acq(g, lp=1, nb=-1) == ARG and acq(g, lp=1, nb=257, Xb=p) == ARG
        assert acq(g, lp=1, nb=2, Xb=None) == ARG and arow(g, lp=1, tr=5) == ARG and arow(g, lp=1, nb=3) == ARG
        assert acq(g, lp=0, tr=2) == 0                                                      # the batch is not looked at without lp
        assert argbest(g, sense=0) == ARG and argbest(g, sense=2) == ARG and topk(g, sense=0) == ARG
        assert topk(g, k=0) == ARG and topk(g, k=65) == ARG and topk(g, k=64) == 0
        assert argbest(g, nex=-1, e=pex) == ARG and argbest(g, nex=257, e=pex) == ARG and argbest(g, nex=1, e=None) == ARG
        ex[0] = 20
        assert argbest(g, nex=1, e=pex) == ARG                                              # an excluded row outside the table
        ex[0] = -1
        assert argbest(g, nex=1, e=pex) == ARG
        ex[0] = 19
        assert argbest(g, nex=1, e=pex) == 0
        assert prow(g, M=0) == ARG and arow(g, M=0) == ARG and prow(g, Xs=None) == ARG and arow(g, out=None) == ARG
        assert prow(g, dv=vp) == ARG and prow(g, dm=vp) == ARG                              # dvdx needs dmdx; dmdx alone comes bare
        assert prow(g, mean=None, var=None, dm=vp) == 0
        # the route counters: fused up to 8 locations, the table arithmetic from 9 on and with small_m = 0
        s0 = h.sparse_rows_stats()
        h.sparse_predict_rows(r["Xs"][:8])
        h.sparse_acq_rows(r["Xs"][:1], 0, 0.01, 0.0, grad=True)
        assert h.sparse_rows_stats() == dict(fused=s0["fused"] + 2, fallback=s0["fallback"])
        h.sparse_predict_rows(r["Xs"][:9])
        h.sparse_acq_rows(r["Xs"][:9], 0, 0.01, 0.0)
        assert h.sparse_rows_stats() == dict(fused=s0["fused"] + 2, fallback=s0["fallback"] + 2)
        h.set_option("small_m", 0)
        one = h.sparse_predict_rows(r["Xs"][:1], grad=True)
        assert h.sparse_rows_stats() == dict(fused=s0["fused"] + 2, fallback=s0["fallback"] + 3)
        assert all(np.array_equal(a, b) for a, b in zip(one, h.sparse_predict(r["Xs"][:1], grad=True)))   # the table arithmetic's bits
        h.set_option("small_m", 8)
        assert h.rows_stats() == dict(fused=0, fallback=0)                                  # the exact model's counters are its own
        # P != 1
        h.set_data(r["X"], np.tile(r["Y"], (1, 2)))
        h.sparse_fit()
        assert all(c(g) == ARG for c in calls)
    finally:
        h.close()


# ---- 7. the model level --------------------------------------------------------------------------------------------------------------
def _model_data(N=60, D=2, seed=21):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    return X, Y


def _twins():
    X, Y = _model_data()
    out = []
    for flag in (True, False):
        np.random.seed(3)
        gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, variance=1.3, lengthscale=0.4), sparse=True, num_inducing=8, max_iters=0,
                         verbose=False, device_acquisitions=flag)
        gm.updateModel(X, Y, None, None)
        gm.model.likelihood.variance.set(0.05)
        out.append(gm)
    assert np.array_equal(out[0].model.Z_values, out[1].model.Z_values)
    return out


def test_model_twins_agree():
    on, off = _twins()
    try:
        table = np.random.RandomState(8).uniform(0, 1, (130, 2))
        tag = "MODEL"
        stats0 = on.model._h.sparse_rows_stats()
        for cls, kw in ((gpo.AcquisitionEI, dict(jitter=0.01)), (gpo.AcquisitionLCB, dict(exploration_weight=2)),
                        (gpo.AcquisitionMPI, dict(jitter=0.01))):
            a_on, a_off = cls(on, **kw), cls(off, **kw)
            assert a_on._sparse_device_ok() and not a_off._sparse_device_ok()
            assert not a_on._device_ok() and not a_off._device_ok()
            for M in (1, 5, 130):
                _rel(tag, "%s %d rows value" % (cls.__name__, M), a_on.acquisition_function(table[:M]), a_off.acquisition_function(table[:M]), TOL_ROWS_TABLE)
                v1, g1 = a_on.acquisition_function_withGradients(table[:M])
                v0, g0 = a_off.acquisition_function_withGradients(table[:M])
                assert v1.shape == v0.shape == (M, 1) and g1.shape == g0.shape == (M, 2)
                _rel(tag, "%s %d rows value (gradient call)" % (cls.__name__, M), v1, v0, TOL_ROWS_TABLE)
                _rel(tag, "%s %d rows gradient" % (cls.__name__, M), g1, g0, TOL_ROWS_TABLE)
            for sense in (-1, +1):
                i1, b1 = a_on.argbest(table, sense)
                i0, b0 = a_off.argbest(table, sense)
                assert i1 == i0 and abs(b1 - b0) <= TOL_ROWS_TABLE * abs(b0)
                k1, w1 = a_on.topk(table, 5, sense)
                k0, w0 = a_off.topk(table, 5, sense)
                assert np.array_equal(k1, k0)
                _rel(tag, "%s topk sense %+d" % (cls.__name__, sense), w1, w0, TOL_ROWS_TABLE)
            # the penalised acquisition after update_batches
            l_on, l_off = gpo.AcquisitionLP(on, acquisition=a_on), gpo.AcquisitionLP(off, acquisition=a_off)
            assert l_on._lp_sparse_ok() and not l_off._lp_sparse_ok() and not l_on._lp_device_ok()
            for lp in (l_on, l_off):
                lp.update_batches(table[[3, 17]], 2.5, float(on.model.Y.min()))
            _rel(tag, "%s LP radii" % cls.__name__, l_on.r_x0, l_off.r_x0, TOL_ROWS_TABLE)
            _rel(tag, "%s LP widths" % cls.__name__, l_on.s_x0, l_off.s_x0, TOL_ROWS_TABLE)
            l_off.r_x0, l_off.s_x0 = l_on.r_x0, l_on.s_x0        # one batch for both: what follows compares the scoring
            for M in (1, 5, 130):
                _rel(tag, "%s LP %d rows value" % (cls.__name__, M), l_on.acquisition_function(table[:M]), l_off.acquisition_function(table[:M]), TOL_ROWS_TABLE)
                v1, g1 = l_on.acquisition_function_withGradients(table[:M])
                v0, g0 = l_off.acquisition_function_withGradients(table[:M])
                assert v1.shape == v0.shape == (M,) and g1.shape == g0.shape == (M, 2)
                _rel(tag, "%s LP %d rows gradient" % (cls.__name__, M), g1, g0, TOL_ROWS_TABLE)
            assert l_on.argbest(table, +1, exclude=[3, 17])[0] == l_off.argbest(table, +1, exclude=[3, 17])[0]
        stats = on.model._h.sparse_rows_stats()
        print("rows calls of the flagged twin: %s -> %s; of the other: %s" % (stats0, stats, off.model._h.sparse_rows_stats()))
        assert stats["fused"] > stats0["fused"] and stats["fallback"] == stats0["fallback"]
        assert off.model._h.sparse_rows_stats() == dict(fused=0, fallback=0)
        # predict / predict_withGradients / get_fmin of the twins
        for M in (1, 8, 9):
            for a, b in zip(on.predict_withGradients(table[:M]), off.predict_withGradients(table[:M])):
                _rel(tag, "predict_withGradients %d rows" % M, a, b, TOL_ROWS_TABLE)
        assert on.get_fmin() == off.get_fmin()
    finally:
        on.model.close()
        off.model.close()


def test_table_batch_and_bayesian_optimization_on_the_device_route():
    on, off = _twins()
    try:
        table = np.random.RandomState(9).uniform(0, 1, (130, 2))
        space = gpo.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}])
        l_on = gpo.AcquisitionLP(on, space, acquisition=gpo.AcquisitionEI(on, space, jitter=0.01))
        l_off = gpo.AcquisitionLP(off, space, acquisition=gpo.AcquisitionEI(off, space, jitter=0.01))
        picked = []
        orig = l_on.argbest

        def spy(x, sense=+1, exclude=(), devices=None):
            scores = np.array(l_on.acquisition_function(x), dtype=float)      # the device's own penalised vector
            scores[list(exclude)] = -np.inf
            got = orig(x, sense, exclude=exclude, devices=devices)
            picked.append((got[0], int(np.argmax(scores))))
            return got

        l_on.argbest = spy
        np.random.seed(11)
        rows_on = gpo.LocalPenalization(l_on, 3).compute_batch_from_table(table, sense=+1)
        np.random.seed(11)
        rows_off = gpo.LocalPenalization(l_off, 3).compute_batch_from_table(table, sense=+1)
        print("table batch: device route %s, host route %s; per round (picked, arg-max of the device's vector) %s" % (rows_on, rows_off, picked))
        assert rows_on[0] == rows_off[0] and len(set(rows_on)) == 3
        assert len(picked) == 3 and all(a == b for a, b in picked)
        s = on.model._h.sparse_rows_stats()
        assert s["fused"] > 0 and s["fallback"] == 0          # the hammer precompute and estimate_L's polish went down by value
    finally:
        on.model.close()
        off.model.close()
    X0, Y0 = _model_data(N=30)
    domain = [{'name': 'x%d' % i, 'type': 'continuous', 'domain': (0.0, 1.0)} for i in range(2)]
    np.random.seed(5)
    model = gpo.GPModel(sparse=True, num_inducing=8, exact_feval=True, max_iters=0, verbose=False, device_acquisitions=True)
    bo = gpo.BayesianOptimization(lambda x: np.sin(3 * np.atleast_2d(x).sum(1))[:, None], domain, X=X0, Y=Y0, model=model,
                                  evaluator_type='local_penalization', batch_size=3)
    try:
        xs = bo.suggest_next_locations()
        print("local-penalisation batch over the sparse model:", xs.tolist())
        assert xs.shape == (3, 2) and np.all((xs >= 0.0) & (xs <= 1.0))
        assert bo.acquisition._lp_sparse_ok() and not bo.acquisition.acq._device_ok()
        s = model.model._h.sparse_rows_stats()
        print("rows calls:", s)
        assert s["fused"] > 0
    finally:
        model.model.close()
