"""GPU: the ensemble entry points (gp_ens_fit, gp_ens_predict_rows, gp_ens_acq_rows, gp_ens_acq, gp_ens_acq_argbest, gp_ens_info),
``GPModel_MCMC`` and the integrated acquisitions on the device.

Cases: tests/_family_shapes.py a, b, c, f, h, j (P = 1), all four families.  Members: ``FS.members(cid)`` (three), and a five-member
set made from them -- members 2, 0, 1 in that order, then member 0 and member 1 rescaled.  Truth: ``FS.oracle(fam, cid, member)``
(direct distances); for the rescaled members an ``OracleGP`` built the same way.

Tolerances (profiles/ens_errors.txt, written by tools/ens_errors.py from this file's printed figures on an MI355X):
* checks 1 and 2 (posterior, fmin and integrated acquisition against the oracle): the device's error is at most
  max(MULT x the float64 oracle's own scatter, FLOOR x scale); the scatter is the distance between the direct-distance and the
  Gram-trick oracle (``FS.oracle(..., direct=False)``), scale the largest reference entry, FLOOR = 1e-13 the project's floor
  (profiles/sparse_acq_errors.txt), MULT = 4 x the worst ratio measured above the floor, rounded up to a power of two: 14.82
  (rbf h set5: 1 rows MPI gradient, a tail value of scale 1.9e-13) -> 64.
* the rule's arithmetic (the device's own gp_ens_predict_rows output through acquisitions._Rule in NumPy against
  gp_ens_acq_rows), relative to the largest entry: worst measured 1.17e-13 (Mat32 h set3: 1 rows EI value, scale 5.5e-18)
  -> RULE_TOL = 1e-12.  The large figures are one-row calls whose only entry lies far in the tail, u = (fmin - m - jitter) / s
  near -8: there EI = s (u Phi + phi) cancels to phi / u^2, so the last-place differences between the device's erfc / exp and
  SciPy's are magnified by u^2 ~ 70 relative to the value itself; where a call holds an entry of ordinary size the figure is
  1e-15 (profiles/ens_errors.txt).
* check 3, rows against table (gp_ens_acq_rows against gp_ens_acq), relative to the largest entry: worst measured 4.3e-14
  (rbf j: EI) -> TABLE_TOL = 1e-12.
None of these is measured against the code under test alone: the first two against the oracle / NumPy, the third between two
device routes that contract in different orders, both held to the oracle by checks 1 and 2.
* check 4: a one-member ensemble against gp_predict_rows / gp_acq_rows of a context set to that member is BIT EQUALITY: the
  ensemble kernels run the single model's device bodies (csrc/rows_body.h).
* check 6, the model level: prediction lists against ``OracleGP`` at the model's ``hmc_samples`` at 1e-6 of the largest reference
  entry (the project's own bound for posteriors, tests/test_gpu_family_shapes.py); the acquisition classes' device route against
  the reference formulas over the model's lists at RULE_TOL (rows) and TABLE_TOL (table).
Every figure is printed before it is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd.acquisitions import _RULES
from oracle import cpu_ref as O

import _family_shapes as FS
import _kernel_families as KF

pytestmark = pytest.mark.gpu

MULT, FLOOR = 64.0, 1e-13
RULE_TOL = 1e-12
TABLE_TOL = 1e-12

CIDS = "abcfhj"
PAIRS = [pytest.param(f, c, id="%s-%s" % (f, c)) for f in FS.ALL_FAMILIES for c in CIDS]
ACQS = (("EI", _lib.GP_ACQ_EI, 0.01), ("LCB", _lib.GP_ACQ_LCB, 2.0), ("MPI", _lib.GP_ACQ_MPI, 0.01))
ROWS = (1, 3, 4, 5, 8)
SET5 = (2, 0, 1, 3, 4)        # members 2, 0, 1, then the rescaled 0 and 1


@functools.lru_cache(maxsize=None)
def member_params(cid):
    """(variance [5], lengthscale [5, nls], noise [5]) indexed by member id: 0..2 of FS.members, 3 = member 0 rescaled, 4 = member 1."""
    var, ls, noise = FS.members(cid)
    var = np.r_[var, var[0] * 1.7, var[1] * 0.6]
    ls = np.vstack([ls, ls[0] * 0.8, ls[1] * 1.25])
    noise = np.r_[noise, noise[0] * 3.0, noise[1] * 0.5]
    return FS.freeze(FS.namespace(var=var, ls=ls, noise=noise))


def member_set(cid, ids):
    p = member_params(cid)
    ids = list(ids)
    return p.var[ids].copy(), p.ls[ids].copy(), p.noise[ids].copy()


@functools.lru_cache(maxsize=None)
def points(cid):
    """Eight locations: the case's first candidates (row 0 ON a training point), points next to training points, a diagonal."""
    c = FS.CASES[cid]
    X, _, Xs, _ = FS.problem(cid)
    pool = np.vstack([Xs[:5], X[:3] + 0.013, X[:3] - 0.02, c.off + np.linspace(0.05, 0.95, 8)[:, None] * np.ones((1, c.D))])[:8]
    pool.setflags(write=False)
    return pool


@functools.lru_cache(maxsize=None)
def _oracle_gp(fam, cid, member, direct):
    if member < 3:
        return FS.oracle(fam, cid, member, direct)
    c, p = FS.CASES[cid], member_params(cid)
    X, Y, _, _ = FS.problem(cid)
    return O.OracleGP(X, Y, KF.make(fam, c.D, p.var[member], p.ls[member], c.ard, direct=direct), p.noise[member])


@functools.lru_cache(maxsize=None)
def ref(fam, cid, member, direct):
    """The oracle's posterior of one member at the eight points, and its fmin; computed once, read-only."""
    gp, x = _oracle_gp(fam, cid, member, direct), points(cid)
    mu, var1 = gp.predict(x)
    _, var0 = gp.predict_noiseless(x)
    dm, dv = gp.predictive_gradients(x)
    fmin = float(gp.predict(gp.X)[0].min())
    return FS.freeze(FS.namespace(mu=mu[:, 0].copy(), var=(var0[:, 0].copy(), var1[:, 0].copy()), dm=dm[:, :, 0].copy(), dv=dv.copy(), fmin=fmin))


def integrated(name, par, fmins, mus, variances, dms, dvs):
    """The mean over members of acquisitions._Rule, negated: (value [k], gradient [k, D]) in float64 NumPy."""
    rule, total, dtotal = _RULES[name], 0.0, 0.0
    for fmin, mu, var, dm, dv in zip(fmins, mus, variances, dms, dvs):
        sd = np.sqrt(np.maximum(var, 1e-10))[:, None]
        val, dval = rule.gradient(par, fmin, mu[:, None], sd.copy(), dm, dv / (2 * sd))
        total, dtotal = total + val, dtotal + dval
    return -(total / len(mus))[:, 0], -dtotal / len(mus)


def truth(what, dev, direct, gram):
    """One quantity against the oracle under the rule of the module docstring."""
    dev, direct, gram = np.asarray(dev, dtype=float), np.asarray(direct, dtype=float), np.asarray(gram, dtype=float)
    scale = max(float(np.max(np.abs(direct))), 1e-300)
    err, scatter = float(np.max(np.abs(dev - direct))), float(np.max(np.abs(gram - direct)))
    bound = max(MULT * scatter, FLOOR * scale)
    print("TRUTH %-44s scale %.3e  device %.3e  oracle %.3e  ratio %7.2f  bound %.3e" % (what, scale, err, scatter, err / max(scatter, 1e-300), bound))
    return err <= bound, what


def relative(tag, what, got, want, tol):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    scale = max(float(np.max(np.abs(want))), 1e-300)
    rel = float(np.max(np.abs(got - want))) / scale
    print("%s %-58s scale %.3e  rel %.3e  tol %.0e" % (tag, what, scale, rel, tol))
    return rel <= tol, what


def failed(results):
    return [w for ok, w in results if not ok]


@pytest.fixture(scope="module")
def h():
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", 0)
    yield hd
    hd.close()


def _ens(h, fam, cid, ids):
    c = FS.CASES[cid]
    X, Y, _, ls = FS.problem(cid)
    h.set_data(X, Y)
    h.set_params(FS.KERNEL_ID[fam], int(c.ard), FS.VAR, ls, FS.NOISE)
    return h.ens_fit(*member_set(cid, ids))


# ---- 1. per-member posterior and fmin against the member's oracle ----------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", PAIRS)
def test_member_posteriors_against_the_oracle(h, fam, cid):
    res, x = [], points(cid)
    for tag, ids in (("set3", (0, 1, 2)), ("set5", SET5)):
        lml, logdet, jit, fmin = _ens(h, fam, cid, ids)
        assert h.ens_info() == len(ids) and np.all(jit == 0.0)
        rd, rg = [ref(fam, cid, m, True) for m in ids], [ref(fam, cid, m, False) for m in ids]
        res.append(truth("%s %s %s: fmin" % (fam, cid, tag), fmin, [r.fmin for r in rd], [r.fmin for r in rg]))
        for k in ROWS:
            for noise in (1, 0):
                mu, var, dm, dv = h.ens_predict_rows(x[:k], bool(noise), grad=True)
                mu2, var2 = h.ens_predict_rows(x[:k], bool(noise))
                assert np.array_equal(mu, mu2)          # the value call's mean is the gradient call's (its variance sums w^2 in another order)
                name = "%s %s %s: %d rows noise=%d " % (fam, cid, tag, k, noise)
                res.append(truth(name + "mean", mu, [r.mu[:k] for r in rd], [r.mu[:k] for r in rg]))
                res.append(truth(name + "var", var, [r.var[noise][:k] for r in rd], [r.var[noise][:k] for r in rg]))
                res.append(truth(name + "var (value call)", var2, [r.var[noise][:k] for r in rd], [r.var[noise][:k] for r in rg]))
                res.append(truth(name + "dmdx", dm, [r.dm[:k] for r in rd], [r.dm[:k] for r in rg]))
                res.append(truth(name + "dvdx", dv, [r.dv[:k] for r in rd], [r.dv[:k] for r in rg]))
    assert not failed(res), failed(res)


# ---- 2. the integrated value and gradient against NumPy ------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", PAIRS)
def test_integrated_acquisition_against_numpy(h, fam, cid):
    res, x = [], points(cid)
    for tag, ids in (("set3", (0, 1, 2)), ("set5", SET5)):
        _, _, _, fmin = _ens(h, fam, cid, ids)
        rd, rg = [ref(fam, cid, m, True) for m in ids], [ref(fam, cid, m, False) for m in ids]
        for k in (1, 4, 8):
            mu, var, dm, dv = h.ens_predict_rows(x[:k], True, grad=True)
            for name, t, par in ACQS:
                got, dgot = h.ens_acq_rows(x[:k], t, par, grad=True)
                want = [integrated(name, par, [r.fmin for r in rr], [r.mu[:k] for r in rr], [r.var[1][:k] for r in rr],
                                   [r.dm[:k] for r in rr], [r.dv[:k] for r in rr]) for rr in (rd, rg)]
                what = "%s %s %s: %d rows %s " % (fam, cid, tag, k, name)
                res.append(truth(what + "value", got[:, 0], want[0][0], want[1][0]))
                res.append(truth(what + "gradient", dgot, want[0][1], want[1][1]))
                # the rule's arithmetic alone: the device's own posteriors through NumPy
                own = integrated(name, par, fmin, mu, var, dm, dv)
                res.append(relative("RULE", what + "value", got[:, 0], own[0], RULE_TOL))
                res.append(relative("RULE", what + "gradient", dgot, own[1], RULE_TOL))
    assert not failed(res), failed(res)


# ---- 3. rows against table; arg-best -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", PAIRS)
def test_table_against_rows_and_argbest(h, fam, cid):
    res, x = [], points(cid)
    _, _, Xs, _ = FS.problem(cid)
    _ens(h, fam, cid, SET5)
    base = np.vstack([x, Xs])
    for name, t, par in ACQS:
        h.set_candidates(base)
        s0 = h.ens_acq(t, par)[:, 0]
        # the best row of either sense once more at the end: a tie, which goes to the lowest index
        tab = np.vstack([base, base[int(np.argmin(s0))], base[int(np.argmax(s0))]])
        h.set_candidates(tab)
        s = h.ens_acq(t, par)[:, 0]
        assert np.array_equal(s, h.ens_acq(t, par)[:, 0])                         # bitwise repeatable
        assert np.array_equal(s[:len(s0)], s0)                                    # a row's score does not depend on the rows after it
        print("%s %s %s: duplicated rows tie: %s %s" % (fam, cid, name, s[-2] == s[int(np.argmin(s0))], s[-1] == s[int(np.argmax(s0))]))
        for sense in (-1, 1):
            want = int(np.argmin(s) if sense < 0 else np.argmax(s))
            got = h.ens_acq_argbest(t, par, sense)
            print("%s %s %s sense %+d: %s, want row %d of %d" % (fam, cid, name, sense, got, want, len(s)))
            assert got == (want, s[want]) and want < len(s0)
        rows = h.ens_acq_rows(tab[:8], t, par)[:, 0]
        res.append(relative("ROWS-TABLE", "%s %s: %s 8 rows" % (fam, cid, name), s[:8], rows, TABLE_TOL))
        rows = h.ens_acq_rows(Xs[:3], t, par)[:, 0]
        res.append(relative("ROWS-TABLE", "%s %s: %s candidates" % (fam, cid, name), s[8:8 + len(rows)], rows, TABLE_TOL))
    assert not failed(res), failed(res)


# ---- 4. properties (b) and (c) on bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", [pytest.param("rbf", "j"), pytest.param("Mat32", "a"), pytest.param("Mat52", "c"),
                                     pytest.param("Exponential", "f"), pytest.param("Mat32", "h"), pytest.param("Exponential", "b")])
def test_bits_do_not_depend_on_size_position_or_company(h, fam, cid):
    c, x = FS.CASES[cid], points(cid)
    _ens(h, fam, cid, (0, 1, 2))
    p3 = h.ens_predict_rows(x, True, grad=True)
    f3 = h.ens_fit(*member_set(cid, (0, 1, 2)))
    _ens(h, fam, cid, SET5)
    f5 = h.ens_fit(*member_set(cid, SET5))
    p5 = h.ens_predict_rows(x, True, grad=True)
    for z3, z5 in ((0, 1), (1, 2), (2, 0)):                     # member z3 of the three sits at z5 of the five
        assert all(np.array_equal(a[z3], b[z5]) for a, b in zip(p3, p5))
        assert all(a[z3] == b[z5] for a, b in zip(f3, f5))      # lml, log det, jitter, fmin
    for k in (1, 3, 4, 5):                                      # the company: x[:k] alone, and x[k - 1] alone
        pk = h.ens_predict_rows(x[:k], True, grad=True)
        p1 = h.ens_predict_rows(x[k - 1:k], True, grad=True)
        assert all(np.array_equal(a, b[:, :k]) for a, b in zip(pk, p5))
        assert all(np.array_equal(a[:, 0], b[:, k - 1]) for a, b in zip(p1, p5))
    for name, t, par in ACQS:                                   # (c): the same call, the same bits
        a, da = h.ens_acq_rows(x, t, par, grad=True)
        b, db = h.ens_acq_rows(x, t, par, grad=True)
        assert np.array_equal(a, b) and np.array_equal(da, db)
        a1 = h.ens_acq_rows(x[2:3], t, par, grad=True)
        assert np.array_equal(a1[0][0], a[2]) and np.array_equal(a1[1][0], da[2])
    # a one-member ensemble against the single model's entries on a context set to that member: the kernels share their bodies
    # (csrc/rows_body.h), so the comparison is bit equality
    p = member_params(cid)
    for m in (0, 4):
        h.ens_fit(p.var[[m]], p.ls[[m]], p.noise[[m]])
        h.set_params(FS.KERNEL_ID[fam], int(c.ard), p.var[m], p.ls[m], p.noise[m])
        h.fit()
        for k in [k for k in (1, 3, 4, 8) if FS.rows_fused(k, c.D)]:      # (beyond that the single model leaves its fused kernels)
            e = h.ens_predict_rows(x[:k], True, grad=True)
            s = h.predict_rows(x[:k], True, grad=True)
            assert np.array_equal(e[0][0], s[0][:, 0]) and np.array_equal(e[1][0], s[1][:, 0])
            assert np.array_equal(e[2][0], s[2][:, :, 0]) and np.array_equal(e[3][0], s[3])
            e0, s0 = h.ens_predict_rows(x[:k], False), h.predict_rows(x[:k], False)
            assert np.array_equal(e0[0][0], s0[0][:, 0]) and np.array_equal(e0[1][0], s0[1][:, 0])
            for name, t, par in ACQS:
                ea, eda = h.ens_acq_rows(x[:k], t, par, grad=True)
                sa, sda = h.acq_rows(x[:k], t, par, h.fmin(), grad=True)
                assert np.array_equal(ea, sa) and np.array_equal(eda, sda), (name, k)
                assert np.array_equal(h.ens_acq_rows(x[:k], t, par), h.acq_rows(x[:k], t, par, h.fmin()))


# ---- 5. state and errors -------------------------------------------------------------------------------------------------------------
def _raw_fit(h, S, var, ls, noise, null=None):
    var, ls, noise = (np.ascontiguousarray(a, dtype=float) for a in (var, ls, noise))
    args = [_lib.dptr(var), _lib.dptr(ls), _lib.dptr(noise)]
    if null is not None:
        args[null] = None
    return h.lib.gp_ens_fit(h.h, int(S), args[0], args[1], args[2], 5, None, None, None, None)


def test_refusals():
    hd = _lib.Handle(0)
    try:
        c = FS.CASES["c"]
        X, Y, Xs, ls = FS.problem("c")
        var, lss, noise = member_set("c", (0, 1, 2))
        out = np.empty((8, 1))
        # before data, before parameters
        assert _raw_fit(hd, 3, var, lss, noise) == _lib.GP_ERR_STATE
        hd.set_data(X, Y)
        assert _raw_fit(hd, 3, var, lss, noise) == _lib.GP_ERR_STATE
        assert hd.ens_info() == 0
        # a scoring call before a valid fit
        x8 = np.ascontiguousarray(points("c"))
        assert hd.lib.gp_ens_acq_rows(hd.h, x8.ctypes.data, 8, 0, 0.01, out.ctypes.data, None) == _lib.GP_ERR_STATE
        assert hd.lib.gp_ens_predict_rows(hd.h, x8.ctypes.data, 8, 1, out.ctypes.data, None, None, None) == _lib.GP_ERR_STATE
        assert hd.lib.gp_ens_acq(hd.h, 0, 0.01, _lib.dptr(out)) == _lib.GP_ERR_STATE
        idx, val = ctypes.c_int64(), ctypes.c_double()
        assert hd.lib.gp_ens_acq_argbest(hd.h, 0, 0.01, 1, ctypes.byref(idx), ctypes.byref(val)) == _lib.GP_ERR_STATE
        hd.set_params(2, 1, FS.VAR, ls, FS.NOISE)
        # S outside 1 .. 64
        assert _raw_fit(hd, 0, var, lss, noise) == _lib.GP_ERR_ARG
        big = np.ones(65)
        assert _raw_fit(hd, 65, big, np.ones((65, c.D)), big) == _lib.GP_ERR_ARG
        # null pointers
        for k in range(3):
            assert _raw_fit(hd, 3, var, lss, noise, null=k) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_fit(None, 3, _lib.dptr(var), _lib.dptr(lss), _lib.dptr(noise), 5, None, None, None, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_info(hd.h, None) == _lib.GP_ERR_ARG
        # non-positive parameters
        assert _raw_fit(hd, 3, var * np.array([1, -1, 1]), lss, noise) == _lib.GP_ERR_ARG
        # the Gower option, an output warp: state
        hd.set_params(0, 1, FS.VAR, ls, FS.NOISE)
        hd.set_gower(np.zeros(c.D, dtype=np.int32), np.ones(c.D))
        assert _raw_fit(hd, 3, var, lss, noise) == _lib.GP_ERR_STATE
        hd.set_gower()
        hd.set_output_warp(np.array([[0.5, 1.0, 0.0]]), 1.0)
        assert _raw_fit(hd, 3, var, lss, noise) == _lib.GP_ERR_STATE
        hd.set_output_warp(None)
        hd.set_data(X, Y)
        hd.set_params(2, 1, FS.VAR, ls, FS.NOISE)
        # a valid ensemble, then the argument checks of the scoring entries
        hd.ens_fit(var, lss, noise)
        assert hd.ens_info() == 3
        assert hd.lib.gp_ens_acq_rows(hd.h, None, 8, 0, 0.01, out.ctypes.data, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_acq_rows(hd.h, x8.ctypes.data, 8, 0, 0.01, None, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_acq_rows(hd.h, x8.ctypes.data, 9, 0, 0.01, out.ctypes.data, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_acq_rows(hd.h, x8.ctypes.data, 0, 0, 0.01, out.ctypes.data, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_acq_rows(hd.h, x8.ctypes.data, 8, 3, 0.01, out.ctypes.data, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_predict_rows(hd.h, None, 8, 1, out.ctypes.data, None, None, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_predict_rows(hd.h, x8.ctypes.data, 9, 1, None, None, None, None) == _lib.GP_ERR_ARG
        g = np.empty((3, 8, c.D))
        assert hd.lib.gp_ens_predict_rows(hd.h, x8.ctypes.data, 8, 1, None, None, g.ctypes.data, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_acq(hd.h, 0, 0.01, None) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_acq(hd.h, 0, 0.01, _lib.dptr(out)) == _lib.GP_ERR_STATE          # no candidate table yet
        hd.set_candidates(Xs)
        assert hd.lib.gp_ens_acq_argbest(hd.h, 0, 0.01, 0, ctypes.byref(idx), ctypes.byref(val)) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_acq_argbest(hd.h, 0, 0.01, 1, None, ctypes.byref(val)) == _lib.GP_ERR_ARG
        assert hd.lib.gp_ens_acq_argbest(hd.h, 7, 0.01, 1, ctypes.byref(idx), ctypes.byref(val)) == _lib.GP_ERR_ARG
        # a failed fit leaves no ensemble: one member with a NaN-free but unfactorable matrix is covered by the jitter test;
        # here: a refused call after a valid one keeps the valid one (the refusal comes before anything is touched)
        assert _raw_fit(hd, 0, var, lss, noise) == _lib.GP_ERR_ARG and hd.ens_info() == 3
        # P != 1
        hd.set_data(X, np.hstack([Y, Y]))
        hd.set_params(2, 1, FS.VAR, ls, FS.NOISE)
        assert _raw_fit(hd, 3, var, lss, noise) == _lib.GP_ERR_ARG
        # case i: N = 2944 pads beyond the batched fit's cap -- refused after gp_set_data alone, on a context that never saw
        # parameters (no fit of that size is made)
        Xi, Yi, _, li0 = FS.problem("i")
        vi, li, ni = FS.members("i")
        h2 = _lib.Handle(0)
        try:
            h2.set_data(Xi, Yi)
            assert _raw_fit(h2, 3, vi, li, ni) == _lib.GP_ERR_ARG
            h2.set_params(2, 1, FS.VAR, li0, FS.NOISE)
            with pytest.raises(ValueError):
                h2.ens_fit(vi, li, ni)
            assert h2.ens_info() == 0
        finally:
            h2.close()
    finally:
        hd.close()


def test_lifetime_beside_the_contexts_own_fit(h):
    fam, cid = "Mat52", "c"
    c, x = FS.CASES[cid], points(cid)
    X, Y, Xs, ls = FS.problem(cid)
    h.set_data(X, Y)
    h.set_params(FS.KERNEL_ID[fam], int(c.ard), FS.VAR, ls, FS.NOISE)
    fit0 = h.fit()
    h.set_candidates(Xs)
    own0 = h.predict_rows(x[:4], True, grad=True)
    tab0 = h.predict(True)
    h.ens_fit(*member_set(cid, SET5))
    # the context's fit, parameters and candidate table are as they were: no refit happens here
    assert h.fit_state() == tuple(fit0)
    own1 = h.predict_rows(x[:4], True, grad=True)
    assert all(np.array_equal(a, b) for a, b in zip(own0, own1))
    assert all(np.array_equal(a, b) for a, b in zip(tab0, h.predict(True)))
    e0 = h.ens_predict_rows(x, True, grad=True)
    a0 = h.ens_acq_rows(x, 0, 0.01, grad=True)
    # the ensemble survives gp_set_params, gp_fit and gp_set_candidates on the context
    h.set_params(0, 0, 0.7, np.array([0.9]), 0.05)
    assert h.ens_info() == 5
    assert all(np.array_equal(a, b) for a, b in zip(e0, h.ens_predict_rows(x, True, grad=True)))
    h.fit()
    h.set_candidates(x)
    assert all(np.array_equal(a, b) for a, b in zip(a0, h.ens_acq_rows(x, 0, 0.01, grad=True)))
    assert all(np.array_equal(a, b) for a, b in zip(e0, h.ens_predict_rows(x, True, grad=True)))
    # gp_set_data drops it
    h.set_data(X, Y)
    assert h.ens_info() == 0
    with pytest.raises(RuntimeError):
        h.ens_acq_rows(x, 0, 0.01)


def test_jitter_ladder_per_member(h):
    """The set-up of tests/test_gpu_fit_grad_batch.py::test_jitter_per_member: duplicated rows, members with a huge variance and no
    noise need the ladder, the others must keep jitter 0 -- and the whole call fails when the ladder is not allowed."""
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, (120, 2))
    Y = (np.sin(2 * np.pi * X).sum(1) / np.sqrt(2) + 0.1 * rng.standard_normal(120))[:, None]
    X, Y = np.vstack([X, X[:40]]), np.vstack([Y, Y[:40]])
    h.set_data(X, Y)
    var = np.array([1.0, 1e8, 1.0, 1e7])
    ls = np.array([[0.3], [2.0], [0.3], [1.5]])
    noise = np.array([1e-2, 1e-12, 1e-3, 1e-12])
    h.set_params(0, False, var[0], ls[0], noise[0])
    lml, logdet, jit, fmin = h.ens_fit(var, ls, noise)
    print("jitter per member:", jit)
    (_, _, jref), _, st = h.fit_grad_batch(var, ls, noise)
    assert not st.any() and np.array_equal(jit, jref)              # the same rung as the batched fit
    assert np.all(jit[[0, 2]] == 0.0) and np.all(jit[[1, 3]] > 0.0)
    mu, v = h.ens_predict_rows(X[:4] + 0.01, True)
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(v)) and np.all(np.isfinite(fmin))
    # members 0 and 2 are what they are alone
    solo = h.ens_fit(var[[0, 2]], ls[[0, 2]], noise[[0, 2]])
    mu2, v2 = h.ens_predict_rows(X[:4] + 0.01, True)
    assert np.array_equal(mu2, mu[[0, 2]]) and np.array_equal(v2, v[[0, 2]]) and np.array_equal(solo[3], fmin[[0, 2]])
    with pytest.raises(np.linalg.LinAlgError):
        h.ens_fit(var, ls, noise, maxtries=0)
    assert h.ens_info() == 0                                         # the failed call left no ensemble


def test_exhausted_ladder_is_the_single_fits_code_and_message(h):
    """A member that exhausts the ladder, over three tiles (tests/_jitter_cases.py, N = 300: members 0 and 2 of the batched case
    around its member 6, whose first non-positive pivot lies among the repeated rows of the third tile).  With the ladder the
    member stops on the first rung and its neighbours keep jitter 0; with maxtries = 0 gp_ens_fit returns the code gp_fit_grad
    returns for that member alone, with the library's message for it, and gp_ens_info reports no ensemble."""
    import _jitter_cases as J
    X, Y = J.batch_problem()
    h.set_data(X, Y)
    pick = [0, 6, 2]
    var, ls, noise = J.BATCH_VAR[pick], J.BATCH_LS[pick], J.BATCH_NOISE[pick]
    h.set_params(0, False, var[1], ls[1], noise[1])
    lml, logdet, jt = _lib._fit_scalars()
    dv, dn, dl = ctypes.c_double(), ctypes.c_double(), np.empty(1)
    alone = h.lib.gp_fit_grad(h.h, 0, ctypes.byref(lml), ctypes.byref(logdet), ctypes.byref(jt), ctypes.byref(dv), _lib.dptr(dl),
                              ctypes.byref(dn))
    h.set_params(0, False, var[0], ls[0], noise[0])
    jit = h.ens_fit(var, ls, noise)[2]
    print("jitter per member:", jit, "gp_fit_grad alone without the ladder:", alone)
    assert h.ens_info() == 3 and jit[0] == 0.0 and jit[2] == 0.0
    assert jit[1] == pytest.approx((var[1] + (noise[1] + 1e-8)) * 1e-6, rel=1e-12)
    out = [np.empty(3) for _ in range(4)]
    rc = h.lib.gp_ens_fit(h.h, 3, _lib.dptr(var), _lib.dptr(ls), _lib.dptr(noise), 0, *[_lib.dptr(o) for o in out])
    msg = h.lib.gp_last_error().decode()
    print("gp_ens_fit without the ladder:", rc, repr(msg))
    assert rc == alone and J.BATCH_N - J.BATCH_DUP < rc <= J.BATCH_N
    assert msg == "not positive definite, even with jitter."
    assert h.ens_info() == 0


# ---- 6. the model level --------------------------------------------------------------------------------------------------------------
def _objective(x):
    x = np.atleast_2d(x)
    return (np.sin(5 * x[:, 0]) + (x[:, 1] - 0.4) ** 2)[:, None]


@pytest.fixture(scope="module")
def mcmc_model():
    rng = np.random.RandomState(2)
    X = rng.uniform(0, 1, (30, 2))
    Y = _objective(X) + 0.05 * rng.standard_normal((30, 1))
    np.random.seed(7)
    mm = gpo.GPModel_MCMC(n_samples=3, n_burnin=5, subsample_interval=2, leapfrog_steps=3)
    mm.updateModel(X, Y, None, None)
    return mm, X, Y


def test_model_predictions_against_the_oracle(mcmc_model):
    mm, X, Y = mcmc_model
    assert mm.hmc_samples.shape == (3, 3) and np.all(mm.hmc_samples > 0) and mm.model._h.ens_info() == 3
    Xs = np.random.RandomState(3).uniform(0, 1, (11, 2))
    means, stds, dms, dss = mm.predict_withGradients(Xs)
    m2, s2 = mm.predict(Xs)
    fmins = mm.get_fmin()
    res = []
    for z, s in enumerate(mm.hmc_samples):
        gm = O.OracleGPModel(O.OracleGP(X, Y, O.make_kernel("rbf", 2, s[0], s[1:2], ARD=False), s[2]))
        mu, sd, dm, ds = gm.predict_withGradients(Xs)
        for what, got, want in (("mean", means[z], mu), ("std", stds[z], sd), ("dmdx", dms[z], dm), ("dsdx", dss[z], ds),
                                ("predict mean", m2[z], mu), ("predict std", s2[z], sd), ("fmin", fmins[z], gm.get_fmin())):
            res.append(relative("MODEL", "sample %d %s" % (z, what), got, want, 1e-6))
    assert not failed(res), failed(res)


@pytest.mark.parametrize("cls,kw", [(gpo.AcquisitionEI_MCMC, dict(jitter=0.01)), (gpo.AcquisitionMPI_MCMC, dict(jitter=0.01)),
                                    (gpo.AcquisitionLCB_MCMC, dict(exploration_weight=2))])
def test_acquisition_classes_on_the_device_route(mcmc_model, cls, kw):
    mm = mcmc_model[0]
    acq = cls(mm, **kw)
    assert acq._ens_ok() and acq.analytical_gradient_acq
    Xs = np.random.RandomState(4).uniform(0, 1, (11, 2))
    res = []
    for k in (1, 8, 11):
        x = Xs[:k]
        want, dwant = acq._compute_acq_withGradients(x)            # the reference's formulas over the model's lists
        val = acq.acquisition_function(x)
        val2, dval = acq.acquisition_function_withGradients(x)
        assert val.shape == (k, 1) and dval.shape == (k, 2)
        res.append(relative("MODEL", "%s %d rows value" % (cls.__name__, k), val, -want, RULE_TOL if k <= 8 else TABLE_TOL))
        res.append(relative("MODEL", "%s %d rows value (gradient call)" % (cls.__name__, k), val2, -want, RULE_TOL))
        res.append(relative("MODEL", "%s %d rows gradient" % (cls.__name__, k), dval, -dwant, RULE_TOL))
    i, v = acq.argbest(Xs, -1)
    scores = acq.acquisition_function(Xs)[:, 0]
    assert (i, v) == (int(np.argmin(scores)), scores[int(np.argmin(scores))])
    assert not failed(res), failed(res)


def test_bayesian_optimization_front_door():
    domain = [{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}]
    np.random.seed(3)
    mm = gpo.GPModel_MCMC(n_samples=3, n_burnin=5, subsample_interval=2, leapfrog_steps=3)
    bo = gpo.BayesianOptimization(_objective, domain, model=mm, acquisition_type='EI_MCMC', initial_design_numdata=8)
    x_opt, fx = bo.run_optimization(max_iter=2)
    print("points:", bo.X[-2:].tolist(), "best", x_opt, fx)
    assert bo.X.shape == (10, 2) and np.all(np.isfinite(bo.X)) and np.all((bo.X >= 0) & (bo.X <= 1)) and np.isfinite(fx)
    assert isinstance(bo.acquisition, gpo.AcquisitionEI_MCMC) and bo.acquisition._ens_ok()
