"""GPU: the ensemble entry points at the sizes their code branches on, against the exact GP in long double.

tests/test_gpu_ensemble.py runs N <= 300, S <= 5 and tables of at most 140 rows.  The cases here (tests/_ens_truth.py, TABLE; their
reach is asserted on the CPU by tests/test_ens_truth_host.py):
  p  770 x 3   Mat32 ARD        S = 3   7 tiles: two factorisation panels (gp_ens_fit: factor_buf, panel_inv_members, solve_rows)
  q  1024 x 2  rbf iso          S = 3   8 tiles: the last size with one 1024-column chunk in the one-location passes
  r  1025 x 5  Exponential ARD  S = 3   9 tiles: rw_nch = nmean = 2, one live column in the second chunk (ens_rows_table strides)
  s  2048 x 3  Mat52 iso        S = 2   GP_ENS_MAX_NPAD: 16 tiles, panels 6 + 6 + 4, a full second chunk
  t  130 x 2   rbf ARD          S = 64  GP_ENS_MAX_S: the last slot of the noise / fmin table and of the arrival counters
  u  300 x 64  Mat32, rbf ARD   S = 3   GP_MAX_D: two locations per pass
  v  160 x 2   rbf iso          S = 4   two members on the jitter ladder next to two that are not
and tables of 512, 513 and 1100 rows (GP_ENS_TABLE_CHUNK = 512: one pass, a second pass of one row, 512 + 512 + 76).

Reference: ``_ens_truth.truth`` -- Cholesky, solves, covariances and their derivatives in np.longdouble (eps 1.1e-19).  Bound of
every comparison against it:  err <= max(MULT x e64, FLOOR_N x scale), where e64 is the error of the float64 direct-distance oracle
(``OracleGP``) against the same truth for that quantity (capped on the CPU at 1e-9 x scale, 1e-6 for the jittered members, so the
bound is never loose), scale the largest truth entry, MULT = 64 the project's figure (profiles/ens_errors.txt) and
FLOOR_N = 1e-13 max(1, Npad / 384): 1e-13 is the project's floor, measured at Npad <= 384, and beyond that size the length of every
contraction, and with it at worst the rounding of its sum, grows linearly with Npad (derived, not measured).  In case v the
members on the ladder and those off it are compared apart (their scales lie 1e8 apart), the truth built with the jitter the device
reports.
Posteriors and fmin keep MULT = 64 (measured on an MI355X: worst ratio above the floor 4.58, rbf q: 1 rows dmdx).  The integrated
acquisitions (rows and table) take MULT_ACQ = 128, profiles/ens_errors.txt's own rule -- 4 x the worst ratio above the floor,
rounded up to a power of two -- on their worst, 18.26 (Mat52 s: 4 rows EI value, scale 4.7e-18), and for a reason in the code's
arithmetic, not in its size: that call's four locations all lie far above fmin and its value is member 1 at row 3, u = (fmin - m -
jitter) / s = -8.04, EI = 9.4e-18.  There EI = s (u Phi + phi) cancels to phi / u^2, and an error dm of the mean shows as
Phi(u) dm / EI = 47.5 dm of the value.  The device's mean of that call is 2.3e-13 off at worst (bound: the floor, 5.2e-13), and
the 8.7e-30 = 1.8e-12 of the EI it is off is the mean of that row, measured 3.9e-14 off (first order, Phi(u) (dfmin - dm) / 2:
7.4e-30).  An error ten times under the posterior's own floor, which the rule lets through, lands above the EI's floor, which
does not pass through the factor 47.5, and is then measured against what the float64 oracle happens to lose at that one row
(7e-15).  Case h of tests/test_gpu_ensemble.py documents the same for a scale of 1.9e-13.
RULE_TOL and TABLE_TOL are tests/test_gpu_ensemble.py's 1e-12 (measured here: 3.2e-13, Mat32 p: 1 rows EI value at a scale of
1.2e-31, and 1.4e-13, Mat52 s: EI 8 rows; the first leaves a factor 3.1, not 4).  Every figure is printed before it is asserted,
in that module's TRUTH / RULE / ROWS-TABLE formats (a TRUTH line here carries its floor as well); tools/ens_errors.py collects them into
profiles/ens_errors.txt.  The module prints its wall time: the host-side truth dominates (two long-double factorisations of
2048 x 2048 for case s), computed once per (case, member) and shared.
"""
import time

import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib

import _ens_truth as ET
import _family_shapes as FS
from test_gpu_ensemble import ACQS, RULE_TOL, TABLE_TOL, failed, integrated, relative

pytestmark = pytest.mark.gpu

MULT, MULT_ACQ = ET.MULT, 128.0
ROWS = (1, 4, 5, 8)
PAIRS = [pytest.param(f, c, id="%s-%s" % (f, c)) for f, c in ET.PAIRS]
T_FIVE = (0, 1, 2, 3, 4)


def truth(what, dev, oracle, true, N, mult=MULT):
    """One quantity against the long-double truth under the rule of the module docstring."""
    true = np.asarray(true, dtype=ET.T)
    e64, scale = ET.e64_of(oracle, true)
    err = float(np.max(np.abs(np.asarray(dev, dtype=ET.T) - true)))
    floor = ET.floor_n(N) * scale
    bound = max(mult * e64, floor)
    print("TRUTH %-44s scale %.3e  device %.3e  oracle %.3e  ratio %7.2f  bound %.3e  floor %.3e"
          % (what, scale, err, e64, err / max(e64, 1e-300), bound, floor))
    return err <= bound, what


def stack(records, field, k, index=None):
    """[S, k, ...] of a field of the members' records (``index``: which of the two variances)."""
    return np.stack([(getattr(r, field) if index is None else getattr(r, field)[index])[:k] for r in records])


def both(fam, cid, ids, jitters=None):
    jitters = [0.0] * len(ids) if jitters is None else jitters
    return ([ET.truth(fam, cid, z, j) for z, j in zip(ids, jitters)], [ET.oracle64(fam, cid, z, j) for z, j in zip(ids, jitters)])


def integrated_over(records, name, par, k):
    return integrated(name, par, [float(r.fmin) for r in records], [r.mu[:k] for r in records], [r.var[1][:k] for r in records],
                      [r.dm[:k] for r in records], [r.dv[:k] for r in records])


def table_scores(name, par, fmins, mus, variances):
    zero = np.zeros((len(mus[0]), 1))
    return integrated(name, par, fmins, mus, variances, [zero] * len(mus), [zero] * len(mus))[0]


def table_truth(fam, cid, ids, M, name, par):
    """(the truth's integrated value, the float64 oracle's) over the case's M-row table; fmin from the members' records."""
    tr, orc = both(fam, cid, ids)
    tt, ot = [ET.truth_table(fam, cid, z, M) for z in ids], [ET.oracle64_table(fam, cid, z, M) for z in ids]
    return (table_scores(name, par, [float(r.fmin) for r in tr], [m.astype(float) for m, _ in tt], [v.astype(float) for _, v in tt]),
            table_scores(name, par, [r.fmin for r in orc], [m for m, _ in ot], [v for _, v in ot]))


@pytest.fixture(scope="module")
def h():
    t0 = time.time()
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", 0)
    yield hd
    hd.close()
    print("\nSIZES wall time of tests/test_gpu_ensemble_sizes.py: %.1f s" % (time.time() - t0))


def fit(h, fam, cid, ids=None):
    c = ET.CASES[cid]
    X, Y, ls = ET.problem(cid)
    var, lss, noise = ET.members(cid)
    ids = list(range(c.S) if ids is None else ids)
    h.set_data(X, Y)
    h.set_params(FS.KERNEL_ID[fam], int(c.ard), FS.VAR, ls, FS.NOISE)
    return h.ens_fit(var[ids], lss[ids], noise[ids])


def member_checks(res, h, name, x, N, tr, orc, sel=slice(None)):
    """(a): mean, variance, dmdx, dvdx of the members ``sel`` (records tr, orc), with and without noise, gradient call and value
    call.  The members' arrays are compared stacked: one scale per call."""
    for k in ROWS:
        for noise in (1, 0):
            mu, var, dm, dv = h.ens_predict_rows(x[:k], bool(noise), grad=True)
            mu2, var2 = h.ens_predict_rows(x[:k], bool(noise))
            assert np.array_equal(mu, mu2)
            mu, var, dm, dv, var2 = (a[sel] for a in (mu, var, dm, dv, var2))
            what = "%s: %d rows noise=%d " % (name, k, noise)
            res.append(truth(what + "mean", mu, stack(orc, "mu", k), stack(tr, "mu", k), N))
            res.append(truth(what + "var", var, stack(orc, "var", k, noise), stack(tr, "var", k, noise), N))
            res.append(truth(what + "var (value call)", var2, stack(orc, "var", k, noise), stack(tr, "var", k, noise), N))
            res.append(truth(what + "dmdx", dm, stack(orc, "dm", k), stack(tr, "dm", k), N))
            res.append(truth(what + "dvdx", dv, stack(orc, "dv", k), stack(tr, "dv", k), N))


# ---- (a) per-member posterior and fmin against the truth ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", PAIRS)
def test_member_posteriors_against_the_truth(h, fam, cid):
    c, x, res = ET.CASES[cid], ET.points(cid), []
    lml, logdet, jit, fmin = fit(h, fam, cid)
    assert h.ens_info() == c.S and np.all(jit == 0.0)
    tr, orc = both(fam, cid, range(c.S))
    name = "%s %s S=%d" % (fam, cid, c.S)
    res.append(truth(name + ": fmin", fmin, [r.fmin for r in orc], [r.fmin for r in tr], c.N))
    member_checks(res, h, name, x, c.N, tr, orc)
    assert not failed(res), failed(res)


# ---- (b) the integrated value and gradient against the truth ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", PAIRS)
def test_integrated_acquisition_against_the_truth(h, fam, cid):
    c, x, res = ET.CASES[cid], ET.points(cid), []
    _, _, _, fmin = fit(h, fam, cid)
    tr, orc = both(fam, cid, range(c.S))
    tr = [ET.as64(r) for r in tr]
    for k in ROWS:
        mu, var, dm, dv = h.ens_predict_rows(x[:k], True, grad=True)
        for name, t, par in ACQS:
            got, dgot = h.ens_acq_rows(x[:k], t, par, grad=True)
            got2 = h.ens_acq_rows(x[:k], t, par)          # the value call sums w^2 in another order: held to the truth, not to bits
            want, orc_want = integrated_over(tr, name, par, k), integrated_over(orc, name, par, k)
            what = "%s %s S=%d: %d rows %s " % (fam, cid, c.S, k, name)
            res.append(truth(what + "value", got[:, 0], orc_want[0], want[0], c.N, MULT_ACQ))
            res.append(truth(what + "value (value call)", got2[:, 0], orc_want[0], want[0], c.N, MULT_ACQ))
            res.append(truth(what + "gradient", dgot, orc_want[1], want[1], c.N, MULT_ACQ))
            own = integrated(name, par, fmin, mu, var, dm, dv)                 # the rule's arithmetic alone
            res.append(relative("RULE", what + "value", got[:, 0], own[0], RULE_TOL))
            res.append(relative("RULE", what + "gradient", dgot, own[1], RULE_TOL))
    assert not failed(res), failed(res)


# ---- (c) the table route ---------------------------------------------------------------------------------------------------------------
def test_table_chunks_against_the_truth(h):
    """Case t, its first five members: 512 rows (one pass of the chunk loop), 513 (a second pass of one row), 1100 (512 + 512 + 76)."""
    fam, cid, res = "rbf", "t", []
    c = ET.CASES[cid]
    fit(h, fam, cid, T_FIVE)
    for name, t, par in ACQS:
        scores = {}
        for M in (512, 513, 1100):
            tab = ET.table(cid, M)
            h.set_candidates(tab)
            s = scores[M] = h.ens_acq(t, par)[:, 0]
            assert np.array_equal(s, h.ens_acq(t, par)[:, 0])                  # bitwise repeatable
            want, orc_want = table_truth(fam, cid, T_FIVE, M, name, par)
            res.append(truth("%s %s table of %d: %s" % (fam, cid, M, name), s, orc_want, want, c.N, MULT_ACQ))
            h.set_candidates(tab[::-1].copy())
            back = h.ens_acq(t, par)[::-1, 0]
            print("%s %s table of %d reversed: %s bitwise equal: %s" % (fam, cid, M, name, np.array_equal(back, s)))
            res.append(relative("ROWS-TABLE", "%s %s table of %d reversed: %s" % (fam, cid, M, name), back, s, TABLE_TOL))
        assert np.array_equal(scores[513][:512], scores[512])                  # a row's score does not depend on the passes after it
        # arg-best: the best row of either sense moved into the last chunk (rows 1024 ..), a plain row taking its place
        s = scores[1100]
        tab = np.array(ET.table(cid, 1100))
        moves = {int(np.argmin(s)): 1050, int(np.argmax(s)): 1090}
        for src, dst in moves.items():
            if src < 1024:
                tab[[src, dst]] = tab[[dst, src]]
        h.set_candidates(tab)
        s = h.ens_acq(t, par)[:, 0]
        for sense in (-1, 1):
            want = int(np.argmin(s) if sense < 0 else np.argmax(s))
            got = h.ens_acq_argbest(t, par, sense)
            print("%s %s %s sense %+d: %s, want row %d of %d" % (fam, cid, name, sense, got, want, len(s)))
            assert got == (want, s[want]) and want >= 1024
    assert not failed(res), failed(res)


@pytest.mark.parametrize("fam,cid", [pytest.param("Exponential", "r"), pytest.param("Mat52", "s")])
def test_table_beyond_one_chunk_of_columns(h, fam, cid):
    """A 140-row table at 9 and 16 tiles: its first 8 rows against gp_ens_acq_rows, all rows against the truth."""
    c, res = ET.CASES[cid], []
    fit(h, fam, cid)
    tab = ET.table(cid, 140)
    h.set_candidates(tab)
    for name, t, par in ACQS:
        s = h.ens_acq(t, par)[:, 0]
        rows = h.ens_acq_rows(tab[:8], t, par)[:, 0]
        res.append(relative("ROWS-TABLE", "%s %s: %s 8 rows" % (fam, cid, name), s[:8], rows, TABLE_TOL))
        want, orc_want = table_truth(fam, cid, range(c.S), 140, name, par)
        res.append(truth("%s %s table of 140: %s" % (fam, cid, name), s, orc_want, want, c.N, MULT_ACQ))
    assert not failed(res), failed(res)


# ---- (d) position, company and size on bits ----------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def test_bits_at_nine_tiles(h):
    """Case r: member z's posterior bits in an ensemble of 3, of those members permuted, and of 2."""
    fam, cid, x = "Exponential", "r", ET.points("r")
    f3 = fit(h, fam, cid, (0, 1, 2))
    p3 = h.ens_predict_rows(x, True, grad=True)
    fp = fit(h, fam, cid, (2, 0, 1))
    pp = h.ens_predict_rows(x, True, grad=True)
    f2 = fit(h, fam, cid, (1, 2))
    p2 = h.ens_predict_rows(x, True, grad=True)
    for z3, zp in ((0, 1), (1, 2), (2, 0)):
        assert _same([a[z3] for a in p3], [a[zp] for a in pp]) and all(a[z3] == b[zp] for a, b in zip(f3, fp))
    for z3, z2 in ((1, 0), (2, 1)):
        assert _same([a[z3] for a in p3], [a[z2] for a in p2]) and all(a[z3] == b[z2] for a, b in zip(f3, f2))


def test_bits_and_the_last_slot_at_64_members(h):
    """Case t: S = 64, then 1, then 64 again on one handle (the counters' reset in gp_ens_fit); members 63 and 0 alone; and the
    integrated value at S = 64 against the mean of the 64 posteriors (the last member's noise, fmin and counter slot)."""
    fam, cid, x, res = "rbf", "t", ET.points("t"), []
    f64 = fit(h, fam, cid)
    p64 = h.ens_predict_rows(x, True, grad=True)
    acq = {name: h.ens_acq_rows(x, t, par, grad=True) for name, t, par in ACQS}
    for name, t, par in ACQS:
        for k in ROWS:
            got, dgot = (acq[name][0][:k], acq[name][1][:k]) if k == 8 else h.ens_acq_rows(x[:k], t, par, grad=True)
            own = integrated(name, par, f64[3], *[a[:, :k] for a in p64])
            res.append(relative("RULE", "%s %s S=64 all members: %d rows %s value" % (fam, cid, k, name), got[:, 0], own[0], RULE_TOL))
            res.append(relative("RULE", "%s %s S=64 all members: %d rows %s gradient" % (fam, cid, k, name), dgot, own[1], RULE_TOL))
    f1 = fit(h, fam, cid, (7,))
    p1 = h.ens_predict_rows(x, True, grad=True)
    assert h.ens_info() == 1 and _same([a[0] for a in p1], [a[7] for a in p64]) and all(a[0] == b[7] for a, b in zip(f1, f64))
    again = fit(h, fam, cid)
    assert h.ens_info() == 64 and _same(again, f64)
    assert _same(h.ens_predict_rows(x, True, grad=True), p64)
    for name, t, par in ACQS:
        assert _same(h.ens_acq_rows(x, t, par, grad=True), acq[name])
    f2 = fit(h, fam, cid, (63, 0))
    p2 = h.ens_predict_rows(x, True, grad=True)
    for z64, z2 in ((63, 0), (0, 1)):
        assert _same([a[z64] for a in p64], [a[z2] for a in p2]) and all(a[z64] == b[z2] for a, b in zip(f64, f2))
    assert not failed(res), failed(res)


# ---- (e) members on the jitter ladder ----------------------------------------------------------------------------------------------------
def test_jittered_members_against_the_truth(h):
    """Case v: members 1 and 3 need the ladder (the CPU test holds the float64 oracle to at least one rung on them), 0 and 2 do
    not.  The rung is the batched fit's; posteriors and fmin of all four against the truth built with the jitter the device reports."""
    fam, cid, x, res = "rbf", "v", ET.points("v"), []
    c = ET.CASES[cid]
    var, ls, noise = ET.members(cid)
    lml, logdet, jit, fmin = fit(h, fam, cid)
    print("jitter per member:", jit)
    (_, _, jref), _, st = h.fit_grad_batch(var, ls, noise)
    assert not st.any() and np.array_equal(jit, jref)
    ill, well = list(ET.V_ILL), [z for z in range(c.S) if z not in ET.V_ILL]
    assert np.all(jit[ill] > 0.0) and np.all(jit[well] == 0.0)
    for tag, ids in (("on the ladder", ill), ("off the ladder", well)):      # apart: their scales are 1e8 apart
        tr, orc = both(fam, cid, ids, [float(jit[z]) for z in ids])
        name = "%s %s %s" % (fam, cid, tag)
        res.append(truth(name + ": fmin", fmin[ids], [r.fmin for r in orc], [r.fmin for r in tr], c.N))
        member_checks(res, h, name, x, c.N, tr, orc, ids)
    assert not failed(res), failed(res)


# ---- (f) refusal one row past the cap ----------------------------------------------------------------------------------------------------
def test_refusal_one_row_past_the_cap():
    """N = 2049 pads to 2176 > GP_ENS_MAX_NPAD: GP_ERR_ARG after gp_set_data alone, on a context that never saw parameters -- no
    fit of that size is made."""
    rng = np.random.default_rng(2049)
    X, Y = rng.uniform(0, 1, (2049, 2)), rng.standard_normal((2049, 1))
    var, ls, noise = (np.ascontiguousarray(a, dtype=float) for a in (np.ones(2), np.ones((2, 2)), np.full(2, 1e-2)))
    hd = _lib.Handle(0)
    try:
        hd.set_data(X, Y)
        rc = hd.lib.gp_ens_fit(hd.h, 2, _lib.dptr(var), _lib.dptr(ls), _lib.dptr(noise), 5, None, None, None, None)
        assert rc == _lib.GP_ERR_ARG
        assert hd.ens_info() == 0
    finally:
        hd.close()
