"""CPU: the long-double truth of the joint expected improvement (tests/_qei_truth.py) -- its gradient against central differences
of its own value, the conditions every case of the table must satisfy (so that a bad seed fails here and is not excused on the
GPU), q = 1 over stratified base samples against the closed-form EI, and the rule that the rows of the factor follow the caller's
order."""
import numpy as np
import pytest

import _qei_truth as QT

T = QT.T
CASE_IDS = [c.id for c in QT.TABLE]


def _value(sv, Xq):
    c = sv.p.case
    return QT.evaluate(c.fam, QT.VARIANCE, c.noise, sv.fit, Xq, sv.p.Z, sv.t0, grad=False).value


@pytest.mark.parametrize("cid", CASE_IDS)
def test_gradient_against_central_differences(cid):
    sv = QT.truth(cid)
    Xq = np.asarray(sv.p.Xq, dtype=T)
    g = sv.truth.grad
    h = T(1e-7)      # truncation ~ h^2 f''' ~ 1e-13, rounding ~ eps_80 / h ~ 1e-12: far inside the 1e-8 asked for
    # every coordinate; case c (q D = 128) every fifth, first and last included
    coords = list(range(g.size)) if g.size <= 64 else sorted(set(range(0, g.size, 5)) | {g.size - 1})
    fd = np.empty(len(coords), dtype=T)
    for k, idx in enumerate(coords):
        E = np.zeros_like(Xq)
        E.flat[idx] = h
        fd[k] = (_value(sv, Xq + E) - _value(sv, Xq - E)) / (2 * h)
    err = float(np.max(np.abs(fd - g.ravel()[coords])))
    print("qei truth[%s] gradient against central differences: worst %.3e (max |g| %.3e)" % (cid, err, float(np.abs(g).max())))
    assert err <= 1e-8 * max(1.0, float(np.abs(g).max()))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_case_conditions(cid):
    sv = QT.truth(cid)
    c = sv.p.case
    share, margin, need = QT.conditions(sv)
    print("qei truth[%s] active share %.3f, smallest margin %.3e, needed %.3e, allowance %.3e" % (cid, share, margin, need, sv.allowance))
    if c.S == 1:
        assert share == 1.0
    else:
        assert 0.4 <= share <= 0.6
        assert int(sv.truth.active.sum()) == c.S // 2      # the midpoint of the two middle order statistics
    assert margin >= need                                   # no sample is left out of any comparison
    assert sv.truth.value > 0 and np.all(np.isfinite(np.asarray(sv.truth.grad, dtype=float)))
    # the float64 restatement selects what the truth selects: its error is rounding, not a flipped sample
    f64 = QT.float64_restatement(cid)
    assert np.array_equal(f64.truth.jstar, sv.truth.jstar) and np.array_equal(f64.truth.active, sv.truth.active)


def test_case_table_covers_what_the_kernels_branch_on():
    by = QT.CASES
    assert by["a"].N == 130 and by["d"].N == 1100                       # two 128-row blocks; two 1024-column chunks
    assert sorted({c.q for c in QT.TABLE}) == [1, 2, 3, 4, 5, 8]        # the pass layouts 1, <= 4, 5 .. 8
    assert by["c"].q * by["c"].D == 128                                 # the limit of the kernel arguments
    assert by["d"].S % 64 and by["d"].S % 256 and by["f"].S == 1
    assert {c.fam for c in QT.TABLE} == set(QT.FAMILY_ID)
    g = QT.problem("g")
    assert g.Z.shape[1] == 8 and g.case.q == 3 and np.array_equal(g.Xq[1], g.X[17])


def test_q1_stratified_samples_against_the_closed_form():
    sv = QT.truth("e")
    c = sv.p.case
    Z = QT.stratified_normals()
    assert Z.shape == (4096, 1) and abs(float(Z.mean())) < 1e-12
    tr = QT.evaluate(c.fam, QT.VARIANCE, c.noise, sv.fit, sv.p.Xq, Z, sv.t0, grad=False)
    m, s = tr.mean[0], np.sqrt(tr.cov[0, 0])
    exact = QT.closed_form_ei(m, s, sv.t0)
    quad = QT.quadrature_error(m, s, sv.t0)
    print("qei truth q = 1: closed form %.6e, stratified estimate %.6e, quadrature error %.3e" % (exact, float(tr.value), quad))
    assert abs(float(tr.value) - exact) <= quad * (1 + 1e-9) + 1e-15      # the estimate IS that midpoint rule
    assert 0 < quad < exact                                               # measured, not assumed; and it is a correction, not the value


def test_rows_follow_the_callers_order():
    """A joint permutation of the locations leaves the posterior the permuted posterior, and the value the same only in
    DISTRIBUTION: with the same base samples the factor's rows mix them differently, sample by sample."""
    sv = QT.truth("b")
    c = sv.p.case
    perm = np.roll(np.arange(c.q), 3)
    tr = QT.evaluate(c.fam, QT.VARIANCE, c.noise, sv.fit, sv.p.Xq[perm], sv.p.Z, sv.t0, grad=False)
    assert float(np.max(np.abs(tr.mean - sv.truth.mean[perm]))) <= 1e-16
    assert float(np.max(np.abs(tr.cov - sv.truth.cov[np.ix_(perm, perm)]))) <= 1e-16
    ys, ys0 = T(sv.t0) - tr.imp, (T(sv.t0) - sv.truth.imp)[:, perm]
    assert float(np.max(np.abs(ys - ys0))) > 1e-3                          # not the same samples
    assert abs(float(tr.value - sv.truth.value)) > sv.allowance             # ... nor the same value
    sd = float(np.std(np.asarray(np.maximum(sv.truth.imp.max(axis=1), 0), dtype=float)))
    assert abs(float(tr.value - sv.truth.value)) <= 6 * sd / np.sqrt(c.S)   # ... but the same expectation: inside the Monte Carlo error
