"""CPU: the long-double GP with an affine mean function of tests/_mean_truth.py against its two float64 references -- the same
formulas in float64, and the pinned oracle used as it is (``oracle.cpu_ref.OracleGP`` on the targets Y - m(X), plus m(x*) and A on
the way out) -- and the reach of the case table tests/test_gpu_mean_function.py runs.

The oracle's error against the truth is e64 of the GPU test's bound max(64 x e64, floor x scale): it is capped here at 1e-9 of the
scale of each quantity (the worst here is 1.2e-10, dvdx of case e), so that bound is never loose.
"""
import numpy as np
import pytest

import _mean_truth as MT

T = MT.T
FIELDS = ("lml", "logdet", "alpha", "dvar", "dls", "dnoise", "dA", "db", "mu", "dm", "dv", "train_mean")


def _err(ref, true):
    true = np.asarray(true, dtype=T)
    return float(np.max(np.abs(np.asarray(ref, dtype=T) - true))), max(float(np.max(np.abs(true))), 1e-300)


@pytest.mark.parametrize("cid", [c.id for c in MT.TABLE])
@pytest.mark.parametrize("ref", ["closed64", "oracle64"])
def test_truth_against_the_float64_references(cid, ref):
    tr, r64 = MT.truth(cid), getattr(MT, ref)(cid)
    for f in FIELDS:
        err, scale = _err(getattr(r64, f), getattr(tr, f))
        print("%s %s %-10s err %.3e scale %.3e" % (ref, cid, f, err, scale))
        assert err <= 1e-9 * scale, (f, err, scale)
    for i in (0, 1):
        err, scale = _err(r64.var[i], tr.var[i])
        assert err <= 1e-9 * scale, ("var", i, err, scale)


@pytest.mark.parametrize("cid", ["b", "d", "e"])
def test_mean_gradients_are_the_derivatives_of_the_lml(cid):
    """dA and db of the truth against central differences of its LML in long double."""
    p = MT.problem(cid)
    c = p.case
    tr = MT.truth(cid)
    h = T(2.0) ** -20

    def lml(A, b):
        return MT.MeanGP(c.fam, c.ard, MT.VAR, p.ls, MT.NOISE, p.X, p.Y, A, b).lml

    if p.A is not None:
        for (d, q) in ((0, 0), (c.D - 1, c.P - 1)):
            E = np.zeros((c.D, c.P), T)
            E[d, q] = h
            fd = (lml(p.A.astype(T) + E, p.b) - lml(p.A.astype(T) - E, p.b)) / (2 * h)
            assert abs(fd - tr.dA[d, q]) <= 1e-9 * max(abs(tr.dA[d, q]), 1.0)      # the LML is quadratic in A: no truncation error
    if p.b is not None:
        e = np.zeros(c.P, T)
        e[0] = h
        fd = (lml(p.A, p.b.astype(T) + e) - lml(p.A, p.b.astype(T) - e)) / (2 * h)
        assert abs(fd - tr.db[0]) <= 1e-9 * max(abs(tr.db[0]), 1.0)


def test_mean_enters_the_posterior_and_fmin_as_the_reference_adds_it():
    """gp.py:293-294: mu += mean_function.f(Xnew); at a training input the mean is y_i - (noise + 1e-8) alpha_i with the RAW y."""
    cid = "d"
    p, tr, gp = MT.problem(cid), MT.truth(cid), MT.model(cid)
    zero = MT.MeanGP(p.case.fam, p.case.ard, MT.VAR, p.ls, MT.NOISE, p.X, np.asarray(gp.R, dtype=np.float64), None, None)
    mu0 = zero.at(MT.points(cid))[0]
    assert np.max(np.abs(mu0 + MT.mean_of(p.A, p.b, MT.points(cid)) - tr.mu)) <= 1e-15
    ident = p.Y.astype(T) - (T(MT.NOISE) + T(1e-8)) * gp.alpha
    assert np.max(np.abs(ident - tr.train_mean)) <= 1e-14 * np.max(np.abs(tr.train_mean))


def test_scores_are_the_oracles_rules():
    cid = "d"
    mu, v0, v1, dm, dv = MT.oracle64_table(cid, 9)
    gp = MT.oracle_gp(cid)
    fmin = float(MT.oracle64(cid).train_mean.min())
    for name in MT.RULES:
        neg, dneg = MT.scores(name, mu[:, 0], v1, dm[:, :, 0], dv, fmin)
        assert neg.shape == (9,) and dneg.shape == (9, 3) and np.all(np.isfinite(neg)) and np.all(np.isfinite(dneg))
    # LCB by hand: -(−m + 2 s)
    neg, dneg = MT.scores("LCB", mu[:, 0], v1, dm[:, :, 0], dv, fmin)
    assert np.allclose(neg, mu[:, 0] - 2.0 * np.sqrt(v1), rtol=0, atol=1e-15)
    assert gp.posterior["jitter"] == 0.0


def test_case_table_reaches_what_it_says():
    t = MT.TABLE
    assert {c.N for c in t} >= {1, 127, 128, 129, 257, MT.MEAN_GRAD_CH - 1, MT.MEAN_GRAD_CH, MT.MEAN_GRAD_CH + 1}
    assert {c.D for c in t} == {1, 3, 64} and {c.P for c in t} == {1, 3, 16}
    assert {c.parts for c in t} == {"A", "b", "Ab"}
    assert {c.fam for c in t} == {"rbf", "Mat52", "Mat32", "Exponential"} and {c.ard for c in t} == {False, True}
    assert all(c.D + c.P <= 79 for c in t)                         # the gradient pass's LDS limit (api_internal.h)
    assert any(c.D == 64 and c.P == 1 for c in t)                  # two locations per fused pass
    for c in t:
        p = MT.problem(c.id)
        assert (p.A is not None) == ("A" in c.parts) and (p.b is not None) == ("b" in c.parts)
        assert np.array_equal(MT.points(c.id)[0], p.X[min(5, c.N - 1)])
