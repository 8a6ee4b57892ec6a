"""CPU: the long-double cost surface of tests/_cost_truth.py is the posterior mean the oracle computes -- ``Stationary.K @ alpha``
and ``gradients_X`` of oracle/cpu_ref.py for RBF and Matern-5/2 --, its gradients are the derivatives of its values in all four
families (central differences in long double), and the case table reaches what tests/test_gpu_cost.py says it reaches."""
import numpy as np
import pytest

from oracle import cpu_ref as O

import _cost_truth as CT

T = np.longdouble


@pytest.mark.parametrize("cid", [c.id for c in CT.TABLE if c.fam in ("rbf", "Mat52") and c.Nc <= 1000])
def test_truth_is_the_oracles_posterior_mean(cid):
    p = CT.problem(cid)
    c = p.case
    logc, dlogc = CT.truth(cid)[:2]
    kern = O.make_kernel(c.fam, c.D, variance=p.variance, lengthscale=p.ls_arg, ARD=c.ard)
    K = kern.K(p.Xs, p.Xc)
    mean = c.shift + c.scale * (K @ p.alpha)
    # the oracle's distances come from the expanded square (|x|^2 + |y|^2 - 2 x.y): absolute error ~ eps D / l^2 in r^2, which a
    # coincident pair turns into r ~ 1e-8 instead of 0 -- hence 1e-7 on the values' scale rather than a few eps
    scale = np.abs(c.scale) * (np.abs(K) @ np.abs(p.alpha)) + abs(c.shift)
    assert np.all(np.abs(mean - logc.astype(float)) <= 1e-7 * scale)
    grad = c.scale * kern.gradients_X(np.tile(p.alpha, (c.M, 1)), p.Xs, p.Xc)
    gscale = np.abs(grad).max() + np.abs(dlogc.astype(float)).max()
    assert np.all(np.abs(grad - dlogc.astype(float)) <= 1e-6 * gscale)


@pytest.mark.parametrize("cid", ["b", "c", "d", "e", "h", "k", "a"])
def test_gradient_is_the_derivative_of_the_value(cid):
    p = CT.problem(cid)
    c = p.case
    rows = [m for m in range(min(c.M, 6)) if m not in c.same]       # (the Exponential has a kink at a coincident point)
    Xs = p.Xs[rows]
    _, dlogc, _, _, sabs = CT.surface(c.fam, p.variance, p.ls, p.Xc, p.alpha, c.shift, c.scale, Xs)
    h = T(2.0) ** -24
    for d in range(min(c.D, 4)):
        step = np.zeros(c.D, T)
        step[d] = h
        up = _surface_ld(p, Xs.astype(T) + step)
        dn = _surface_ld(p, Xs.astype(T) - step)
        fd = (up - dn) / (2 * h)
        # truncation h^2 f''' / 6 with h = 6e-8; cancellation eps_ld |f| / h = 2e-12 |f|
        assert np.all(np.abs(fd - dlogc[:, d]) <= 1e-9 * (sabs / p.ls[d] + np.abs(dlogc[:, d])))


def _surface_ld(p, Xs_ld):
    """logc at long-double locations (the finite differences move the locations by less than a double's spacing allows)."""
    c = p.case
    l = p.ls.astype(T)
    df = (Xs_ld / l)[:, None, :] - (p.Xc.astype(T) / l)[None, :, :]
    r = np.sqrt((df * df).sum(-1))
    k = CT.family(c.fam, p.variance, r)[0]
    return T(c.shift) + T(c.scale) * (p.alpha.astype(T) * k).sum(-1)


def test_coincident_rows_have_r_zero_and_the_exponential_takes_nothing_from_them():
    for cid in ("d", "h", "k"):
        p = CT.problem(cid)
        assert p.case.fam == "Exponential" and p.case.same
        for row in p.case.same:
            hit = np.flatnonzero((p.Xc == p.Xs[row]).all(1))
            assert hit.size >= 1
            # the truth without the coincident term equals the truth with it: its gradient share is exactly 0
            keep = np.setdiff1d(np.arange(p.case.Nc), hit)
            with_, without = (CT.surface("Exponential", p.variance, p.ls, p.Xc[sel], p.alpha[sel], 0.0, 1.0, p.Xs[[row]])[1]
                              for sel in (np.arange(p.case.Nc), keep))
            assert np.array_equal(with_, without)


def test_case_table_reaches_what_it_says():
    t = CT.TABLE
    assert {c.Nc for c in t} >= {1, 63, 65, 257, 1000}
    assert {c.D for c in t} == {1, 3, 8, 64}
    assert {c.M for c in t} >= {1, 5, 8, 9, 130, 1025}
    assert {(c.fam, c.ard) for c in t} == {(f, a) for f in CT.KERNEL_IDS for a in (False, True)}
    assert any(len(c.same) >= 2 and c.M > 8 for c in t)
    assert any(c.shift != 0.0 and c.scale != 1.0 for c in t)
    assert any(-(-c.Nc // CT.COST_CB) > 256 for c in t)            # a second round of the few-rows kernel's threads
