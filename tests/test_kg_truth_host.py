"""CPU: the knowledge gradient's truth (tests/_kg_truth.py) held to what does not depend on it -- a Monte Carlo of E[min] over the
truth's own lines, central differences of its value, the two-line closed form -- and the conditions every case of the table must
satisfy so that the GPU tests test something: substantial KG, and no gradient taken at the kink of the lowest intercept."""
import numpy as np
import pytest

import _kg_truth as KT

T = KT.T
CASE_IDS = [c.id for c in KT.TABLE]


@pytest.mark.parametrize("cid", CASE_IDS)
def test_conditions(cid):
    sv = KT.truth(cid)
    c = sv.p.case
    share, worst = KT.conditions(sv)
    v = np.asarray(sv.truth.value, dtype=float)
    print("kg conditions[%s]: share of locations with KG >= 1000 allowances %.2f; smallest intercept gap / allowance where x's own "
          "line is one of the two lowest: %.3e; KG median %.3e, max %.3e; floored locations %d"
          % (cid, share, worst, np.median(v), v.max(), int(sv.truth.floored.sum())))
    assert share >= 0.5
    assert worst >= KT.MARGIN_FACTOR
    assert sv.truth.value.shape == (c.Mt,) and sv.truth.grad.shape == (c.Mr, c.D) and sv.truth.mu.shape == (c.A,)
    # KG >= 0 (to the rounding of the sum's terms), and the masses of the lines add up to one
    rounding = 64 * np.finfo(np.float64).eps * (np.asarray(sv.truth.atil, dtype=float).max(1) + np.abs(np.asarray(sv.truth.b, dtype=float)).max(1))
    assert np.all(v >= -rounding)
    assert np.allclose(np.asarray(sv.truth.p.sum(1), dtype=float), 1.0, rtol=0, atol=1e-15)
    assert np.allclose(np.asarray(sv.truth.q.sum(1), dtype=float), 0.0, rtol=0, atol=1e-15)


def test_the_special_locations_are_what_they_claim():
    d, e, g = KT.truth("d"), KT.truth("e"), KT.truth("g")
    assert np.array_equal(d.p.Xs[2], d.p.X[17]) and not d.truth.floored[2]          # on a training input, far above the floor at y_std 1.7
    assert np.array_equal(g.p.Xs[2], g.p.X[17]) and g.truth.floored[2] and g.truth.floored.sum() == 1 and g.p.case.Mr > 2
    assert np.array_equal(e.p.Xa[200], e.p.Xa[5])                                   # the same point twice
    tr = e.truth
    assert np.all(tr.atil[:, 200] == tr.atil[:, 5]) and np.all(tr.b[:, 200] == tr.b[:, 5])
    assert np.all(tr.p[:, 200] == 0) and np.all(tr.q[:, 200] == 0)                  # the lowest index owns the interval
    assert np.array_equal(e.p.Xs[10], e.p.Xa[9]) and e.p.case.Mr <= 10              # on a point: beyond the gradient rows
    A = e.p.case.A
    assert abs(float(tr.atil[10, A] - tr.atil[10, 9])) < 1e-12 and abs(float(tr.b[10, A] - tr.b[10, 9])) < 1e-6      # nearly identical lines


@pytest.mark.parametrize("cid,rows", [("b", (0, 1, 20)), ("c", (0, 17)), ("e", (1, 10))])
def test_truth_against_monte_carlo(cid, rows):
    """2 10^6 samples of min_i (a~_i + b_i Z) at 5 standard errors, in chunks (no [S, A + 1] array of the whole sample)."""
    tr = KT.truth(cid).truth
    rng = np.random.default_rng(77)
    S, chunk = 2_000_000, 50_000
    for m in rows:
        a, b = np.asarray(tr.atil[m], dtype=float), np.asarray(tr.b[m], dtype=float)
        s1 = s2 = 0.0
        for _ in range(S // chunk):
            z = rng.standard_normal(chunk)
            y = np.min(a[None, :] + z[:, None] * b[None, :], axis=1)
            s1 += float(y.sum())
            s2 += float((y * y).sum())
        mean = s1 / S
        se = np.sqrt(max(s2 / S - mean * mean, 0.0) / S)
        kg = float(tr.value[m])
        print("kg Monte Carlo[%s, row %d]: truth %.6e  estimate %.6e  |diff| / standard error = %.2f" % (cid, m, kg, -mean, abs(kg + mean) / se))
        assert abs(kg + mean) <= 5 * se


@pytest.mark.parametrize("cid", ["b", "g"])
def test_truth_gradient_against_central_differences(cid):
    sv = KT.truth(cid)
    c, p = sv.p.case, sv.p
    h = 1e-6
    pts = []
    for m in range(c.Mr):
        for d in range(c.D):
            for sgn in (+1, -1):
                x = np.asarray(p.Xs[m], dtype=T).copy()
                x[d] += sgn * T(h)
                pts.append(x)
    v = KT.evaluate(c.fam, KT.VARIANCE, c.noise, sv.fit, p.Xa, np.array(pts, dtype=T), 0, y_std=c.y_std).value.reshape(c.Mr, c.D, 2)
    num = (v[:, :, 0] - v[:, :, 1]) / (2 * T(h))
    g = sv.truth.grad
    scale = float(np.max(np.abs(g)))
    err = float(np.max(np.abs(num - g)))
    print("kg central differences[%s]: max |g| %.3e  max |difference quotient - gradient| %.3e" % (cid, scale, err))
    # the quotient's own error: h^2 / 6 |f'''| ~ 1e-12 |g| / l^2 at lengthscales ~ 0.05 .. 0.5, and rounding 1e-19 KG / h
    assert err <= 1e-6 * scale
    if cid == "g":      # the floored location: no variance left to learn from, every q_i is 0 -- KG and its gradient are 0 there
        assert sv.truth.floored[2] and float(np.max(np.abs(num[2] - g[2]))) <= 1e-6 * scale


def test_one_point_is_the_two_line_closed_form():
    sv = KT.truth("a")
    tr = sv.truth
    assert sv.p.case.A == 1 and tr.atil.shape == (1, 2)
    closed = KT.two_line_closed_form(tr.atil[0], tr.b[0])
    print("kg A = 1: sweep %.18e  closed form %.18e" % (float(tr.value[0]), float(closed)))
    assert abs(float(tr.value[0] - closed)) <= 1e-17 * max(1.0, abs(float(closed)))


def test_hull_sweep_on_lines_by_hand():
    # three lines: 0 + 1 z, 0 - 1 z, and -1 + 0 z is NOT below their minimum anywhere beyond |z| < 1: it owns (-1, 1)
    a, b = np.array([0.0, 0.0, -1.0], dtype=T), np.array([1.0, -1.0, 0.0], dtype=T)
    lo, hi = KT.hull(a, b)
    assert (lo[0], hi[0]) == (-np.inf, -1.0) and (lo[2], hi[2]) == (-1.0, 1.0) and (lo[1], hi[1]) == (1.0, np.inf)
    # a dominated line, a parallel higher line and an identical twin own nothing
    a, b = np.array([0.0, 0.0, 5.0, 1.0, 0.0], dtype=T), np.array([1.0, -1.0, 0.0, 1.0, 1.0], dtype=T)
    lo, hi = KT.hull(a, b)
    p, q = KT.masses(lo, hi)
    assert float(p[0]) == 0.5 and float(p[1]) == 0.5 and np.all(p[2:] == 0) and np.all(q[2:] == 0)
    # E[min(z, -z)] = -E|z| = -sqrt(2 / pi)
    assert abs(float(-(a @ p + b @ q)) - np.sqrt(2 / np.pi)) < 1e-18
    f64 = KT.hull(a.astype(np.float64), b.astype(np.float64))
    assert f64[0].dtype == np.float64
