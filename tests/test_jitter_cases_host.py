"""CPU: the conditions that keep tests/test_gpu_jitter_routes.py from being a lottery, for every row of tests/_jitter_cases.py.

(a) Ky = K - delta I has exactly one eigenvalue -delta per duplicated pair and the next one is at least 100 delta (which is why
    delta = 3e-4 is given only to the rows whose K has its second eigenvalue above 3e-2);
(b) on every failing rung the smallest eigenvalue is at most minus half the rung (minus half delta on the un-jittered attempt), on
    the passing rung at least half the rung: no attempt's outcome depends on rounding;
(c) LAPACK's dpotrf reports info = b + 1 on every failing attempt, b the first duplicate row;
(d) the oracle's ladder stops on the rung the table states;
(e) the float64 oracle is within a tenth of the GPU test's tolerance of a long-double factorisation of the same jittered matrix
    (lml and log det 1e-9 max(1, |ref|), alpha 1e-7 relmax): every row with N <= 385, and one row of N = 1280;
(f) append rows: the oracle's refit of the grown data stops on the rung of the fit of the first N0 rows; border rows: the first N0
    rows need no jitter, dpotrf of the grown matrix stops at row N0 + j, the refit lands on the table's rung;
and for the batched entry: the hard members fail un-jittered, two of them in the third tile, and the easy ones factor.
"""
import numpy as np
import pytest
from scipy.linalg import lapack

import _jitter_cases as J
from _sparse_ref import LD
from oracle import cpu_ref as O

_EIG = {}


def eig_K(cid):
    if cid not in _EIG:
        _EIG[cid] = np.linalg.eigvalsh(J.kernel(J.CASES[cid].fam).K(J.problem(cid)[0]))
    return _EIG[cid]


def Ky_of(kern, X, delta):
    Ky = kern.K(X).copy()
    O.diag_add(Ky, J.noise_of(delta) + 1e-8)
    return Ky


def attempts(delta, tries):
    """The diagonal shifts of the attempts that fail, and the one that passes."""
    return [0.0] + [J.rung(delta, t) for t in range(1, tries)], J.rung(delta, tries)


def test_the_table_covers_what_it_claims():
    ids = [c.id for c in J.TABLE]
    assert len(set(ids)) == len(ids)
    b = {J.first_pivot(c) for c in J.TABLE if c.N == 1280}
    assert b >= {1, 133, 261, 383, 384, 677, 1279}
    assert all(J.DELTA in c.deltas for c in J.TABLE)
    assert {d for c in J.TABLE for d in c.deltas} == set(J.TRIES)
    assert any(c.P == 2 for c in J.TABLE) and any(len(c.pairs) == 2 for c in J.TABLE)
    assert {(c.N, J.first_pivot(c)) for c in J.TABLE if not c.multi} == {(257, 256), (385, 384)}
    # a multi-delta row on the look-ahead routes, and both families at the extreme deltas
    assert any(c.multi and len(c.deltas) == 3 for c in J.TABLE)
    for d in (3e-6, 3e-4):
        assert {c.fam for c in J.TABLE if d in c.deltas} == {"rbf", "Mat52"}


@pytest.mark.parametrize("cid,delta", J.SINGLE, ids=lambda v: str(v))
def test_eigenvalues_keep_every_rung_decision_away_from_rounding(cid, delta):
    c = J.CASES[cid]
    w = eig_K(cid) + (J.noise_of(delta) + 1e-8)
    npairs = len(c.pairs)
    print("%s delta %g: smallest %s next %.3e" % (cid, delta, w[:npairs], w[npairs]))
    assert np.all(np.abs(w[:npairs] + delta) <= 1e-2 * delta)          # (a) -delta to two digits and better
    assert w[npairs] >= 100 * delta
    failing, passing = attempts(delta, J.TRIES[delta])
    for r in failing:                                                   # (b)
        assert w[0] + r <= -0.5 * max(r, delta)
    assert w[0] + passing >= 0.5 * passing
    # the hopeless delta: every one of the five rungs fails by the same margin
    w5 = eig_K(cid) + (J.noise_of(J.DELTA_FAILS) + 1e-8)
    for t in range(1, J.MAXTRIES + 1):
        assert w5[0] + J.rung(J.DELTA_FAILS, t) <= -0.5 * J.DELTA_FAILS
    assert J.VAR + (-2.0 + 1e-8) < 0          # noise -2: the non-positive diagonal


@pytest.mark.parametrize("cid,delta", J.SINGLE, ids=lambda v: str(v))
def test_lapack_pivot_and_the_oracles_rung(cid, delta):
    c = J.CASES[cid]
    X = J.problem(cid)[0]
    kern = J.kernel(c.fam)
    Ky = Ky_of(kern, X, delta)
    failing, passing = attempts(delta, J.TRIES[delta])
    for r in failing:                                                   # (c)
        _, info = lapack.dpotrf(Ky + r * np.eye(c.N), lower=1)
        assert info == J.first_pivot(c) + 1, (r, info)
    assert lapack.dpotrf(Ky + passing * np.eye(c.N), lower=1)[1] == 0
    jit = J.oracle(cid, delta).posterior["jitter"]                      # (d)
    assert abs(jit - passing) <= 1e-12 * passing, (jit, passing)
    if delta == J.DELTA:
        K5 = Ky_of(kern, X, J.DELTA_FAILS)
        for t in range(0, J.MAXTRIES + 1):
            r = J.rung(J.DELTA_FAILS, t) if t else 0.0
            # (K - 0.5 I has many negative eigenvalues: the pivot is some earlier row, so only the sign is stated)
            assert 0 < lapack.dpotrf(K5 + r * np.eye(c.N), lower=1)[1] <= J.first_pivot(c) + 1
        with pytest.raises(np.linalg.LinAlgError, match="even with jitter"):
            O.jitchol(K5, J.MAXTRIES)
        with pytest.raises(np.linalg.LinAlgError, match="non-positive diagonal"):
            O.jitchol(kern.K(X) + (-2.0 + 1e-8) * np.eye(c.N), J.MAXTRIES)


def _truth_gap(gp, delta, Xs=None):
    """The oracle's lml, log det and alpha -- and, with ``Xs``, its posterior mean and variance with noise there -- against a
    long-double factorisation of the same jittered float64 matrix."""
    p = gp.posterior
    N, P = gp.Y.shape
    A = p["K"].copy()
    O.diag_add(A, gp.noise_var + 1e-8)
    A = A + np.eye(N) * p["jitter"]          # (as jitchol adds it)
    A = A.astype(np.longdouble)
    L, _ = LD.chol(A)
    Y = gp.Y.astype(np.longdouble)
    alpha = LD.solve(L, LD.solve(L, Y, 0), 1)
    logdet = 2 * np.sum(np.log(np.diag(L)))
    lml = 0.5 * (-N * P * np.log(2 * np.longdouble(np.pi)) - P * logdet - np.sum(alpha * Y))
    g_lml = float(abs(p["lml"] - lml)) / max(1.0, abs(float(lml)))
    g_ld = float(abs(p["logdet"] - logdet)) / max(1.0, abs(float(logdet)))
    g_al = float(np.max(np.abs(p["alpha"] - alpha))) / max(1.0, float(np.max(np.abs(alpha))))
    if Xs is None:
        return g_lml, g_ld, g_al
    Kx = gp.kern.K(gp.X, Xs).astype(np.longdouble)
    t = LD.solve(L, Kx, 0)
    var = gp.kern.Kdiag(Xs).astype(np.longdouble) - np.sum(t * t, 0) + np.longdouble(gp.noise_var)
    m0, v0 = gp.predict(Xs)
    g_m = float(np.max(np.abs(m0 - Kx.T @ alpha))) / max(1.0, float(np.max(np.abs(m0))))
    g_v = float(np.max(np.abs(v0[:, 0] - var) / np.abs(var)))
    return g_lml, g_ld, g_al, g_m, g_v


TRUTH = tuple((c.id, d) for c in J.TABLE if c.N <= 385 for d in c.deltas) + (("mid", 3e-6), ("mid", 3e-5))


@pytest.mark.parametrize("cid,delta", TRUTH, ids=lambda v: str(v))
def test_oracle_against_a_long_double_truth(cid, delta):
    """(e): cond of the jittered matrix is 4e6 at delta = 3e-6 (the worst the GPU test compares posteriors at), so float64 carries
    ~1e-10 there.  The posterior at the first five candidates rides along (1e-7 relative)."""
    g_lml, g_ld, g_al, g_m, g_v = _truth_gap(J.oracle(cid, delta), delta, J.problem(cid)[2][:5])
    print("%s delta %g: lml %.2e logdet %.2e alpha %.2e mean %.2e var %.2e" % (cid, delta, g_lml, g_ld, g_al, g_m, g_v))
    assert g_lml <= 1e-9 and g_ld <= 1e-9 and g_al <= 1e-7
    # the first candidates: the duplicated point itself, where the variance with the (negative) noise is ~ (jitter - 3 delta) / 2
    assert g_m <= 1e-7 and g_v <= 1e-7


@pytest.mark.parametrize("c", J.APPEND, ids=lambda c: c.id)
def test_append_rows_refit_on_the_rung_of_the_first_fit(c):
    X, Y, _ = J.append_problem(c.id)
    kern = J.kernel(c.fam)
    want = J.rung(J.DELTA, J.TRIES[J.DELTA])
    for n in (c.N0, c.N0 + c.k):
        w = np.linalg.eigvalsh(kern.K(X[:n])) - J.DELTA
        assert abs(w[0] + J.DELTA) <= 1e-2 * J.DELTA and w[1] >= 100 * J.DELTA
        gp = O.OracleGP(X[:n], Y[:n], kern, J.noise_of(J.DELTA))
        assert abs(gp.posterior["jitter"] - want) <= 1e-12 * want
        assert max(_truth_gap(gp, J.DELTA)[:2]) <= 1e-9 and _truth_gap(gp, J.DELTA)[2] <= 1e-7
    assert lapack.dpotrf(Ky_of(kern, X, J.DELTA), lower=1)[1] == c.pair[1] + 1


@pytest.mark.parametrize("c", J.BORDER, ids=lambda c: c.id)
def test_border_rows_fail_at_the_duplicated_row(c):
    X, Xbad, Y, _ = J.border_problem(c.id)
    kern = J.kernel(c.fam)
    assert O.OracleGP(X[:c.N0], Y[:c.N0], kern, J.noise_of(J.DELTA)).posterior["jitter"] == 0.0
    assert O.OracleGP(X, Y, kern, J.noise_of(J.DELTA)).posterior["jitter"] == 0.0       # the clean append
    assert np.linalg.eigvalsh(kern.K(X))[0] - J.DELTA >= 100 * J.DELTA
    Xg = np.vstack([X[:c.N0], Xbad])
    w = np.linalg.eigvalsh(kern.K(Xg)) - J.DELTA
    assert abs(w[0] + J.DELTA) <= 1e-2 * J.DELTA and w[1] >= 100 * J.DELTA
    assert lapack.dpotrf(Ky_of(kern, Xg, J.DELTA), lower=1)[1] == c.N0 + c.j + 1
    # the border's own pivot (the Schur complement of the first N0 + j rows) is negative by about twice delta
    n = c.N0 + c.j
    Ky = Ky_of(kern, Xg, J.DELTA)
    piv = Ky[n, n] - Ky[n, :n] @ np.linalg.solve(Ky[:n, :n], Ky[:n, n])
    assert piv <= -J.DELTA
    want = J.rung(J.DELTA, J.TRIES[J.DELTA])
    jit = O.OracleGP(Xg, Y, kern, J.noise_of(J.DELTA)).posterior["jitter"]
    assert abs(jit - want) <= 1e-12 * want


def test_batch_members_fail_unjittered():
    """The hard members of the batched case fail un-jittered on the CPU (the easy ones factor), members 6 and 7 in the third
    tile and not before: their first 260 rows factor, and the first rung factors all 300."""
    X, Y = J.batch_problem()
    n = J.BATCH_N - J.BATCH_DUP
    assert X.shape == (J.BATCH_N, 2) and np.array_equal(X[n:], X[:J.BATCH_DUP]) and n > 2 * J.TILE
    hard = J.BATCH_NOISE < 1e-6
    assert hard.any() and not hard.all()
    for r in range(len(J.BATCH_VAR)):
        K = O.make_kernel("rbf", 2, J.BATCH_VAR[r], J.BATCH_LS[r], ARD=False).K(X)
        A = K + (J.BATCH_NOISE[r] + 1e-8) * np.eye(J.BATCH_N)
        info = lapack.dpotrf(A, lower=1)[1]
        print("member %d: dpotrf info %d" % (r, info))
        assert (info > 0) == bool(hard[r])
        if r in J.BATCH_THIRD_TILE:
            assert n < info <= J.BATCH_N
            assert lapack.dpotrf(A[:n, :n], lower=1)[1] == 0
            assert np.linalg.eigvalsh(K[:n, :n])[0] >= 1e-2 * J.BATCH_VAR[r]
            assert np.all(np.diag(A) == J.BATCH_VAR[r])                         # the diagonal's 1e-8 is rounded away
            assert lapack.dpotrf(A + np.diag(A).mean() * 1e-6 * np.eye(J.BATCH_N), lower=1)[1] == 0
