"""CPU: the long-double truth of tests/_ens_truth.py is the float64 oracle wherever float64 can tell, its case table reaches what it
says it reaches, and on every case the float64 oracle stays close enough to the truth that the bound of
tests/test_gpu_ensemble_sizes.py, max(64 x e64, FLOOR_N x scale), is never loose."""
import numpy as np
import pytest

from oracle import cpu_ref as O

import _ens_truth as ET
import _family_shapes as FS
import _kernel_families as KF
from test_gpu_ensemble import ACQS, integrated

CAP, CAP_JITTER = 1e-9, 1e-6


ROWS = (1, 4, 5, 8)             # the row counts of the GPU module: a quantity's scale is the largest entry of the rows of one call


def quantities(orc, tr, k=8):
    """(name, oracle, truth) of a member's record: the posterior at the first k of the eight points, and fmin."""
    return (("mean", orc.mu[:k], tr.mu[:k]), ("var", orc.var[0][:k], tr.var[0][:k]), ("var + noise", orc.var[1][:k], tr.var[1][:k]),
            ("dmdx", orc.dm[:k], tr.dm[:k]), ("dvdx", orc.dv[:k], tr.dv[:k]), ("fmin", orc.fmin, tr.fmin))


# ---- the reference against the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FS.ALL_FAMILIES)
@pytest.mark.parametrize("cid", ["c", "h"])
def test_truth_is_the_direct_oracle_to_float64_rounding(fam, cid):
    """_family_shapes cases c (127 x 8, ARD) and h (257 x 32, iso), the three members of FS.members: mean, both variances,
    predictive_gradients and fmin.  Bound, relative to the largest entry: 64 x 2^-53 x N variance / noise -- a backward-stable
    float64 solve loses eps x cond(Ky), cond(Ky) <= N variance / noise + 1 (lambda_max(K) <= N variance, lambda_min(Ky) >= noise),
    and 64 covers the constants of the solve and of the sums behind the gradients."""
    c = FS.CASES[cid]
    X, Y, Xs, _ = FS.problem(cid)
    x = np.vstack([Xs[:4], X[:2] + 0.013, X[2:3] - 0.02, np.full((1, c.D), 0.31)])
    var, ls, noise = FS.members(cid)
    bad = []
    for z in range(3):
        m = ET.Member(fam, c.ard, var[z], ls[z], noise[z], 0.0, X, Y)
        tr = ET._pack(*m.at(x), fmin=m.fmin, dtype=ET.T)
        gp = FS.oracle(fam, cid, z, True)
        assert gp.posterior["jitter"] == 0.0
        orc = ET._pack(*ET._oracle_at(gp, x, noise[z]), fmin=float(gp.predict(gp.X)[0].min()), dtype=np.float64)
        assert np.array_equal(orc.var[1], gp.predict(x)[1][:, 0])              # the noise added by hand is the oracle's own
        bound = 64 * 2.0 ** -53 * c.N * var[z] / noise[z]
        for what, a, b in quantities(orc, tr):
            e, s = ET.e64_of(a, b)
            print("%s %s member %d %-12s oracle against truth %.2e of the scale %.2e (bound %.2e)" % (fam, cid, z, what, e / s, s, bound))
            if not e <= bound * s:
                bad.append((z, what, e / s))
    assert not bad, bad


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_what_it_claims():
    """rw_decode / rw_nch (rows_body.h), nJ = ceil(nt / 6) (gp_ens_fit), ceil(M / 512) (ens_table_scores) and min(4, 128 // D)
    (ens_passes), restated in tests/_ens_truth.py."""
    C = ET.CASES
    assert [c.id for c in ET.TABLE] == list("pqrstuv") and all(C[k].N <= ET.ENS_MAX_NPAD for k in C)
    # the decode against its own definition: row block R has rw_nch(R) chunks, in order
    want = [(R, ch) for R in range(24) for ch in range(ET.rw_nch(R))]
    assert [ET.rw_decode(i) for i in range(len(want))] == want and ET.rows_tiles(24) == len(want)
    nt = {k: ET.tiles(C[k].N) for k in C}
    assert nt == {"p": 7, "q": 8, "r": 9, "s": 16, "t": 2, "u": 3, "v": 2}
    # p: two panels, the second one tile wide, one chunk everywhere
    assert ET.panels(7) == [6, 1] and max(ET.rw_nch(R) for R in range(7)) == 1
    # q: the last one-chunk size; nothing ragged
    assert ET.panels(8) == [6, 2] and ET.rw_nch(8 - 1) == 1 and ET.rw_nch(8) == 2 and C["q"].N == ET.npad(C["q"].N) and C["q"].N % 64 == 0
    # r: the last row block meets two chunks (nmean = rw_nch(nt - 1) = 2); one live column in the second; 127 padded rows
    assert ET.panels(9) == [6, 3] and ET.rw_nch(9 - 1) == 2 and [ET.rw_decode(i) for i in (8, 9)] == [(8, 0), (8, 1)]
    assert C["r"].N - ET.RW_CW == 1 and ET.npad(C["r"].N) - C["r"].N == 127 and ET.rows_tiles(9) == 10
    # s: the cap; three panels; the second chunk full
    assert ET.npad(C["s"].N) == C["s"].N == ET.ENS_MAX_NPAD and ET.panels(16) == [6, 6, 4]
    assert {ET.rw_nch(R) for R in range(16)} == {1, 2} and C["s"].N - ET.RW_CW == ET.RW_CW
    assert ET.npad(2049) == 2176 > ET.ENS_MAX_NPAD                              # the refusal one row past it
    # t: the member cap, ragged tiles
    assert C["t"].S == ET.ENS_MAX_S and C["t"].N % ET.GP_TILE != 0 and len(ET.members("t")[0]) == 64
    # u: two locations per pass at GP_MAX_D; four everywhere else, so 5 rows are a pass of four and a pass of one
    assert C["u"].D == ET.GP_MAX_D and ET.pass_width(64) == 2 and {ET.pass_width(C[k].D) for k in "pqrstv"} == {4}
    assert np.array_equal(ET.problem("u")[0], FS.problem("g")[0])
    # v: 40 exactly repeated rows
    Xv, Yv, _ = ET.problem("v")
    assert np.array_equal(Xv[120:], Xv[:40]) and np.array_equal(Yv[120:], Yv[:40])
    # the tables of the chunk loop
    assert ET.table_chunks(512) == [(512, 512)] and ET.table_chunks(513) == [(512, 512), (1, 128)]
    assert ET.table_chunks(1100) == [(512, 512), (512, 512), (76, 128)] and ET.table_chunks(140) == [(140, 256)]
    for k in C:
        X, Y, ls = ET.problem(k)
        var, lss, noise = ET.members(k)
        assert X.shape == (C[k].N, C[k].D) and Y.shape == (C[k].N, 1) and lss.shape == (C[k].S, C[k].D if C[k].ard else 1)
        assert np.array_equal(ET.points(k)[0], X[5]) and np.array_equal(ET.table(k, 140)[:8], ET.points(k))
        assert not X.flags.writeable and ET.problem(k)[0] is X
    assert np.array_equal(ET.table("t", 513)[:512], ET.table("t", 512))


# ---- the reference is tight enough -------------------------------------------------------------------------------------------------------
def _cap_check(fam, cid, ids, jitters, cap, tables=(), acquisitions=True):
    tr = [ET.truth(fam, cid, z, j) for z, j in zip(ids, jitters)]
    orc = [ET.oracle64(fam, cid, z, j) for z, j in zip(ids, jitters)]
    bad, worst = [], (0.0, "")
    def note(what, e, s):
        nonlocal worst
        worst = max(worst, (e / s, what))
        if not e <= cap * s:
            bad.append((what, e / s))
    for k in ROWS:                        # the members' arrays stacked, as the GPU module compares them: one scale per call
        per_member = [quantities(a, b, k) for a, b in zip(orc, tr)]
        for q, (what, _, _) in enumerate(per_member[0]):
            note("%d rows %s" % (k, what), *ET.e64_of(np.stack([m[q][1] for m in per_member]), np.stack([m[q][2] for m in per_member])))
    t64 = [ET.as64(r) for r in tr]
    for name, _, par in ACQS if acquisitions else ():
        for k in ROWS:
            args = lambda rr: ([float(r.fmin) for r in rr], [r.mu[:k] for r in rr], [r.var[1][:k] for r in rr], [r.dm[:k] for r in rr],
                               [r.dv[:k] for r in rr])
            want, got = integrated(name, par, *args(t64)), integrated(name, par, *args(orc))
            note("%s %d rows value" % (name, k), *ET.e64_of(got[0], want[0]))
            note("%s %d rows gradient" % (name, k), *ET.e64_of(got[1], want[1]))
    for M, sub in tables:
        for z in sub:
            (mu, v), (mu0, v0) = ET.oracle64_table(fam, cid, z, M), ET.truth_table(fam, cid, z, M)
            note("member %d table of %d mean" % (z, M), *ET.e64_of(mu, mu0))
            note("member %d table of %d var" % (z, M), *ET.e64_of(v, v0))
    print("%s %s: the float64 oracle's largest error against the truth: %.2e of the scale (%s); cap %.0e" % (fam, cid, worst[0], worst[1], cap))
    assert not bad, bad


TABLES = {"t": ((1100, (0, 1, 2, 3, 4)),), "r": ((140, (0, 1, 2)),), "s": ((140, (0, 1)),)}


@pytest.mark.parametrize("fam,cid", [pytest.param(f, c, id="%s-%s" % (f, c)) for f, c in ET.PAIRS])
def test_float64_oracle_is_within_the_cap_of_the_truth(fam, cid):
    """e64 <= 1e-9 x scale for every member, every quantity of the GPU module -- the posterior at the eight points, fmin, the
    integrated acquisitions and their gradients, the table's means and variances.  A condition on the inputs: a case that breaks it
    gets other parameters (_ens_truth.ISO_LS, NOISE_FACTOR), not another cap.  (The suite has no ``slow`` marker: the cases at
    N >= 1024 are computed once, through the cache the GPU module shares.)"""
    c = ET.CASES[cid]
    _cap_check(fam, cid, range(c.S), [0.0] * c.S, CAP, TABLES.get(cid, ()))


def test_jitter_case_climbs_the_ladder_within_its_cap():
    """Case v: on members 1 and 3 the float64 oracle's jitchol climbs at least one rung, on 0 and 2 none; with the oracle's rung in
    the truth's diagonal, e64 <= 1e-6 x scale (1e-9 for the two well-posed members) on what the GPU module compares in this case:
    the members' posteriors and fmin."""
    X, Y, _ = ET.problem("v")
    var, ls, noise = ET.members("v")
    jit = []
    for z in range(4):
        gp = O.OracleGP(X, Y, KF.make("rbf", 2, var[z], ls[z], False, direct=True), noise[z])
        jit.append(gp.posterior["jitter"])
    print("case v: the oracle's jitter per member", jit, "rungs", [j / (v + n + 1e-8) for j, v, n in zip(jit, var, noise)])
    assert all((jit[z] > 0.0) == (z in ET.V_ILL) for z in range(4))
    _cap_check("rbf", "v", ET.V_ILL, [jit[z] for z in ET.V_ILL], CAP_JITTER, acquisitions=False)
    _cap_check("rbf", "v", (0, 2), [0.0, 0.0], CAP, acquisitions=False)
