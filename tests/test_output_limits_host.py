"""CPU: the case table of tests/_output_limits.py says what the LDS arithmetic of the gradient launches says, its targets cannot
hide an index error, and the float64 oracles that tests/test_gpu_output_limits.py compares the device with are within a tenth of
the parity bar of a long-double truth on every case -- per output column."""
import numpy as np
import pytest

import _output_limits as OL
import _sparse_ref as SR
from _sparse_ref import LD

T = np.longdouble
LIMIT = OL.LDS_GFX950


# ---- the LDS arithmetic -----------------------------------------------------------------------------------------------------------
def test_lds_formulas_reproduce_the_table():
    """The `grad` column is what lml_grad_lds_bytes (csrc/grad.hip) gives against 163840 bytes; the figures the issue quotes; the
    closed forms D + P <= 79 / 2 D + P <= 79 over every accepted shape; gradx and the sparse pass fit at every accepted shape."""
    for c in OL.TABLE:
        need = OL.lds_lml_grad(c.D, c.gower, c.P)
        print("%-7s D %2d P %3d gower %d: %6d B, %s" % (c.id, c.D, c.P, c.gower, need, c.grad))
        assert OL.fits(c) == (c.grad == "yes")
        assert (c.grad == "P") == (c.P > 16)
        assert (c.grad == "lds") == (c.P <= 16 and need > LIMIT)
    assert OL.lds_lml_grad(64, False, 16) == 164416 and OL.lds_lml_grad(64, False, 1) == 133696
    assert OL.lds_lml_grad(64, False, 15) <= LIMIT and OL.lds_lml_grad(63, False, 16) <= LIMIT
    assert OL.lds_gradx(64, 16) == LIMIT                       # fits by zero bytes
    for D in range(1, 65):
        for P in range(1, 17):
            assert (OL.lds_lml_grad(D, False, P) <= LIMIT) == (D + P <= 79)
            assert (OL.lds_lml_grad(D, True, P) <= LIMIT) == (2 * D + P <= 79)
            assert OL.lds_gradx(D, P) <= LIMIT and OL.lds_sparse_grad(D, P) <= LIMIT
    assert all(OL.lds_lml_grad(40, True, P) > LIMIT for P in range(1, 17))       # Gower D = 40: no P fits
    assert OL.lds_lml_grad(39, True, 1) <= LIMIT < OL.lds_lml_grad(39, True, 2)
    assert OL.lds_sparse_grad(64, 16) == 147456
    # the cases the issue sets
    ids = {c.id: (c.D, c.P, c.gower, c.grad) for c in OL.TABLE}
    assert ids["D64P15"] == (64, 15, False, "yes") and ids["D63P16"] == (63, 16, False, "yes") and ids["D64P16"] == (64, 16, False, "lds")
    assert ids["G39P1"] == (39, 1, True, "yes") and ids["G39P2"] == (39, 2, True, "lds") and ids["G40P1"] == (40, 1, True, "lds")
    assert [OL.CASES[i].P for i in OL.OUTPUT_IDS] == [128, 127, 17, 16, 4]
    assert all(OL.CASES[i].D == 3 and OL.CASES[i].N == 130 and set(OL.CASES[i].fams) == set(OL.ALL_FAMILIES) for i in OL.OUTPUT_IDS)
    assert [(c.Mz, c.N, c.P, c.grad) for c in OL.SPARSE] == [(130, 300, 16, True), (130, 300, 17, False), (130, 300, 128, False)]


# ---- the targets ------------------------------------------------------------------------------------------------------------------
def _all_targets():
    for c in OL.TABLE:
        yield c.id, OL.problem(c.id)[1], c.P
    for c in OL.SPARSE:
        yield c.id, OL.sparse_problem(c.id)[1], c.P


def test_targets_have_full_rank_and_no_affine_copies():
    """Full column rank with the columns brought to unit length (the scales alone span 64 : 1), and no column an affine image of
    another: |correlation| = 1 for an affine copy; two copies of ONE signal under their own 0.1 noise would have 0.98 (signal
    power 1/2 over 1/2 + 0.01), so 0.95 says the signals themselves differ."""
    for cid, Y, P in _all_targets():
        assert Y.shape[1] == P
        top = np.max(np.abs(Y), axis=0)
        s = OL.scales(P)
        assert np.all(top > 0.5 * s) and np.all(top < 1.5 * s)                 # the scale of every column is the table's
        sv = np.linalg.svd(Y / np.linalg.norm(Y, axis=0), compute_uv=False)
        worst = 0.0
        if P > 1:
            cc = np.corrcoef(Y.T) - np.eye(P)
            worst = float(np.max(np.abs(cc)))
        print("%-7s P %3d: smallest singular value %.3e, largest |correlation| %.3f" % (cid, P, sv[-1], worst))
        assert np.linalg.matrix_rank(Y) == P and sv[-1] > 1e-3
        assert worst <= 0.95


# ---- the exact model's oracle against a long-double truth -------------------------------------------------------------------------
def _truth(fam, cid):
    """lml, alpha, posterior mean / variance at the first five candidates and -- where the case takes gradients -- the hyper-
    gradients, in long double: the kernel in long double for the plain cases (tests/_sparse_ref.Kern), the oracle's float64
    Gower K carried over for the Gower ones (the factorisation and the solves are what is measured there)."""
    c = OL.CASES[cid]
    X, Y, Xs, ls = OL.problem(cid)
    gp = OL.oracle(fam, cid)
    Xs = Xs[:5]
    kern = SR.Kern(fam, c.D, OL.variance_of(cid), ls, True, LD)
    if c.gower:
        K, Kx = gp.kern.K(X).astype(T), gp.kern.K(X, Xs).astype(T)
    else:
        K, Kx = kern.K(X.astype(T)), kern.K(X.astype(T), Xs.astype(T))
    A = K + np.eye(c.N, dtype=T) * (T(OL.NOISE) + T(1e-8))
    L, _ = LD.chol(A)
    Yl = Y.astype(T)
    alpha = LD.solve(L, LD.solve(L, Yl, 0), 1)
    logdet = 2 * np.sum(np.log(np.diag(L)))
    lml = T(0.5) * (-c.N * c.P * np.log(2 * (np.arctan(T(1)) * 4)) - c.P * logdet - np.sum(alpha * Yl))
    t = LD.solve(L, Kx, 0)
    var = T(OL.variance_of(cid)) - np.sum(t * t, 0) + T(OL.NOISE)
    out = dict(lml=lml, alpha=alpha, mean=Kx.T @ alpha, var=var)
    if c.grad == "yes":
        Wi = LD.solve(L, LD.solve(L, np.eye(c.N, dtype=T), 0), 1)
        dL_dK = T(0.5) * (alpha @ alpha.T - c.P * Wi)
        dv, dl = kern.update_gradients_full(dL_dK, X.astype(T))
        if c.gower:        # the fork's pairing: the Gower K weighs the variance gradient (stationary.py:224)
            dv = np.sum(K * dL_dK) / T(OL.variance_of(cid))
        out.update(dv=dv, dl=dl, dn=np.trace(dL_dK))
    return out


@pytest.mark.parametrize("fam,cid", OL.PAIRS, ids=lambda v: str(v))
def test_oracle_against_a_long_double_truth(fam, cid):
    c = OL.CASES[cid]
    gp, tr = OL.oracle(fam, cid), _truth(fam, cid)
    p = gp.posterior
    assert p["jitter"] == 0.0
    Xs = OL.problem(cid)[2][:5]
    mu, var = gp.predict(Xs)
    e = dict(lml=abs(p["lml"] - float(tr["lml"])) / abs(float(tr["lml"])), alpha=OL.col_err(p["alpha"], tr["alpha"]),
             mean=OL.col_err(mu, tr["mean"]), var=float(np.max(np.abs(var[:, 0] - tr["var"]) / np.abs(tr["var"]))))
    if c.grad == "yes":
        dv, dl, dn = gp.gradients()
        scale = max(abs(float(tr["dv"])), float(np.max(np.abs(tr["dl"]))), 1.0)
        e["grad"] = max(abs(dv - float(tr["dv"])), float(np.max(np.abs(dl - tr["dl"])))) / scale
        e["dnoise"] = abs(dn - float(tr["dn"])) / max(abs(float(tr["dn"])), 1.0)
    print("%-11s %-7s " % (fam, cid) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e.pop("lml") <= 1e-9
    assert all(v <= 1e-7 for v in e.values()), e


# ---- the sparse model's oracle against the long-double one -------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", OL.SPARSE_PAIRS, ids=lambda v: str(v))
def test_sparse_oracle_against_a_long_double_truth(fam, cid):
    c = OL.SPARSE_CASES[cid]
    X, Y, Z, Xs, ls = OL.sparse_problem(cid)
    fit = {}
    for lin in (SR.F64, LD):
        f = SR.inference(fam, X, Z, Y, OL.VAR, ls, True, OL.SPARSE_NOISE, lin, grads=c.grad)
        assert f["jitter_kmm"] == 0.0 and f["jitter_b"] == 0.0
        f["pred"] = SR.predict(f, Z, Xs[:5], OL.SPARSE_NOISE, True, lin, grads=False)
        fit[lin] = f
    a, b = fit[SR.F64], fit[LD]
    e = dict(lml=abs(float(a["lml"] - b["lml"])) / abs(float(b["lml"])), w=OL.col_err(a["woodbury_vector"], b["woodbury_vector"]),
             mean=OL.col_err(a["pred"][0], b["pred"][0]), var=float(np.max(np.abs(a["pred"][1] - b["pred"][1]) / np.abs(b["pred"][1]))))
    if c.grad:
        scale = max(abs(float(b["dvariance"])), float(np.max(np.abs(b["dlengthscale"]))), 1.0)
        e["grad"] = max(abs(float(a["dvariance"] - b["dvariance"])), float(np.max(np.abs(a["dlengthscale"] - b["dlengthscale"])))) / scale
        e["dnoise"] = abs(float(a["dnoise"] - b["dnoise"])) / max(abs(float(b["dnoise"])), 1.0)
        e["dZ"] = float(np.max(np.abs(a["dZ"] - b["dZ"]))) / float(np.max(np.abs(b["dZ"])))
    print("%-11s %-5s " % (fam, cid) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e.pop("lml") <= 1e-9
    assert all(v <= 1e-7 for v in e.values()), e
