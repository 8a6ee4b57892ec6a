"""GPU: ``gp_append`` -- observations appended to a fitted GP, the factor grown in O(k N^2) -- against the CPU oracle FITTED TO
THE GROWN DATA (never a device refit), at the bounds tests/test_gpu_random_shapes.py holds a fresh device fit to: LML within
1e-8 max(1, |lml|); alpha, mean, variance, predictive gradients, fmin and EI / LCB / MPI within 1e-6; the EI gradient of the rows
call within 1e-5; ``gp_get_chol`` within 1e-6 max|L|.  Inputs: noise 1e-2, uniform X in the unit box, the lengthscales of that
file -- cond(Ky) <= 5e4 (tests/test_append_host.py), so the oracle is good to ~1e-11 there.

Shapes (tests/_append_cases.py): in place (100, 1), (100, 8), (120, 8); a new tile (128, 1), (256, 5); split across the boundary
(120, 9), (250, 28); two tiles of history with a 9-row border (300, 9).  Each runs with the explicit inverse factor valid before
the append (``rows_build`` 1 and one ``predict_rows`` call: the factor is extended, and the gradient ``acq_rows`` call after the
append is served fused) and without it (``rows_build`` 0).  One more shape, (2100, 9), takes the streaming kernels past their
1024-row / 1024-column chunks, which the shapes above never leave.

The non-positive pivot: an input whose border pivot is <= 0 in fp64 reproducibly on both sides was not found -- with the 1e-8 the
diagonal always gets, coincident rows at noise 0 leave a pivot of +1e-8 .. 2e-8 whose sign is decided by rounding of order
cond eps ~ 1e-8 -- so that case is left out.  The positive return, the untouched context (the split's undo included) and the model's
fall-back to the refit are exercised with a border that is not FINITE instead (a NaN coordinate), which the entry point reports
the same way.  (With a slightly NEGATIVE noise the pivot of a repeated row is -2 delta, away from rounding: that finite border, and
appends to a fit that needed jitter, are in tests/test_gpu_jitter_routes.py.)
"""
import json
import os

import numpy as np
import pytest

import _append_cases as C
import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

NOISE = 1e-2
ACQS = ((_lib.GP_ACQ_EI, 0.01, O.acq_EI), (_lib.GP_ACQ_LCB, 2.0, O.acq_LCB), (_lib.GP_ACQ_MPI, 0.01, O.acq_MPI))


def relmax(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, np.max(np.abs(b)))


def fitted_handle(X, Y, kid, ard, var, ls, noise, Xs, rows_build, warm=True):
    """A handle fitted to (X, Y) with the candidates resident and, ``warm``, every cache an append must drop filled: Ky^-1, the
    candidates' posterior, fmin, the LML gradient's products; with ``rows_build`` 1 the explicit inverse factor as well."""
    h = _lib.Handle(0)
    h.set_option("rows_build", rows_build)
    h.set_data(X, Y)
    h.set_params(kid, ard, var, ls, noise)
    h.set_candidates(Xs)
    h.fit()
    if warm:
        h.woodbury_inv()
        h.predict(True)
        if Y.shape[1] == 1:
            h.fmin()
        h.lml_grad(ls.size)
    if rows_build == 1 and Y.shape[1] == 1:
        h.predict_rows(Xs[:1], True)
    return h


def check_against_oracle(h, gp, Xs, nls, P, fused_expected=None):
    """Everything the handle serves after an append against the oracle ``gp`` of the grown data; the candidates ``Xs`` are
    still resident (set_candidates is NOT called again)."""
    p = gp.posterior
    lml, logdet, jit = h.fit_state()
    print("lml %.3e logdet %.3e alpha %.3e" % (abs(lml - p["lml"]) / max(1.0, abs(p["lml"])), abs(logdet - p["logdet"]),
                                              relmax(h.alpha(), p["alpha"])))
    assert jit == 0.0
    assert abs(lml - p["lml"]) <= 1e-8 * max(1.0, abs(p["lml"]))
    assert abs(logdet - p["logdet"]) <= 1e-8 * max(1.0, abs(p["logdet"]))
    assert relmax(h.alpha(), p["alpha"]) < 1e-6
    L = h.chol()
    assert L.shape == p["L"].shape and np.max(np.abs(L - p["L"])) < 1e-6 * np.max(np.abs(p["L"]))
    Wi = h.woodbury_inv()
    assert np.max(np.abs(Wi - p["Wi"])) < 1e-6 * np.max(np.abs(p["Wi"]))
    mu, v = h.predict(True)
    m0, v0 = gp.predict(Xs)
    assert mu.shape == m0.shape
    assert relmax(mu, m0) < 1e-6 and np.max(np.abs(v - v0) / np.abs(v0)) < 1e-6
    mu2, v2 = h.predict(False)
    m1, v1 = gp.predict_noiseless(Xs)
    assert relmax(mu2, m1) < 1e-6 and np.max(np.abs(v2 - v1)) < 1e-6 * max(1.0, np.max(np.abs(v1))) + 1e-9
    dv, dl, dn = h.lml_grad(nls)
    r = gp.gradients()
    sc = max(1.0, abs(r[0]), np.max(np.abs(r[1])), abs(r[2]))
    assert abs(dv - r[0]) < 1e-6 * sc and np.max(np.abs(dl - r[1])) < 1e-6 * sc and abs(dn - r[2]) < 1e-6 * sc
    if P != 1:
        mr, vr = h.predict_rows(Xs[:3], True)
        assert relmax(mr, m0[:3]) < 1e-6 and np.max(np.abs(vr - v0[:3]) / np.abs(v0[:3])) < 1e-6
        return
    dm, dvx = h.predict_grad()
    dm0, dv0 = gp.predictive_gradients(Xs)
    assert np.max(np.abs(dm - dm0)) < 1e-6 * max(1.0, np.max(np.abs(dm0)))
    assert np.max(np.abs(dvx - dv0)) < 1e-6 * max(1.0, np.max(np.abs(dv0)))
    model = O.OracleGPModel(gp)
    f0 = model.get_fmin()
    fmin = h.fmin()
    assert abs(fmin - f0) <= 1e-6 * max(1.0, abs(f0))
    for t, par, fn in ACQS:
        a0 = O.acquisition_function(fn(model, Xs, par) if fn is O.acq_LCB else fn(model, Xs, par, f0))
        a = h.acq(t, par, fmin)
        assert np.max(np.abs(a - a0)) < 1e-6 * max(1.0, np.max(np.abs(a0)))
    before = h.rows_stats()
    for k in (1, 3, 5):
        xs = Xs[:k]
        mr, vr, dmr, dvr = h.predict_rows(xs, True, grad=True)
        assert relmax(mr, m0[:k]) < 1e-6 and np.max(np.abs(vr - v0[:k]) / np.abs(v0[:k])) < 1e-6
        assert np.max(np.abs(dmr - dm0[:k])) < 1e-6 * max(1.0, np.max(np.abs(dm0)))
        assert np.max(np.abs(dvr - dv0[:k])) < 1e-6 * max(1.0, np.max(np.abs(dv0)))
        a0, da0 = O.acq_EI_withGradients(model, xs, 0.01, f0)
        ar, dar = h.acq_rows(xs, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
        assert np.max(np.abs(ar + a0)) < 1e-6 * max(1.0, np.max(np.abs(a0)))
        assert np.max(np.abs(dar + da0)) < 1e-5 * max(1.0, np.max(np.abs(da0)))
    after = h.rows_stats()
    if fused_expected:      # the extended inverse factor serves the gradient calls: fused, never the batched route
        assert after["fused"] == before["fused"] + 6 and after["fallback"] == before["fallback"]


def _shape_cases():
    out = []
    for i, ((N0, k), want) in enumerate(C.SHAPES):
        for rb in (1, 0):
            kname, kid, ard = C.KERNELS[(2 * i + rb) % len(C.KERNELS)]
            out.append((N0, k, want, 2 if (i + rb) % 2 else 5, 1, kname, kid, ard, rb))
    # two outputs (the inverse factor's path takes P = 1 only: these go through the substitution against L)
    for i, ((N0, k), want) in enumerate(C.SHAPES[2::2]):
        kname, kid, ard = C.KERNELS[(i + 3) % len(C.KERNELS)]
        out.append((N0, k, want, 5 if i % 2 else 2, 2, kname, kid, ard, i % 2))
    return out


@pytest.mark.parametrize("case", _shape_cases(), ids=lambda c: "N%d+%d-D%d-P%d-%s%s-rb%d" % (c[0], c[1], c[3], c[4], c[5],
                                                                                            "-ard" if c[7] else "", c[8]))
def test_append_matches_the_oracle_of_the_grown_data(case):
    N0, k, want, D, P, kname, kid, ard, rb = case
    X, Y, Xs, ls, var, kern = C.problem(31 * N0 + k + rb, N0 + k, D, P, kname, ard)
    Y0 = 0.5 * Y[:N0] + 0.3        # the BO loop re-normalises: EVERY target changes with the append, not only the tail
    h = fitted_handle(X[:N0], Y0, kid, ard, var, ls, NOISE, Xs, rb)
    try:
        s0 = h.append_stats()
        lml, logdet = h.append(X[N0:], Y)
        s1 = h.append_stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (want[0], want[1], 0)
        assert h.N == N0 + k and (lml, logdet) == h.fit_state()[:2]
        gp = O.OracleGP(X, Y, kern, NOISE)
        check_against_oracle(h, gp, Xs, ls.size, P, fused_expected=(rb == 1 and P == 1))
    finally:
        h.close()


@pytest.mark.parametrize("rb", (1, 0))
def test_append_beyond_one_chunk_of_the_streaming_kernels(rb):
    """N0 = 2100, k = 9: the column sums of L21 Li11 run over three 1024-row chunks (strips from column 1024 on start in the
    second, from 2048 on in the third), the Gram over three 1024-column chunks, and the nine rows take two passes -- the paths
    the small shapes above never reach.  cond(Ky) grows with N (~2e5 here): still five orders inside the bounds."""
    N0, k = 2100, 9
    X, Y, Xs, ls, var, kern = C.problem(2100 + rb, N0 + k, 5, 1, "Mat52", True)
    h = fitted_handle(X[:N0], 0.5 * Y[:N0] + 0.3, 1, True, var, ls, NOISE, Xs, rb)
    try:
        h.append(X[N0:], Y)
        assert h.append_stats() == (1, 0, 0)
        check_against_oracle(h, O.OracleGP(X, Y, kern, NOISE), Xs, ls.size, 1, fused_expected=(rb == 1))
    finally:
        h.close()


def test_gower_append():
    """The mixed-variable configuration of tests/test_gpu_gower.py (its fixture's inputs, domain and hyper-parameters): five
    rows appended under 95, against the oracle's Gower model of all 100."""
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "gp_gower.npz"))
    dom = json.loads(str(G["domain_json"]))
    for d in dom:
        d["domain"] = tuple(d["domain"])
    tag = "G_N100_M40_s3_Mat52_n0.01"
    g = lambda name: G[tag + "/" + name]
    X, Y, Xs, ls, var, noise = g("X"), g("Y"), g("Xs"), g("lengthscale"), float(g("variance")), float(g("noise"))
    space = gpo.Design_space(dom)
    for rb in (1, 0):
        k = gpo.kern.Matern52(6, variance=var, lengthscale=ls, ARD=True, Gower=True, space=space)
        m = gpo.models.GPRegression(X[:95], Y[:95] * 0.7 - 0.1, k, noise_var=noise)
        m._h.set_option("rows_build", rb)
        m.predict(Xs)
        if rb:
            m._h.predict_rows(Xs[:1], True)
        m.append_XY(X[95:], Y)
        assert m._h.append_stats() == (1, 0, 0) and not m._dirty
        gp = O.OracleGP(X, Y, O.make_kernel("Mat52", 6, var, ls, ARD=True, Gower=True, space=O.MixedSpace(dom)), noise)
        assert abs(m.log_likelihood() - gp.log_likelihood()) <= 1e-8 * max(1.0, abs(gp.log_likelihood()))
        assert abs(gp.log_likelihood() - float(g("lml"))) <= 1e-8 * abs(float(g("lml")))      # (the fixture's own record agrees)
        mu, v = m.predict(Xs)
        m0, v0 = gp.predict(Xs)
        assert relmax(mu, m0) < 1e-6 and np.max(np.abs(v - v0) / np.abs(v0)) < 1e-6
        dm, dv = m.predictive_gradients(Xs[:5])
        dm0, dv0 = gp.predictive_gradients(Xs[:5])
        assert np.max(np.abs(dm - dm0)) < 1e-6 * max(1.0, np.max(np.abs(dm0)))
        assert np.max(np.abs(dv - dv0)) < 1e-6 * max(1.0, np.max(np.abs(dv0)))
        assert np.max(np.abs(m._h.chol() - gp.posterior["L"])) < 1e-6 * np.max(np.abs(gp.posterior["L"]))
        m.close()


# ---- chains ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rb", (1, 0))
def test_chain_of_appends(rb):
    """126 + 1 (in place) + 4 (split) + 125 (in place, fills the tile: sixteen passes of eight rows) + 3 (a new tile), the
    oracle of the data so far after each."""
    steps = (1, 4, 125, 3)
    N0, D = 126, 2
    X, Y, Xs, ls, var, kern = C.problem(99 + rb, N0 + sum(steps), D, 1, "Mat52", True)
    h = fitted_handle(X[:N0], Y[:N0], 1, True, var, ls, NOISE, Xs, rb)
    try:
        n, want = N0, [0, 0]
        for k in steps:
            a, b = C.routes(n, k)
            want[0] += a
            want[1] += b
            n += k
            Yn = Y[:n] * (1.0 + 0.01 * n)
            h.append(X[n - k:n], Yn)
            assert h.append_stats() == (want[0], want[1], 0)
            check_against_oracle(h, O.OracleGP(X[:n], Yn, kern, NOISE), Xs, ls.size, 1, fused_expected=(rb == 1))
        assert tuple(want) == (3, 2)
    finally:
        h.close()


def test_append_refit_append():
    """append, then other hyper-parameters and a fit of the grown data, then append again."""
    X, Y, Xs, ls, var, kern = C.problem(5, 140, 5, 1, "rbf", False)
    h = fitted_handle(X[:120], Y[:120], 0, False, var, ls, NOISE, Xs, 1)
    try:
        h.append(X[120:126], Y[:126])
        check_against_oracle(h, O.OracleGP(X[:126], Y[:126], kern, NOISE), Xs, 1, 1, fused_expected=True)
        ls2, var2 = ls * 1.3, var * 0.8
        h.set_params(0, False, var2, ls2, 2 * NOISE)
        h.fit()
        h.append(X[126:140], Y)      # 126 + 14 crosses into a new tile; no inverse factor this time (the fit dropped it)
        assert h.append_stats() == (2, 1, 0)
        import _kernel_families as KF
        check_against_oracle(h, O.OracleGP(X, Y, KF.make("rbf", 5, var2, ls2, False), 2 * NOISE), Xs, 1, 1)
    finally:
        h.close()


def test_append_after_fit_predict():
    X, Y, Xs, ls, var, kern = C.problem(6, 260, 2, 1, "Mat32", False)
    h = _lib.Handle(0)
    try:
        h.set_data(X[:250], Y[:250])
        h.set_params(2, False, var, ls, NOISE)
        h.set_candidates(Xs)
        h.fit_predict(True)
        h.append(X[250:], Y)
        assert h.append_stats() == (1, 1, 0)
        check_against_oracle(h, O.OracleGP(X, Y, kern, NOISE), Xs, 1, 1)
    finally:
        h.close()


# ---- stress, determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rb", (1, 0))
def test_stress_noise_1e6(rb):
    """exact_feval's noise 1e-6, N0 = 200, k = 5: cond(Ky) ~ 1e8 (tests/test_append_host.py), so either side carries
    cond eps ~ 3e-8; the variance is held to the absolute criterion of tests/test_gpu_random_shapes.py:88, the mean to 1e-6."""
    X, Y, Xs, ls, var, kern = C.problem(4242, 205, 2, 1, "Mat52", False)
    Y = np.sin(3 * X[:, :1]) + X[:, 1:2] ** 2      # a smooth objective, as exact_feval means it
    h = fitted_handle(X[:200], Y[:200], 1, False, var, ls, 1e-6, Xs, rb)
    try:
        assert h.fit_state()[2] == 0.0
        h.append(X[200:], Y)
        gp = O.OracleGP(X, Y, kern, 1e-6)
        assert gp.posterior["jitter"] == 0.0
        for noise_on in (True, False):
            mu, v = h.predict(noise_on)
            m0, v0 = gp.predict(Xs, include_likelihood=noise_on)
            print("stress rb=%d noise=%d: mean %.3e var %.3e" % (rb, noise_on, relmax(mu, m0), np.max(np.abs(v - v0))))
            assert relmax(mu, m0) < 1e-6
            assert np.max(np.abs(v - v0)) < 1e-6 * max(1.0, np.max(np.abs(v0))) + 1e-9
    finally:
        h.close()


@pytest.mark.parametrize("rb", (1, 0))
def test_same_sequence_same_bits(rb):
    X, Y, Xs, ls, var, kern = C.problem(77, 140, 5, 1, "rbf", True)
    got = []
    for _ in range(2):
        h = fitted_handle(X[:120], Y[:120], 0, True, var, ls, NOISE, Xs, rb)
        h.append(X[120:129], Y[:129])        # split
        h.append(X[129:140], Y)              # in place
        got.append((h.alpha(), h.chol(), h.fit_state()))
        h.close()
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes() and got[0][2] == got[1][2]


# ---- refusals and the positive return ---------------------------------------------------------------------------------------------
def _raw_append(h, Xn, k, Yall):
    return h.lib.gp_append(h.h, _lib.dptr(Xn), k, _lib.dptr(Yall), None, None)


def _state(h):
    """fit state, alpha and L, and the row count the library itself writes (a sentinel behind alpha's N rows stays)."""
    buf = np.full((h.N + 4, h.P), -7.0)
    _lib.check(h.lib, h.lib.gp_get_alpha(h.h, _lib.dptr(buf)), "gp_get_alpha")
    assert np.all(buf[h.N:] == -7.0)
    return h.fit_state(), buf.tobytes(), h.chol().tobytes()


def test_refusals_leave_the_context_untouched():
    X, Y, Xs, ls, var, kern = C.problem(8, 110, 2, 1, "rbf", False)
    Xn, Yall = np.ascontiguousarray(X[100:]), np.ascontiguousarray(Y)
    h = _lib.Handle(0)
    try:
        h.set_data(X[:100], Y[:100])
        h.set_params(0, False, var, ls, NOISE)
        assert _raw_append(h, Xn, 10, Yall) == _lib.GP_ERR_STATE          # before any fit
        h.fit()
        s = _state(h)
        assert _raw_append(h, Xn, 0, Yall) == _lib.GP_ERR_ARG
        big = np.zeros((129, 2))
        assert _raw_append(h, big, 129, np.zeros((229, 1))) == _lib.GP_ERR_ARG
        assert _state(h) == s
        with pytest.raises(ValueError):
            h.append(np.zeros((129, 2)), np.zeros((229, 1)))
        assert h.N == 100 and h.append_stats() == (0, 0, 4)
        # an output warp: its fit is a fit of f(Y)
        h.set_output_warp([[1.0, 0.5, 0.1]], 1.0)
        h.fit()
        s = _state(h)
        assert _raw_append(h, Xn, 10, Yall) == _lib.GP_ERR_STATE
        assert _state(h) == s and h.append_stats() == (0, 0, 5)
        h.set_output_warp(None)      # the warp off again: the handle appends as any other
        h.set_candidates(Xs)
        h.fit()
        h.append(Xn, Yall)
        check_against_oracle(h, O.OracleGP(X, Y, kern, NOISE), Xs, 1, 1)
    finally:
        h.close()


@pytest.mark.parametrize("rb", (1, 0))
@pytest.mark.parametrize("N0,k,bad", [(100, 3, 1), (120, 9, 8), (128, 2, 0)], ids=["in-place", "second-border", "new-tile"])
def test_border_that_is_not_finite_returns_positive_and_changes_nothing(N0, k, bad, rb):
    """A NaN coordinate in new row ``bad``: a positive return, nothing of the context overwritten -- for the split append
    (120, 9) the NaN sits in the SECOND border, after the first was committed and has to be taken back -- and the handle
    goes on: the clean append afterwards matches the oracle."""
    X, Y, Xs, ls, var, kern = C.problem(9 + N0, N0 + k, 2, 1, "Mat52", False)
    h = fitted_handle(X[:N0], Y[:N0], 1, False, var, ls, NOISE, Xs, rb)
    try:
        s = _state(h)
        rows0 = h.predict_rows(Xs[:2], True, grad=True)
        Xn = X[N0:].copy()
        Xn[bad, 0] = np.nan
        rc = _raw_append(h, Xn, k, np.ascontiguousarray(Y))
        assert rc > 0 and N0 < rc <= N0 + k
        with pytest.raises(np.linalg.LinAlgError):
            h.append(Xn, Y)
        assert h.N == N0 and _state(h) == s and h.append_stats() == (0, 0, 2)
        rows1 = h.predict_rows(Xs[:2], True, grad=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rows0, rows1))
        h.append(X[N0:], Y)
        check_against_oracle(h, O.OracleGP(X, Y, kern, NOISE), Xs, 1, 1)
    finally:
        h.close()


# ---- model level ---------------------------------------------------------------------------------------------------------------------
def test_gpregression_append_xy():
    X, Y, Xs, ls, var, kern = C.problem(10, 135, 2, 1, "Mat52", False)
    Y = 3.0 + 2.0 * Y
    m = gpo.models.GPRegression(X[:120], Y[:120], gpo.kern.Matern52(2, variance=var, lengthscale=ls), noise_var=NOISE, normalizer=True)
    try:
        m.predict(Xs)
        m.append_XY(X[120:130], Y[:130])         # 10 rows across the tile boundary, the normaliser's mean and scale move
        assert m._h.append_stats() == (1, 1, 0) and not m._dirty
        assert m.X.shape == (130, 2) and m.Y.shape == (130, 1) and m.num_data == 130
        gp = O.OracleGP(X[:130], Y[:130], kern, NOISE, normalizer=True)
        assert np.array_equal(m.Y_normalized, gp.Y_normalized)
        assert abs(m.log_likelihood() - gp.log_likelihood()) <= 1e-8 * max(1.0, abs(gp.log_likelihood()))
        mu, v = m.predict(Xs)
        m0, v0 = gp.predict(Xs)
        assert relmax(mu, m0) < 1e-6 and np.max(np.abs(v - v0) / np.abs(v0)) < 1e-6
        # dirty after a parameter change: exactly the set_XY route
        m.kern.variance[:] = var * 1.5
        assert m._dirty
        m.append_XY(X[130:], Y)
        assert m._h.append_stats() == (1, 1, 0) and m._dirty and m.X.shape == (135, 2)
        import _kernel_families as KF
        gp = O.OracleGP(X, Y, KF.make("Mat52", 2, var * 1.5, ls, False), NOISE, normalizer=True)
        assert abs(m.log_likelihood() - gp.log_likelihood()) <= 1e-8 * max(1.0, abs(gp.log_likelihood()))
        mu, v = m.predict(Xs)
        m0, v0 = gp.predict(Xs)
        assert relmax(mu, m0) < 1e-6 and np.max(np.abs(v - v0) / np.abs(v0)) < 1e-6
        # a border that is not finite lands on the refit (which then fails as the reference's does: jitchol on NaN)
        bad = np.full((1, 2), np.nan)
        m.predict(Xs)
        with pytest.raises(np.linalg.LinAlgError):
            m.append_XY(bad, np.vstack([Y, [[0.0]]]))
            m.log_likelihood()
        assert m._h.append_stats()[2] == 1 and m.X.shape == (136, 2)
    finally:
        m.close()


def test_gpmodel_incremental():
    X, Y, Xs, ls, var, kern = C.problem(11, 131, 2, 1, "Mat52", False)
    gm = gpo.GPModel(kernel=gpo.kern.Matern52(2, variance=var, lengthscale=ls), noise_var=NOISE, max_iters=0, incremental=True,
                     verbose=False)
    try:
        n = 120
        gm.updateModel(X[:n], Y[:n], None, None)
        gm.predict(Xs)
        stats = (0, 0, 0)
        for k, route in ((3, (1, 0)), (6, (1, 1)), (2, (1, 0))):
            n += k
            gm.updateModel(X[:n], Y[:n], None, None)
            stats = (stats[0] + route[0], stats[1] + route[1], 0)
            assert gm.model._h.append_stats() == stats
            om = O.OracleGPModel(O.OracleGP(X[:n], Y[:n], kern, NOISE))
            mu, sd = gm.predict(Xs)
            m0, s0 = om.predict(Xs)
            assert relmax(mu, m0) < 1e-6 and relmax(sd, s0) < 1e-6
            assert abs(gm.get_fmin() - om.get_fmin()) <= 1e-6 * max(1.0, abs(om.get_fmin()))
            _, _, dm, ds = gm.predict_withGradients(Xs[:4])
            _, _, dm0, ds0 = om.predict_withGradients(Xs[:4])
            assert np.max(np.abs(dm - dm0)) < 1e-6 * max(1.0, np.max(np.abs(dm0)))
            assert np.max(np.abs(ds - ds0)) < 1e-6 * max(1.0, np.max(np.abs(ds0)))
        # a head that differs in ONE bit is other data: the refit route
        Xb = X.copy()
        Xb[7, 1] = np.nextafter(Xb[7, 1], 2.0)
        gm.updateModel(Xb, Y, None, None)
        assert gm.model._h.append_stats() == stats and gm.model._dirty
        om = O.OracleGPModel(O.OracleGP(Xb, Y, kern, NOISE))
        mu, sd = gm.predict(Xs)
        m0, s0 = om.predict(Xs)
        assert relmax(mu, m0) < 1e-6 and relmax(sd, s0) < 1e-6
    finally:
        gm.model.close()


def test_bayesian_optimization_incremental_suggests_the_same_locations():
    """Three iterations on a 2-D quadratic from 20 points with the hyper-parameters kept: the appended and the refitted model
    suggest the same locations (a consistency check between two device runs, on top of the oracle checks above)."""
    dom = [{'name': 'x', 'type': 'continuous', 'domain': (-1.0, 1.0), 'dimensionality': 2}]
    f = lambda x: np.sum((np.atleast_2d(x) - 0.3) ** 2, axis=1, keepdims=True)
    X0 = np.random.default_rng(12).uniform(-1, 1, (20, 2))
    runs = []
    for inc in (False, True):
        np.random.seed(12)
        bo = gpo.BayesianOptimization(f=f, domain=dom, X=X0, Y=f(X0), acquisition_type='EI', max_iters=0, incremental=inc,
                                      exact_feval=False)
        bo.run_optimization(max_iter=3, eps=-1.0)
        runs.append(bo.X[20:].copy())
        stats = bo.model.model._h.append_stats()
        assert stats == ((3, 0, 0) if inc else (0, 0, 0))
        bo.model.model.close()
    print("suggested, refit:\n", runs[0], "\nappended:\n", runs[1], "\nmax diff %.3e" % np.max(np.abs(runs[0] - runs[1])))
    assert runs[0].shape == (3, 2) and np.max(np.abs(runs[0] - runs[1])) < 1e-6
