"""GPU: ``gp_fit_grad_x_batch`` and ``gp_fit_grad_warp_batch`` -- R members against the single call one member at a time
(``set_data(Xw[r], Y)`` + ``fit_grad_x``; ``fit_grad_warp``), position and company, the jitter ladder per member, the untouched
resident state, the refusals, one oracle case per entry, and ``optimize_restarts(parallel=True)`` of ``InputWarpedGP`` /
``WarpedGP`` against their serial restarts.

Rule of ``test_members_equal_the_single_call``.  Where Npad <= 768 the single call takes the single-stream route the batch
mirrors: lml, log det, jitter, every gradient, dL_dX / dpsi / dd / log_jacobian are THE SAME BITS.  Above (N = 770, 2048) the
single call factors with look-ahead and the rule is ``_close`` of tests/test_gpu_fit_grad_batch.py: the head within 1e-12
relative, every gradient entry within 1e-12 of the member's largest, dL_dX within 1e-12 of the member's largest |dL_dX| (it sums
the same Ky^-1 entries).  The log-Jacobian never depends on the route: the same bits at every size.  (Measured on an MI355X with
the default options: every member of the N = 770 and N = 2048 cases came out with the single call's bits as well -- all printed
differences 0 -- so the 1e-12 rule has not been needed yet and no wider one was derived.)

Shapes, the smallest at which each branch can go wrong: N = 1, 2, 127, 128, 129, 300 (one tile and its edges, three tiles);
770 (seven tiles, two panels: the first size off the bitwise rule); 2048 (the cap; a second chunk of column tiles in gradx at
five tiles and above).  D = 1, 3, 17 (a second pass of 16 dimensions in gradx and in the ARD sums); R = 1, 2, 5, 64; P = 1 and 3
for the x-batch; the four families, ARD on and off; T = 1, 3, 8 warp terms.  The members of the x-batch are Kumaraswamy warps of
one base X with exponents over 0.3 .. 3, the last one collapsing rows 0 and 1 onto the same point (tests/_warped_batch_cases.py).
Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

import gaussian_process_optimization_amd as gpo
from gaussian_process_optimization_amd import _lib
from gaussian_process_optimization_amd.warping_functions import IdentityFunction

import _warped_batch_cases as C

pytestmark = pytest.mark.gpu

KID = {f: i for i, f in enumerate(C.FAMILIES)}


@pytest.fixture(scope="module")
def h():
    hh = _lib.Handle(0)
    yield hh
    hh.close()


def _load(h, X, Y):
    """New data on the shared handle, with no output warp and no Gower set-up left over from an earlier test."""
    if getattr(h, "N", None) is not None:
        h.set_output_warp(None)
    h.set_data(X, Y)
    h.set_gower()


def _npad(N):
    return -(-N // 128) * 128


# ---- single-member references -------------------------------------------------------------------------------------------------
def _single_x(h, fam, ard, Xw, Y, var, ls, noise, maxtries=5):
    """(head [lml, logdet, jitter], grads [dv, dl.., dn], dL_dX) of one member alone, or None where it is not positive definite."""
    h.set_data(Xw, Y)
    h.set_params(KID[fam], ard, var, ls, noise)
    try:
        fit, (dv, dl, dn), dX = h.fit_grad_x(ls.size, maxtries)
    except np.linalg.LinAlgError:
        return None
    return np.array(fit), np.r_[dv, dl, dn], dX


def _batch_x(res, r):
    (lml, logdet, jit), (dv, dl, dn), dX, _ = res
    return np.array([lml[r], logdet[r], jit[r]]), np.r_[dv[r], dl[r], dn[r]], dX[r]


def _single_w(h, fam, ard, var, ls, noise, psi, d, maxtries=5):
    """(head [lml, logdet, jitter, log_jacobian], grads [dv, dl.., dn, dpsi.., dd]) of one member alone, or None."""
    h.set_params(KID[fam], ard, var, ls, noise)
    try:
        fit, (dv, dl, dn), lj, (dpsi, dd) = h.fit_grad_warp(psi, d, ls.size, maxtries)
    except np.linalg.LinAlgError:
        return None
    return np.r_[fit, lj], np.r_[dv, dl, dn, dpsi.ravel(), dd]


def _batch_w(res, r):
    (lml, logdet, jit), (dv, dl, dn), lj, (dpsi, dd), _ = res
    return np.r_[lml[r], logdet[r], jit[r], lj[r]], np.r_[dv[r], dl[r], dn[r], dpsi[r].ravel(), dd[r]]


def _report(what, r, got, ref):
    parts = []
    for name, a, b in zip(("head", "grad", "dL_dX"), got, ref):
        s = max(float(np.max(np.abs(b))), 1e-300)
        parts.append("%s %.2e" % (name, float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / s))
    print("%s member %d: %s" % (what, r, "  ".join(parts)))


# ---- members against the single call ---------------------------------------------------------------------------------------------
X_CASES = [  # (N, family, ard, D, P, R)
    (1, "rbf", False, 1, 1, 2), (2, "Mat52", True, 3, 1, 5), (127, "Mat32", True, 1, 3, 5), (128, "Exponential", False, 3, 1, 2),
    (129, "Mat52", True, 17, 1, 5), (300, "rbf", True, 17, 3, 5), (300, "Mat32", False, 3, 1, 64), (300, "Exponential", True, 3, 1, 1),
    (128, "rbf", False, 17, 3, 1), (770, "Mat52", True, 3, 1, 2), (770, "Exponential", False, 17, 3, 5), (770, "rbf", True, 1, 1, 1),
    (2048, "rbf", True, 3, 1, 5), (2048, "Mat32", False, 1, 3, 2), (2048, "Mat52", False, 17, 1, 1),
]


@pytest.mark.parametrize("N,fam,ard,D,P,R", X_CASES)
def test_members_equal_the_single_call_x(h, N, fam, ard, D, P, R):
    X, Y = C.data(N, D, P, seed=N + D)
    Xw = C.kumar_members(X, R, seed=R + N)
    var, ls, noise = C.kernel_members(R, D, ard, seed=R + N + 1)
    _load(h, X, Y)
    h.set_params(KID[fam], ard, var[0], ls[0], noise[0])
    res = h.fit_grad_x_batch(Xw, var, ls, noise)
    status = res[3]
    exact = 0
    for r in range(R):
        ref = _single_x(h, fam, ard, Xw[r], Y, var[r], ls[r], noise[r])
        if ref is None:
            assert status[r] > 0 and np.all(np.isnan(res[2][r]))
            continue
        assert status[r] == 0, r
        got = _batch_x(res, r)
        _report("x-batch N=%d" % N, r, got, ref)
        assert got[0][2] == ref[0][2], (r, got[0][2], ref[0][2])       # the same rung of the jitter ladder
        assert np.all(np.isfinite(got[2]))
        assert C.close(got[0], ref[0], got[1], ref[1]), (r, got[:2], ref[:2])
        assert np.max(np.abs(got[2] - ref[2])) <= 1e-12 * np.max(np.abs(ref[2])), r
        exact += int(all(C.same_bits(a, b) for a, b in zip(got, ref)))
    if _npad(N) <= 768:
        assert exact == int(np.sum(status == 0)), (exact, R)


W_CASES = [  # (N, family, ard, D, T, R)
    (1, "rbf", False, 1, 1, 2), (2, "Mat52", True, 3, 3, 5), (127, "Mat32", True, 1, 8, 5), (128, "Exponential", False, 3, 1, 2),
    (129, "Mat52", True, 17, 3, 5), (300, "rbf", True, 17, 8, 64), (300, "Mat32", False, 3, 3, 1), (300, "Exponential", True, 3, 1, 5),
    (770, "Exponential", True, 3, 3, 5), (770, "rbf", False, 1, 1, 2), (770, "Mat32", True, 17, 8, 1),
    (2048, "Mat52", True, 3, 3, 5), (2048, "Mat32", False, 17, 8, 2), (2048, "rbf", False, 1, 1, 1),
]


@pytest.mark.parametrize("N,fam,ard,D,T,R", W_CASES)
def test_members_equal_the_single_call_warp(h, N, fam, ard, D, T, R):
    X, Y = C.data(N, D, 1, seed=N + D + 7)
    psi, d = C.tanh_members(R, T, seed=R + N + T)
    var, ls, noise = C.kernel_members(R, D, ard, seed=R + N + 2)
    _load(h, X, Y)
    h.set_params(KID[fam], ard, var[0], ls[0], noise[0])
    res = h.fit_grad_warp_batch(psi, d, var, ls, noise)            # no warp on: the raw targets are the resident ones
    status = res[4]
    exact = 0
    for r in range(R):
        ref = _single_w(h, fam, ard, var[r], ls[r], noise[r], psi[r], d[r])
        if ref is None:
            assert status[r] > 0
            continue
        assert status[r] == 0, r
        got = _batch_w(res, r)
        _report("warp-batch N=%d" % N, r, got, ref)
        assert got[0][2] == ref[0][2], (r, got[0][2], ref[0][2])
        assert np.float64(got[0][3]).tobytes() == np.float64(ref[0][3]).tobytes()      # the log-Jacobian: no route in it
        assert C.close(got[0], ref[0], got[1], ref[1]), (r, got, ref)
        exact += int(all(C.same_bits(a, b) for a, b in zip(got, ref)))
    if _npad(N) <= 768:
        assert exact == int(np.sum(status == 0)), (exact, R)
    # a warp is on now (the last single call's): the batch reads the raw targets kept beside the warped ones -- the same bits
    again = h.fit_grad_warp_batch(psi, d, var, ls, noise)
    for a, b in zip(_flat_w(res), _flat_w(again)):
        assert C.same_bits(a, b)
    h.set_output_warp(None)


def _flat_w(res):
    (lml, logdet, jit), (dv, dl, dn), lj, (dpsi, dd), st = res
    return [lml, logdet, jit, dv, dl, dn, lj, dpsi, dd, st.astype(float)]


def _flat_x(res):
    (lml, logdet, jit), (dv, dl, dn), dX, st = res
    return [lml, logdet, jit, dv, dl, dn, dX, st.astype(float)]


# ---- position and company ----------------------------------------------------------------------------------------------------------
def _hard_member(X):
    """Inputs with duplicated rows and parameters that need the jitter ladder (tests/test_gpu_fit_grad_batch.py)."""
    Xd = X.copy()
    Xd[X.shape[0] // 2:] = X[:X.shape[0] - X.shape[0] // 2]
    return Xd, 1e8, 1e-12


@pytest.mark.parametrize("N,D,ard", [(129, 3, True), (770, 17, False)])
def test_a_member_is_the_same_wherever_and_with_whomever_x(h, N, D, ard):
    X, Y = C.data(N, D, 1, seed=31)
    Xw = C.kumar_members(X, 5, seed=32)
    var, ls, noise = C.kernel_members(5, D, ard, seed=33)
    _load(h, X, Y)
    h.set_params(KID["rbf"], ard, var[0], ls[0], noise[0])
    alone = h.fit_grad_x_batch(Xw[3:4], var[3:4], ls[3:4], noise[3:4])
    five = h.fit_grad_x_batch(Xw, var, ls, noise)
    assert alone[3][0] == 0 and five[3][3] == 0
    for a, b in zip(_batch_x(alone, 0), _batch_x(five, 3)):
        assert C.same_bits(a, b)
    # ... and behind a member that climbs the jitter ladder: the later rounds factor that member alone
    Xd, vbad, nbad = _hard_member(Xw[0])
    pair = h.fit_grad_x_batch(np.stack([Xd, Xw[3]]), np.r_[vbad, var[3]], np.vstack([np.full_like(ls[3], 2.0 * np.sqrt(D)), ls[3]]),
                              np.r_[nbad, noise[3]])
    print("jitter of the member ahead: %g (status %d)" % (pair[0][2][0], pair[3][0]))
    assert pair[3][0] != 0 or pair[0][2][0] > 0
    for a, b in zip(_batch_x(alone, 0), _batch_x(pair, 1)):
        assert C.same_bits(a, b)


@pytest.mark.parametrize("N,D,ard", [(129, 3, True), (770, 17, False)])
def test_a_member_is_the_same_wherever_and_with_whomever_warp(h, N, D, ard):
    X, Y = C.data(N, D, 1, seed=41)
    X[N // 2:] = X[:N - N // 2]                         # duplicated rows: a member with a huge variance and no noise needs jitter
    psi, d = C.tanh_members(5, 3, seed=42)
    var, ls, noise = C.kernel_members(5, D, ard, seed=43)
    _load(h, X, Y)
    h.set_params(KID["rbf"], ard, var[0], ls[0], noise[0])
    alone = h.fit_grad_warp_batch(psi[3:4], d[3:4], var[3:4], ls[3:4], noise[3:4])
    five = h.fit_grad_warp_batch(psi, d, var, ls, noise)
    assert alone[4][0] == 0 and five[4][3] == 0
    for a, b in zip(_batch_w(alone, 0), _batch_w(five, 3)):
        assert C.same_bits(a, b)
    pair = h.fit_grad_warp_batch(psi[[0, 3]], d[[0, 3]], np.r_[1e8, var[3]], np.vstack([np.full_like(ls[3], 2.0 * np.sqrt(D)), ls[3]]),
                                 np.r_[1e-12, noise[3]])
    print("jitter of the member ahead: %g (status %d)" % (pair[0][2][0], pair[4][0]))
    assert pair[4][0] != 0 or pair[0][2][0] > 0
    for a, b in zip(_batch_w(alone, 0), _batch_w(pair, 1)):
        assert C.same_bits(a, b)


# ---- jitter per member ---------------------------------------------------------------------------------------------------------------
def _nan_iff_failed(flat, status):
    for r in range(status.size):
        for a in flat[:-1]:
            row = np.asarray(a[r], dtype=float)
            assert np.all(np.isnan(row)) if status[r] else np.all(np.isfinite(row)), (r, status[r])


def test_jitter_per_member_x(h):
    N, D = 160, 2
    X, Y = C.data(N, D, 1, seed=51)
    Xw = C.kumar_members(X, 4, seed=52)
    Xw[1] = _hard_member(Xw[1])[0]                       # member 1 alone has duplicated inputs
    var = np.array([1.0, 1e8, 0.7, 1.3])
    ls = np.array([[0.3], [2.0], [0.4], [0.25]])
    noise = np.array([1e-2, 1e-12, 1e-3, 1e-2])
    _load(h, X, Y)
    h.set_params(KID["rbf"], False, var[0], ls[0], noise[0])
    res = h.fit_grad_x_batch(Xw, var, ls, noise)
    st, jit = res[3], res[0][2]
    print("status", st, "jitter", jit)
    assert st[0] == st[2] == st[3] == 0 and (st[1] != 0 or jit[1] > 0) and jit[0] == jit[2] == jit[3] == 0.0
    _nan_iff_failed(_flat_x(res), st)
    if st[1] == 0:
        ref = _single_x(h, "rbf", False, Xw[1], Y, var[1], ls[1], noise[1])
        got = _batch_x(res, 1)
        assert ref is not None and got[0][2] == ref[0][2] and C.close(got[0], ref[0], got[1], ref[1])
        h.set_data(X, Y)
    keep = [0, 2, 3]
    without = h.fit_grad_x_batch(Xw[keep], var[keep], ls[keep], noise[keep])
    for i, r in enumerate(keep):                         # the others: bitwise what they are without it
        for a, b in zip(_batch_x(res, r), _batch_x(without, i)):
            assert C.same_bits(a, b)
    res0 = h.fit_grad_x_batch(Xw, var, ls, noise, maxtries=0)      # no retries: exactly that member fails, alone, with a status
    assert res0[3][1] > 0 and not res0[3][keep].any()
    _nan_iff_failed(_flat_x(res0), res0[3])
    for r in keep:
        for a, b in zip(_batch_x(res0, r), _batch_x(res, r)):
            assert C.same_bits(a, b)


def test_jitter_per_member_warp(h):
    N, D = 160, 2
    X, Y = C.data(N, D, 1, seed=61)
    X[120:] = X[:40]
    psi, d = C.tanh_members(4, 3, seed=62)
    var = np.array([1.0, 1e8, 0.7, 1.3])
    ls = np.array([[0.3], [2.0], [0.4], [0.25]])
    noise = np.array([1e-2, 1e-12, 1e-3, 1e-2])
    _load(h, X, Y)
    h.set_params(KID["rbf"], False, var[0], ls[0], noise[0])
    res = h.fit_grad_warp_batch(psi, d, var, ls, noise)
    st, jit = res[4], res[0][2]
    print("status", st, "jitter", jit)
    assert st[0] == st[2] == st[3] == 0 and (st[1] != 0 or jit[1] > 0) and jit[0] == jit[2] == jit[3] == 0.0
    _nan_iff_failed(_flat_w(res), st)
    keep = [0, 2, 3]
    without = h.fit_grad_warp_batch(psi[keep], d[keep], var[keep], ls[keep], noise[keep])
    for i, r in enumerate(keep):
        for a, b in zip(_batch_w(res, r), _batch_w(without, i)):
            assert C.same_bits(a, b)
    res0 = h.fit_grad_warp_batch(psi, d, var, ls, noise, maxtries=0)
    assert res0[4][1] > 0 and not res0[4][keep].any()
    _nan_iff_failed(_flat_w(res0), res0[4])
    h.set_params(KID["rbf"], False, var[1], ls[1], noise[1])
    with pytest.raises(np.linalg.LinAlgError):
        h.fit_grad_warp(psi[1], d[1], 1, 0)
    h.set_output_warp(None)


# ---- the resident state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warp_on", [False, True], ids=["warp-off", "warp-on"])
def test_resident_state_is_untouched(h, warp_on):
    N, D = 300, 3
    X, Y = C.data(N, D, 1, seed=71)
    Xs = np.random.default_rng(72).uniform(0, 1, (50, D))
    psi0, d0 = C.tanh_members(1, 2, seed=73)
    _load(h, X, Y)
    h.set_params(KID["Mat52"], True, 1.3, np.array([0.3, 0.5, 0.7]), 1e-3)

    def single():
        if warp_on:
            fit, grads, lj, (dpsi, dd) = h.fit_grad_warp(psi0[0], d0[0], D)
            return np.r_[fit, grads[0], grads[1], grads[2], lj, dpsi.ravel(), dd]
        fit, grads, dX = h.fit_grad_x(D)
        return np.r_[fit, grads[0], grads[1], grads[2], dX.ravel()]

    def state():
        return [np.array(h.fit_state()), h.alpha(), h.targets()] + list(h.predict())

    before_call = single()
    h.set_candidates(Xs)
    before = state()
    Xw = C.kumar_members(X, 5, seed=74)
    var, ls, noise = C.kernel_members(5, D, True, seed=75)
    psi, d = C.tanh_members(5, 3, seed=76)
    for call in (lambda: h.fit_grad_x_batch(Xw, var, ls, noise), lambda: h.fit_grad_warp_batch(psi, d, var, ls, noise)):
        res = call()
        assert not res[-1].any()
        for a, b in zip(before, state()):
            assert C.same_bits(a, b)
    if warp_on:     # the warp in force and its log-Jacobian: setting the same warp again returns the same number
        assert np.float64(h.set_output_warp(psi0[0], d0[0])).tobytes() == np.float64(before_call[3 + 1 + D + 1]).tobytes()
    assert C.same_bits(single(), before_call)
    h.set_output_warp(None)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(h):
    D = 2
    X, Y = C.data(100, D, 1, seed=81)
    _load(h, X, Y)
    h.set_params(0, True, 1.0, np.array([0.3, 0.3]), 1e-2)
    ones = lambda R: (np.ones(R), np.full((R, 2), 0.3), np.full(R, 1e-2))     # noqa: E731
    Xw = lambda R: np.tile(X, (R, 1, 1))                                        # noqa: E731
    warp = lambda R, T=2: (np.ones((R, T, 3)), np.ones(R))                      # noqa: E731
    with pytest.raises(ValueError, match="64"):
        h.fit_grad_x_batch(Xw(65), *ones(65))
    with pytest.raises(ValueError, match="64"):
        h.fit_grad_warp_batch(*warp(65), *ones(65))
    for bad in (0, 9):
        with pytest.raises(ValueError, match="terms"):
            h.fit_grad_warp_batch(np.ones((2, bad, 3)), np.ones(2), *ones(2))
    v, l, n = ones(2)
    for which in range(3):                               # a non-positive parameter, in either entry
        args = [v.copy(), l.copy(), n.copy()]
        args[which].flat[-1] = 0.0
        with pytest.raises(ValueError, match="positive"):
            h.fit_grad_x_batch(Xw(2), *args)
        with pytest.raises(ValueError, match="positive"):
            h.fit_grad_warp_batch(*warp(2), *args)
    with pytest.raises(ValueError, match="warp parameters"):
        h.fit_grad_warp_batch(np.ones((2, 2, 3)), np.array([1.0, 0.0]), *ones(2))
    with pytest.raises(ValueError):                      # inputs of another shape than the resident ones
        h.fit_grad_x_batch(np.ones((2, 99, D)), *ones(2))
    # R = 0 and null pointers: through the raw library call
    lib, p = h.lib, _lib.dptr(np.zeros(2 * 100 * D))
    st = np.zeros(2, dtype=np.int32).ctypes.data_as(_lib.c_int_p)
    assert lib.gp_fit_grad_x_batch(h.h, 0, p, p, p, p, 5, p, p, p, p, p, p, p, st) == _lib.GP_ERR_ARG
    assert lib.gp_fit_grad_warp_batch(h.h, 0, 1, p, p, p, p, p, 5, p, p, p, p, p, p, p, p, p, st) == _lib.GP_ERR_ARG
    assert lib.gp_fit_grad_x_batch(h.h, 1, None, p, p, p, 5, p, p, p, p, p, p, p, st) == _lib.GP_ERR_ARG
    assert b"null" in lib.gp_last_error()
    assert lib.gp_fit_grad_x_batch(h.h, 1, p, p, p, p, 5, p, p, p, p, p, p, None, st) == _lib.GP_ERR_ARG
    assert lib.gp_fit_grad_warp_batch(h.h, 1, 1, None, p, p, p, p, 5, p, p, p, p, p, p, p, p, p, st) == _lib.GP_ERR_ARG
    assert lib.gp_fit_grad_warp_batch(h.h, 1, 1, p, p, p, p, p, 5, p, p, p, p, p, p, p, p, p, None) == _lib.GP_ERR_ARG
    assert b"null" in lib.gp_last_error()
    # the Gower option on: no input gradients (as gp_lml_grad_x)
    h.set_gower(np.array([0, 1]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match="Gower"):
        h.fit_grad_x_batch(Xw(2), *ones(2))
    h.set_gower()
    # two outputs: no output warp
    h.set_data(X, np.c_[Y, Y])
    h.set_params(0, True, 1.0, np.array([0.3, 0.3]), 1e-2)
    with pytest.raises(ValueError, match="P = 1"):
        h.fit_grad_warp_batch(*warp(2), *ones(2))
    # N = 2049 pads beyond the cap
    X, Y = C.data(2049, D, 1, seed=82)
    h.set_data(X, Y)
    h.set_params(0, True, 1.0, np.array([0.3, 0.3]), 1e-2)
    with pytest.raises(ValueError, match="2048"):
        h.fit_grad_x_batch(np.tile(X, (2, 1, 1)), *ones(2))
    with pytest.raises(ValueError, match="2048"):
        h.fit_grad_warp_batch(*warp(2), *ones(2))


# ---- one oracle case per entry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,ard", [("Mat52", True), ("Exponential", False)])
def test_x_members_against_the_oracle(h, fam, ard):
    N, D, R = 200, 3, 3
    X, Y = C.data(N, D, 1, seed=91)
    Xw = C.kumar_members(X, R, seed=92)
    var, ls, noise = C.kernel_members(R, D, ard, seed=93)
    noise = np.maximum(noise, 1e-2)
    _load(h, X, Y)
    h.set_params(KID[fam], ard, var[0], ls[0], noise[0])
    (lml, _, _), (dv, dl, dn), dX, st = h.fit_grad_x_batch(Xw, var, ls, noise)
    assert not st.any()
    for r in range(R):
        lml0, (dv0, dl0, dn0), dX0 = C.oracle_x(fam, ard, Xw[r], Y, var[r], ls[r], noise[r])
        print("member %d: lml %.12f oracle %.12f" % (r, lml[r], lml0))
        assert abs(lml[r] - lml0) <= 1e-8 * abs(lml0)
        scale = max(abs(dv0), float(np.max(np.abs(dl0))), 1.0)
        C.err("  hyper-gradients", np.r_[dv[r], dl[r]], np.r_[dv0, dl0], 1e-6, scale)
        C.err("  dnoise", [dn[r]], [dn0], 1e-6, max(abs(dn0), 1.0))
        C.err("  dL_dX", dX[r], dX0, 1e-6)
    # the collapsing member (the last): its coincident rows carry no 0 / 0
    assert np.array_equal(Xw[R - 1][0], Xw[R - 1][1]) and np.all(np.isfinite(dX[R - 1][:2]))


@pytest.mark.parametrize("fam,ard", [("Mat32", True), ("rbf", False)])
def test_warp_members_against_the_oracle(h, fam, ard):
    N, D, R, T = 200, 3, 3, 3
    X, Y = C.data(N, D, 1, seed=95)
    psi, d = C.tanh_members(R, T, seed=96)
    var, ls, noise = C.kernel_members(R, D, ard, seed=97)
    noise = np.maximum(noise, 1e-2)
    _load(h, X, Y)
    h.set_params(KID[fam], ard, var[0], ls[0], noise[0])
    (lml, _, _), (dv, dl, dn), lj, (dpsi, dd), st = h.fit_grad_warp_batch(psi, d, var, ls, noise)
    assert not st.any()
    for r in range(R):
        ll0, natural = C.oracle_warp(fam, ard, X, Y, var[r], ls[r], noise[r], psi[r], d[r])
        print("member %d: LML + log-Jacobian %.12f  oracle %.12f" % (r, lml[r] + lj[r], ll0))
        assert abs(lml[r] + lj[r] - ll0) <= 1e-8 * abs(ll0)
        got = np.r_[dv[r], dl[r], dn[r], dpsi[r][:, 0], dpsi[r][:, 1], dpsi[r][:, 2], dd[r]]
        C.err("  natural gradient", got, natural, 1e-6)
        nk = 2 + ls.shape[1]
        C.err("  its warp entries alone", got[nk:], natural[nk:], 1e-6)


# ---- the models ------------------------------------------------------------------------------------------------------------------------
class _Counting(object):
    NAMES = ("fit_grad_x", "fit_grad_warp", "fit_grad_x_batch", "fit_grad_warp_batch")

    def __init__(self, h):
        self.h, self.calls = h, {n: 0 for n in self.NAMES}

    def __getattr__(self, name):
        attr = getattr(self.h, name)
        if name not in self.NAMES:
            return attr

        def counted(*a, **k):
            self.calls[name] += 1
            return attr(*a, **k)
        return counted


def _compare_runs(rs, rp):
    """``_compare_runs`` of tests/test_gpu_fit_grad_batch.py: every run within 1e-8 relative, the same winner."""
    assert len(rs) == len(rp)
    for (fs, _), (fp, _) in zip(rs, rp):
        print("run: serial %.12f  lockstep %.12f" % (fs, fp))
        assert abs(fs - fp) <= 1e-8 * abs(fs), (fs, fp)
    assert int(np.argmin([f for f, _ in rs])) == int(np.argmin([f for f, _ in rp]))


def _model_data(N=200, D=3, seed=12):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.exp(np.sin(4 * X ** 2).sum(1, keepdims=True) / np.sqrt(D)) + 0.05 * rng.standard_normal((N, 1))
    return X, Y


def _input_warped(X, Y):
    D = X.shape[1]
    m = gpo.models.InputWarpedGP(X, Y, kernel=gpo.kern.Matern52(D, variance=1.0, ARD=True), Xmin=[0.0] * D, Xmax=[1.0] * D)
    m.Gaussian_noise.variance.set(1e-2)
    m.Gaussian_noise.constrain_bounded(1e-9, 1e6, warning=False)
    return m


def _warped(X, Y, warping_function=None):
    m = gpo.models.WarpedGP(X, Y, kernel=gpo.kern.Matern32(X.shape[1], variance=1.0, ARD=True), warping_terms=2,
                            warping_function=warping_function)
    m.Gaussian_noise.variance.set(1e-2)
    m.Gaussian_noise.constrain_positive(warning=False)
    return m


MODELS = {"input_warped": (_input_warped, "fit_grad_x"), "warped": (_warped, "fit_grad_warp")}


@pytest.mark.parametrize("which", ["input_warped", "warped"])
def test_model_parallel_restarts_against_serial(which):
    make, single = MODELS[which]
    X, Y = _model_data()
    ms, mp = make(X, Y), make(X, Y)
    try:
        np.random.seed(77)
        rs = ms.optimize_restarts(5, verbose=False, max_iters=200)
        np.random.seed(77)
        mp._h = _Counting(mp._h)
        rp = mp.optimize_restarts(5, verbose=False, max_iters=200, parallel=True)
        _compare_runs(rs, rp)
        print("calls", mp._h.calls)
        assert mp._h.calls[single] == 0 and mp._h.calls[single + "_batch"] >= 1
        assert abs(ms.log_likelihood() - mp.log_likelihood()) <= 1e-8 * abs(ms.log_likelihood())
    finally:
        ms.close()
        mp.close()


@pytest.mark.parametrize("which", ["input_warped", "warped"])
def test_bo_model_parallel_restarts_against_serial(which):
    X, Y = _model_data(seed=13)
    space = gpo.Design_space([{'name': 'x%d' % i, 'type': 'continuous', 'domain': (0.0, 1.0)} for i in range(X.shape[1])])
    single = MODELS[which][1]
    out = []
    for flag in (False, True):
        if which == "input_warped":
            gm = gpo.models.InputWarpedGPModel(space, optimize_restarts=5, max_iters=200, verbose=False, ARD=True,
                                               parallel_restarts=flag)
        else:
            gm = gpo.models.WarpedGPModel(optimize_restarts=5, max_iters=200, warping_terms=2, verbose=False, parallel_restarts=flag)
        gm._create_model(X, Y)
        try:
            gm.model._h = _Counting(gm.model._h)
            np.random.seed(78)
            runs = []
            orig = gm.model.optimize_restarts
            gm.model.optimize_restarts = lambda *a, **k: runs.extend(orig(*a, **k)) or runs
            if which == "warped" and not flag:     # (the serial WarpedGPModel makes one ``optimize``: the restarts it is held against)
                gm.model.optimize_restarts(num_restarts=5, verbose=False, optimizer=gm.optimizer, max_iters=gm.max_iters)
            else:
                gm.updateModel(X, Y, None, None)
            out.append((runs, gm.model.log_likelihood()))
            print("parallel_restarts=%s calls %s" % (flag, gm.model._h.calls))
            if flag:
                assert gm.model._h.calls[single] == 0 and gm.model._h.calls[single + "_batch"] >= 1
            else:
                assert gm.model._h.calls[single] >= 1 and gm.model._h.calls[single + "_batch"] == 0
        finally:
            gm.model.close()
    _compare_runs(out[0][0], out[1][0])
    assert abs(out[0][1] - out[1][1]) <= 1e-8 * abs(out[0][1])


@pytest.mark.parametrize("which", ["input_warped", "warped"])
def test_parallel_restarts_above_the_limit_take_the_serial_route(which):
    make, single = MODELS[which]
    X, Y = _model_data(N=3000, D=2, seed=4)
    m = make(X, Y)
    try:
        m._h = _Counting(m._h)
        np.random.seed(0)
        runs = m.optimize_restarts(2, verbose=False, max_iters=3, parallel=True)
        assert len(runs) == 2 and m._h.calls[single + "_batch"] == 0 and m._h.calls[single] >= 1
    finally:
        m.close()


def test_identity_warp_takes_the_serial_route():
    X, Y = _model_data(N=60, D=2, seed=5)
    m = _warped(X, Y, warping_function=IdentityFunction())
    try:
        m._h = _Counting(m._h)
        np.random.seed(0)
        runs = m.optimize_restarts(2, verbose=False, max_iters=5, parallel=True)
        assert len(runs) == 2 and m._h.calls["fit_grad_warp_batch"] == 0 and m._h.calls["fit_grad_x_batch"] == 0
    finally:
        m.close()
