"""GPU: multi-output fits at the limits of P and D (the case table tests/_output_limits.py) against the float64 oracle, which
tests/test_output_limits_host.py holds to a long-double truth at a tenth of the bar used here.

Everything indexed by the output p is held per output column, relative to that column's own largest reference magnitude
(OL.col_err): the columns differ in scale by up to 64 and no two are alike, so a swapped or mis-strided output index cannot pass.

The bar is the project's parity bar: LML 1e-8 relative (log det 1e-10, as tests/test_gpu_family_shapes.py),
alpha, means, variances and the full covariance 1e-6, gradients 1e-6 of their scale (kernel entries against max(|dvariance|,
max |dlengthscale|, 1), the noise entry against max(|dnoise|, 1), as tests/test_gpu_parity.py scales them).

The refusal cases -- shapes whose fused gradient pass needs more LDS than a workgroup has (csrc/grad.hip, lml_grad_lds_bytes) --
call the gradient entries only after gp_lml_grad_lds has said that the library makes that comparison and what it comes to: no
test here issues an oversized launch.

Every figure is printed before it is asserted ("output_limits: case quantity error"; tools/output_limits_table.py turns a log of
them into profiles/output_limits.txt).
"""
import contextlib
import functools
import re

import numpy as np
import pytest

from gaussian_process_optimization_amd import _lib

import _output_limits as OL
import _sparse_ref as SR

pytestmark = pytest.mark.gpu

TOL, TOL_LML, TOL_LOGDET = 1e-6, 1e-8, 1e-10
DEFAULTS = {"emulate_fp64": 0, "lookahead": 1, "lookahead_min_tiles": 40, "panel_tiles": 6, "own_keep_per_row": 36,
            "own_keep_base": 200, "pipe_stages": 0, "pipe_start_pct": -1}
LDS_MESSAGE = re.compile(r"D = (\d+), P = (\d+), Gower (on|off) need (\d+) bytes of LDS per workgroup in the gradient pass, "
                         r"the device has (\d+)")


def _params(pairs):
    return [pytest.param(f, c, id="%s-%s" % (f, c)) for f, c in pairs]


def _hold(case, what, err, tol):
    err = float(err)
    print("output_limits: %-20s %-22s %.3e  tol %.0e" % (case, what, err, tol))
    assert np.isfinite(err) and err <= tol, (case, what, err, tol)


def _rel(got, ref, scale=None):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    s = float(np.max(np.abs(ref))) if scale is None else float(scale)
    return float(np.max(np.abs(got - ref))) / s


def _hold_grads(case, what, got, ref):
    (dv, dl, dn), (dv0, dl0, dn0) = got, ref
    scale = max(abs(float(dv0)), float(np.max(np.abs(dl0))), 1.0)
    _hold(case, what + " dvariance", abs(dv - dv0) / scale, TOL)
    _hold(case, what + " dlengthscale", _rel(dl, dl0, scale), TOL)
    _hold(case, what + " dnoise", abs(dn - dn0) / max(abs(float(dn0)), 1.0), TOL)


def _bits(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _ref(fam, cid):
    """The oracle's numbers of one case, computed once and shared (read-only) by every test that needs them."""
    c = OL.CASES[cid]
    X, Y, Xs, ls = OL.problem(cid)
    gp = OL.oracle(fam, cid)
    p = gp.posterior
    assert p["jitter"] == 0.0
    r = _Namespace(lml=p["lml"], logdet=p["logdet"], alpha=p["alpha"])
    r.mu, r.var = gp.predict(Xs)
    _, r.var0 = gp.predict_noiseless(Xs)
    _, r.cov = gp.predict(Xs, full_cov=True)
    r.dmdx, r.dvdx = gp.predictive_gradients(Xs[:OL.M_GRAD])
    if c.grad == "yes":
        r.grads = gp.gradients()
    for v in vars(r).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


class _Namespace(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


@contextlib.contextmanager
def route(h, opts):
    try:
        for k, v in opts.items():
            h.set_option(k, v)
        yield h
    finally:
        for k in opts:
            h.set_option(k, DEFAULTS[k])


@pytest.fixture(scope="module")
def h():
    hd = _lib.Handle(0)
    hd.set_option("emulate_fp64", 0)
    yield hd
    hd.close()


def _set(h, fam, cid, member=0, rows=None, scale=1.0):
    """Data, parameters and Gower setting of a case (a member of its batch; its first `rows` rows; its targets times `scale`)."""
    c = OL.CASES[cid]
    X, Y, Xs, ls = OL.problem(cid)
    var, lsm, noise = OL.members(cid)
    n = c.N if rows is None else rows
    h.set_data(X[:n], Y[:n] * scale)
    h.set_gower()
    h.set_params(OL.KERNEL_ID[fam], 1, var[member], lsm[member], noise[member])
    if c.gower:
        disc, ranges, _ = OL.gower_setup(cid)
        h.set_gower(disc, ranges)
    return c, X, Y, Xs, ls


# ---- P = 129 ---------------------------------------------------------------------------------------------------------------------
def test_p129_is_refused_and_the_previous_fit_stays(h):
    c, X, Y, Xs, ls = _set(h, "rbf", "P4")
    state = h.fit()
    h.set_candidates(Xs)
    alpha, (mu, var) = h.alpha(), h.predict(True)
    rng = np.random.default_rng(129)
    with pytest.raises(ValueError, match="P=129"):
        h.set_data(X, rng.standard_normal((c.N, OL.P_REFUSED_BY_SET_DATA)))
    assert (h.N, h.D, h.P) == (c.N, c.D, c.P)
    assert h.fit_state() == state and _bits(h.alpha(), alpha)
    mu1, var1 = h.predict(True)
    assert _bits(mu1, mu) and _bits(var1, var)
    assert h.fit() == state and _bits(h.alpha(), alpha)          # the data is still there: a new fit is the old one


# ---- the exact model: fit and prediction at every shape, the refused ones included --------------------------------------------------
@pytest.mark.parametrize("fam,cid", _params((f, c) for f, c in OL.PAIRS if c != "LA"))
def test_fit_and_prediction(h, fam, cid):
    """gp_fit scalars, alpha for all P columns, gp_predict on the tile route (M = 130) and the small-M route (M = 3), the full
    covariance, gp_predict_grad (dmdx [M, D, P], M = 5), and gp_fit_predict == gp_fit + gp_predict bit for bit on both routes.
    The shapes whose gradient pass is refused are among the cases: fit and prediction work there."""
    c, X, Y, Xs, ls = _set(h, fam, cid)
    r = _ref(fam, cid)
    case = "%s-%s" % (fam, cid)
    lml, logdet, jit = h.fit()
    assert jit == 0.0
    _hold(case, "lml", abs(lml - r.lml) / abs(r.lml), TOL_LML)
    _hold(case, "logdet", abs(logdet - r.logdet) / abs(r.logdet), TOL_LOGDET)
    alpha = h.alpha()
    assert alpha.shape == (c.N, c.P)
    _hold(case, "alpha", OL.col_err(alpha, r.alpha), TOL)
    for name, m in (("tile", OL.M_TILE), ("small", OL.M_SMALL)):
        h.set_candidates(Xs[:m])
        mu, var = h.predict(True)
        assert mu.shape == (m, c.P) and var.shape == (m, 1)
        _hold(case, "mean " + name, OL.col_err(mu, r.mu[:m]), TOL)
        _hold(case, "var " + name, np.max(np.abs(var / r.var[:m] - 1.0)), TOL)
        mu0, var0 = h.predict(False)
        _hold(case, "mean0 " + name, OL.col_err(mu0, r.mu[:m]), TOL)
        _hold(case, "var0 " + name, _rel(var0, r.var0[:m], OL.variance_of(cid)), TOL)
        (lml1, logdet1, jit1), mu1, var1 = h.fit_predict(True)
        assert (lml1, logdet1, jit1) == (lml, logdet, jit) and _bits(mu1, mu) and _bits(var1, var), name
    h.set_candidates(Xs)
    mu2, cov = h.predict_full_cov(True)
    _hold(case, "full_cov mean", OL.col_err(mu2, r.mu), TOL)
    _hold(case, "full_cov", _rel(cov, r.cov), TOL)
    h.set_candidates(Xs[:OL.M_GRAD])
    dm, dv = h.predict_grad()
    assert dm.shape == (OL.M_GRAD, c.D, c.P)
    _hold(case, "dmdx", OL.col_err(dm, r.dmdx), TOL)
    _hold(case, "dvdx", _rel(dv, r.dvdx), TOL)
    _hold(case, "dmdx alone", OL.col_err(h.predict_grad(mean_only=True), r.dmdx), TOL)


# ---- the look-ahead scheduler with a full RHS tile -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2])
def test_lookahead_with_a_full_rhs_tile_is_bitwise_single_stream(h, W):
    """N = 300 (three tiles), P = 128: with lookahead_min_tiles = 0 the look-ahead factorisation carries the full RHS tile row
    through its chain and bulk streams.  gp_fit and gp_fit_predict reproduce the single-stream route (lookahead = 0) of the same
    panel width bit for bit, as tests/test_gpu_jitter_routes.py holds the jittered fits; the single-stream result is held to the
    oracle."""
    c, X, Y, Xs, ls = _set(h, "rbf", "LA")
    r = _ref("rbf", "LA")
    case = "rbf-LA-W%d" % W
    h.set_candidates(Xs)
    with route(h, {"lookahead": 0, "panel_tiles": W}):
        s0 = h.fit()
        a0, (m0, v0) = h.alpha(), h.predict(True)
        f0 = h.fit_predict(True)
    _hold(case, "lml", abs(s0[0] - r.lml) / abs(r.lml), TOL_LML)
    _hold(case, "alpha", OL.col_err(a0, r.alpha), TOL)
    _hold(case, "mean tile", OL.col_err(m0, r.mu), TOL)
    _hold(case, "var tile", np.max(np.abs(v0 / r.var - 1.0)), TOL)
    assert f0[0] == s0 and _bits(f0[1], m0) and _bits(f0[2], v0)
    owned = {"plain": {"own_keep_per_row": 0}, "owned": {"own_keep_per_row": 1, "own_keep_base": 0}}
    pipe = {"auto": {"pipe_stages": 0, "pipe_start_pct": -1}, "all": {"pipe_stages": 1 << 20, "pipe_start_pct": 0}}
    for o, p in (("plain", "auto"), ("owned", "all")):
        with route(h, dict(owned[o], lookahead=1, lookahead_min_tiles=0, panel_tiles=W, **pipe[p])):
            s1 = h.fit()
            a1, (m1, v1) = h.alpha(), h.predict(True)
            f1 = h.fit_predict(True)
        print("la-%s-%s-W%d: lml %.3e alpha %.3e mean %.3e var %.3e" % (o, p, W, abs(s1[0] - s0[0]), np.max(np.abs(a1 - a0)),
                                                                     np.max(np.abs(m1 - m0)), np.max(np.abs(v1 - v0))))
        assert s1 == s0 and _bits(a1, a0) and _bits(m1, m0) and _bits(v1, v0), (o, p, W)
        assert f1[0] == s0 and _bits(f1[1], m0) and _bits(f1[2], v0), (o, p, W)


# ---- gp_append at P = 16 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["rbf", "Mat32"])
def test_append_three_rows_at_p16(fam):
    """The first 127 rows of case P16 fitted, its last three appended (the border crosses the tile edge at 128): everything the
    handle serves afterwards against the oracle's fit of all 130 rows."""
    hd = _lib.Handle(0)
    try:
        hd.set_option("emulate_fp64", 0)
        c, X, Y, Xs, ls = _set(hd, fam, "P16", rows=OL.N - OL.APPEND_K)
        r = _ref(fam, "P16")
        case = "%s-P16-append" % fam
        hd.fit()
        lml, logdet = hd.append(X[OL.N - OL.APPEND_K:], Y)
        _hold(case, "lml", abs(lml - r.lml) / abs(r.lml), TOL_LML)
        _hold(case, "logdet", abs(logdet - r.logdet) / abs(r.logdet), TOL_LOGDET)
        _hold(case, "alpha", OL.col_err(hd.alpha(), r.alpha), TOL)
        for name, m in (("tile", OL.M_TILE), ("small", OL.M_SMALL)):
            hd.set_candidates(Xs[:m])
            mu, var = hd.predict(True)
            _hold(case, "mean " + name, OL.col_err(mu, r.mu[:m]), TOL)
            _hold(case, "var " + name, np.max(np.abs(var / r.var[:m] - 1.0)), TOL)
        _hold_grads(case, "lml_grad", hd.lml_grad(ls.size), r.grads)
    finally:
        hd.close()


# ---- emulate_fp64 = 1 at P = 16 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,scale", OL.EMULATED, ids=["P16", "P16-x1000"])
def test_emulated_fp64_at_p16(cid, scale):
    """The bulk contractions on the int8 matrix cores, on a handle of its own: the targets as they are, and times 1e3 (the
    fixed-point range of the residue form depends on the operands' size).  Whether the call stays in residue form or repeats in
    fp64, it meets the bar."""
    hd = _lib.Handle(0)
    try:
        hd.set_option("emulate_fp64", 1)
        c, X, Y, Xs, ls = _set(hd, "rbf", cid, scale=scale)
        gp = OL.oracle("rbf", cid, 0, scale)
        p = gp.posterior
        case = "rbf-%s-emu-x%g" % (cid, scale)
        lml, logdet, jit = hd.fit()
        assert jit == 0.0 and p["jitter"] == 0.0
        _hold(case, "lml", abs(lml - p["lml"]) / abs(p["lml"]), TOL_LML)
        _hold(case, "logdet", abs(logdet - p["logdet"]) / abs(p["logdet"]), TOL_LOGDET)
        _hold(case, "alpha", OL.col_err(hd.alpha(), p["alpha"]), TOL)
        mu_ref, var_ref = gp.predict(Xs)
        for name, m in (("tile", OL.M_TILE), ("small", OL.M_SMALL)):
            hd.set_candidates(Xs[:m])
            mu, var = hd.predict(True)
            _hold(case, "mean " + name, OL.col_err(mu, mu_ref[:m]), TOL)
            _hold(case, "var " + name, np.max(np.abs(var / var_ref[:m] - 1.0)), TOL)
        hd.set_candidates(Xs)
        _, cov = hd.predict_full_cov(True)
        _hold(case, "full_cov", _rel(cov, gp.predict(Xs, full_cov=True)[1]), TOL)
        _hold_grads(case, "lml_grad", hd.lml_grad(ls.size), gp.gradients())
        (l2, d2, j2), g2 = hd.fit_grad(ls.size)
        _hold(case, "fit_grad lml", abs(l2 - p["lml"]) / abs(p["lml"]), TOL_LML)
        _hold_grads(case, "fit_grad", g2, gp.gradients())
    finally:
        hd.close()


# ---- gradients -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,cid", _params((f, c) for f, c in OL.PAIRS if OL.CASES[c].grad == "yes"))
def test_gradients(h, fam, cid):
    """gp_lml_grad, gp_fit_grad (== gp_fit + gp_lml_grad bit for bit) and gp_fit_grad_batch (three members) at P = 16 and P = 4
    with D = 3 and at every boundary shape that fits -- D + P = 79, and 2 D + P = 79 for the Gower model, whose oracle is the one
    tests/test_gpu_gower.py uses for gp_lml_grad (the fork's update_gradients_full, O.make_kernel(..., Gower=True))."""
    c, X, Y, Xs, ls = _set(h, fam, cid)
    r = _ref(fam, cid)
    case = "%s-%s" % (fam, cid)
    need, avail = h.lml_grad_lds()
    assert need == OL.lds_lml_grad(c.D, c.gower, c.P) and need <= avail
    state = h.fit()
    g = h.lml_grad(ls.size)
    _hold_grads(case, "lml_grad", g, r.grads)
    state2, g2 = h.fit_grad(ls.size)
    assert state2 == state and g2[0] == g[0] and _bits(g2[1], g[1]) and g2[2] == g[2]
    var, lsm, noise = OL.members(cid)
    (lml, logdet, jit), (dv, dl, dn), status = h.fit_grad_batch(var, lsm, noise)
    assert status.shape == (3,) and not status.any()
    for m in range(3):
        gp = OL.oracle(fam, cid, m)
        assert gp.posterior["jitter"] == 0.0 and jit[m] == 0.0
        _hold(case, "batch %d lml" % m, abs(lml[m] - gp.posterior["lml"]) / abs(gp.posterior["lml"]), TOL_LML)
        _hold_grads(case, "batch %d" % m, (dv[m], dl[m], dn[m]), gp.gradients())
    assert h.fit_state() == state                                # the batch leaves the resident fit alone


def _dl_dx_ref(fam, cid):
    """The recipe of tests/test_gpu_lml_grad_x.py::_ref on this table's data: the direct-distance kernel's gradients_X(dL_dK, X)
    with X2 = None on the oracle's dL_dK."""
    gp = OL.oracle(fam, cid)
    return np.asarray(gp.kern.gradients_X(gp.posterior["dL_dK"], gp.X), dtype=float)


@pytest.mark.parametrize("fam", OL.CASES["D64P16"].fams)
def test_lml_grad_x_at_d64_p16(h, fam):
    """gp_lml_grad_x at (64, 16) asks for exactly the 163840 bytes a workgroup has and does not reach launch_lml_grad: it works
    where gp_lml_grad is refused.  1e-6 of the largest reference entry, as tests/test_gpu_lml_grad_x.py."""
    c, X, Y, Xs, ls = _set(h, fam, "D64P16")
    assert OL.lds_gradx(c.D, c.P) == OL.LDS_GFX950
    h.fit()
    _hold("%s-D64P16" % fam, "dL_dX", _rel(h.lml_grad_x(), _dl_dx_ref(fam, "D64P16")), TOL)


def _gradient_entries(h, c, X, ls, cid):
    """(name, call) of every entry that reaches launch_lml_grad for this shape."""
    var, lsm, noise = OL.members(cid)
    out = [("gp_lml_grad", lambda: h.lml_grad(ls.size)), ("gp_fit_grad", lambda: h.fit_grad(ls.size)),
           ("gp_fit_grad_batch", lambda: h.fit_grad_batch(var, lsm, noise))]
    if not c.gower:
        out += [("gp_fit_grad_x", lambda: h.fit_grad_x(ls.size)),
                ("gp_fit_grad_x_batch", lambda: h.fit_grad_x_batch(np.stack([X, X * 0.9, X * 1.1]), var, lsm, noise))]
    if c.P == 1:
        psi = np.array([[0.7, 0.5, 0.1]])
        out += [("gp_fit_grad_warp", lambda: h.fit_grad_warp(psi, 1.0, ls.size)),
                ("gp_fit_grad_warp_batch", lambda: h.fit_grad_warp_batch(np.stack([psi] * 3), np.ones(3), var, lsm, noise))]
    return out


def test_p17_is_refused_by_every_gradient_entry(h):
    c, X, Y, Xs, ls = _set(h, "rbf", "P17")
    state = h.fit()
    h.set_candidates(Xs)
    alpha, (mu, var) = h.alpha(), h.predict(True)
    entries = _gradient_entries(h, c, X, ls, "P17") + [("gp_lml_grad_x", h.lml_grad_x)]
    assert len(entries) == 6
    for name, call in entries:
        with pytest.raises(ValueError, match="P <= 16"):
            call()
        mu1, var1 = h.predict(True)
        assert h.fit_state() == state and _bits(h.alpha(), alpha) and _bits(mu1, mu) and _bits(var1, var), name


@pytest.mark.parametrize("fam,cid", _params((f, c) for f, c in OL.PAIRS if c in OL.BOUNDARY_REFUSED))
def test_refused_shapes(h, fam, cid):
    """Every entry that reaches launch_lml_grad returns GP_ERR_ARG (ValueError) up front, with D, P, the Gower setting, the bytes
    needed and the bytes there are in the message; gp_fit_grad and the others leave the prior fit intact -- the fit's scalars, alpha,
    the resident candidates' posterior (bit for bit) and, for the warp entries, the targets.  That gp_fit and gp_predict work at
    these shapes is test_fit_and_prediction's business."""
    c, X, Y, Xs, ls = _set(h, fam, cid)
    need, avail = h.lml_grad_lds()                               # the library makes the comparison, and it says "refused"
    assert need == OL.lds_lml_grad(c.D, c.gower, c.P) and avail == OL.LDS_GFX950 and need > avail
    state = h.fit()
    h.set_candidates(Xs)
    alpha, (mu, var) = h.alpha(), h.predict(True)
    entries = _gradient_entries(h, c, X, ls, cid)
    assert len(entries) == (5 if not c.gower else 3) + (2 if c.P == 1 else 0)
    for name, call in entries:
        with pytest.raises(ValueError) as e:
            call()
        m = LDS_MESSAGE.search(str(e.value))
        print("%s: %s" % (name, e.value))
        assert m, (name, str(e.value))
        assert (int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(4)), int(m.group(5))) == \
            (c.D, c.P, "on" if c.gower else "off", need, avail), name
        assert name in str(e.value)
        mu1, var1 = h.predict(True)
        assert h.fit_state() == state and _bits(h.alpha(), alpha) and _bits(mu1, mu) and _bits(var1, var), name
        assert _bits(h.targets(), Y), name
    assert h.fit() == state and _bits(h.alpha(), alpha)          # and a new fit at this shape is the old one


# ---- the sparse model --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sparse_ref(fam, cid):
    c = OL.SPARSE_CASES[cid]
    X, Y, Z, Xs, ls = OL.sparse_problem(cid)
    fit = SR.inference(fam, X, Z, Y, OL.VAR, ls, True, OL.SPARSE_NOISE, SR.F64, grads=c.grad)
    assert fit["jitter_kmm"] == 0.0 and fit["jitter_b"] == 0.0
    pred = SR.predict(fit, Z, Xs, OL.SPARSE_NOISE, True, SR.F64, grads=True)
    return fit, pred


@pytest.mark.parametrize("fam,cid", _params(OL.SPARSE_PAIRS))
def test_sparse_model(h, fam, cid):
    """Mz = 130 over N = 300 against tests/_sparse_ref.py in float64: P = 16 with the gradient (every cm[] register of
    sparse_grad_tile_kernel in use), P = 17 and P = 128 without it (refused: P <= 16), fit and prediction at all three."""
    c = OL.SPARSE_CASES[cid]
    X, Y, Z, Xs, ls = OL.sparse_problem(cid)
    fit, (mu0, var0, dm0, dv0) = _sparse_ref(fam, cid)
    case = "%s-%s" % (fam, cid)
    h.set_data(X, Y)
    h.set_gower()
    h.set_params(OL.KERNEL_ID[fam], 1, OL.VAR, ls, OL.SPARSE_NOISE)
    h.sparse_set_inducing(Z)
    lml, jk, jb = h.sparse_fit()
    assert jk == 0.0 and jb == 0.0
    _hold(case, "lml", abs(lml - fit["lml"]) / abs(fit["lml"]), TOL_LML)
    wv, wi = h.sparse_posterior()
    assert wv.shape == (c.Mz, c.P)
    _hold(case, "woodbury_vector", OL.col_err(wv, fit["woodbury_vector"]), TOL)
    _hold(case, "woodbury_inv", _rel(wi, fit["woodbury_inv"]), TOL)
    mu, var, dm, dv = h.sparse_predict(Xs, include_noise=True, grad=True)
    assert mu.shape == (OL.M_TILE, c.P) and dm.shape == (OL.M_TILE, c.D, c.P)
    _hold(case, "mean", OL.col_err(mu, mu0), TOL)
    _hold(case, "var", np.max(np.abs(var[:, 0] / var0 - 1.0)), TOL)
    _hold(case, "dmdx", OL.col_err(dm, dm0), TOL)
    _hold(case, "dvdx", _rel(dv, dv0), TOL)
    if c.grad:
        assert OL.lds_sparse_grad(c.D, c.P) <= OL.LDS_GFX950
        lml2, (dvar, dl, dn, dZ) = h.sparse_fit_grad(ls.size)
        assert lml2 == lml
        _hold_grads(case, "fit_grad", (dvar, dl, dn), (float(fit["dvariance"]), fit["dlengthscale"], float(fit["dnoise"])))
        _hold(case, "dZ", _rel(dZ, fit["dZ"]), TOL)
    else:
        with pytest.raises(ValueError, match="P <= 16"):
            h.sparse_fit_grad(ls.size)
        mu1, var1 = h.sparse_predict(Xs, include_noise=True)
        assert _bits(mu1, mu) and _bits(var1, var)               # the refusal left the sparse fit as it was
