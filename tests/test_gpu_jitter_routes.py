"""GPU: fits that NEED the jitter ladder (fit_impl / ladder_step, csrc/api_factor.hip), and fits the ladder cannot save, on every
factorisation route and through gp_fit, gp_fit_predict and gp_fit_grad.  The inputs are those of tests/_jitter_cases.py: the
failing pivot b and the rung are known in advance, and tests/test_jitter_cases_host.py shows that no attempt's outcome is near
rounding and that the float64 oracle is good to a tenth of the bounds used here.

A  the single-stream route against the oracle, every row and delta of the table, at the project's bounds
   (tests/test_gpu_parity.py, tests/test_gpu_random_shapes.py): jitter 1e-12 relative; lml and log det 1e-8 max(1, |ref|); alpha,
   means, variances, the full covariance of a 128-row slice, Ky^-1, gradients, fmin (both routes), EI values 1e-6; the EI
   gradient of the rows call 1e-5.  The measured maxima are printed ("jitter_routes: ..."; kept in profiles/jitter_routes.txt).
B  every fp64 route gives BITWISE the single-stream result at the same panel width under jitter; inner_tiles = 2 and the
   emulated route are held to the oracle instead.
C  with fewer attempts than needed every entry point on every route returns b + 1, LAPACK's info; with exactly as many it
   succeeds; delta = 0.5 stays positive after five attempts; noise -2 is GP_ERR_NOT_PD_DIAG.
D  after an exhausted ladder the context refuses what needs a fit, keeps its candidates, and the next well-conditioned fit is
   bitwise that of a fresh context; the same after a jittered success.
E  gp_append on a jittered fit against the oracle's refit of the grown data, and a finite border that is not positive definite.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import _jitter_cases as J
from gaussian_process_optimization_amd import _lib
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

DEFAULTS = {"emulate_fp64": 0, "lookahead": 1, "lookahead_min_tiles": 40, "panel_tiles": 6, "own_keep_per_row": 36,
            "own_keep_base": 200, "pipe_stages": 0, "pipe_start_pct": -1, "pipe_stages_grad": 0, "pipe_start_pct_grad": 40,
            "inner_tiles": 1, "fmin_direct": 0}
OWNED = {"plain": {"own_keep_per_row": 0}, "owned": {"own_keep_per_row": 1, "own_keep_base": 0}}
PIPE = {"auto": {"pipe_stages": 0, "pipe_start_pct": -1, "pipe_stages_grad": 0, "pipe_start_pct_grad": 40},
        "all": {"pipe_stages": 1 << 20, "pipe_start_pct": 0, "pipe_stages_grad": 1 << 20, "pipe_start_pct_grad": 0}}


def single(W):
    return {"lookahead": 0, "panel_tiles": W}


def lookahead(owned, pipe, W):
    return dict(OWNED[owned], lookahead=1, lookahead_min_tiles=0, panel_tiles=W, **PIPE[pipe])


# the fp64 look-ahead routes: (panel width, options); each must reproduce single(W) bit for bit
LA = {"la-%s-%s-W%d" % (o, p, W): (W, lookahead(o, p, W)) for o in sorted(OWNED) for p in sorted(PIPE) for W in (1, 3)}
# other arithmetic: held to the oracle.  Two tile columns per step: tile 1 (b = 133) is the second tile of potrf_pair_kernel,
# tile 2 (b = 261) the first of the next pair at panel widths 2 and 4.  Emulated: panel edges on 256-column blocks.
HELD = {"inner2-single-W2": dict(single(2), inner_tiles=2),
        "inner2-la-W4": dict(lookahead("owned", "all", 4), inner_tiles=2),
        "emulated-W2": dict(emulate_fp64=1, lookahead=1, panel_tiles=2)}
ROUTES = dict({"single-W1": single(1), "single-W3": single(3)}, **{k: v[1] for k, v in LA.items()}, **HELD)
ENTRIES = ("fit", "fit_predict", "fit_grad")
FULL_DELTAS_ROUTE = "la-owned-all-W3"      # the look-ahead configuration that also runs delta = 3e-6 and 3e-4


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1.0, np.max(np.abs(b))))


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
    hh = _lib.Handle(0)
    try:
        yield hh
    finally:
        for k, v in DEFAULTS.items():
            hh.set_option(k, v)
        hh.close()


def load(h, cid, delta):
    c = J.CASES[cid]
    X, Y, Xs = J.problem(cid)
    h.set_data(X, Y)
    h.set_params(J.KERNEL_ID[c.fam], 0, J.VAR, [J.LS], J.noise_of(delta))
    h.set_candidates(Xs)
    return c


def raw(h, entry, maxtries):
    """The return code of an entry point, and what it wrote."""
    lml, logdet, jit = _lib._fit_scalars()
    sc = (ctypes.byref(lml), ctypes.byref(logdet), ctypes.byref(jit))
    if entry == "fit":
        rc = h.lib.gp_fit(h.h, maxtries, *sc)
        out = ()
    elif entry == "fit_predict":
        mean, var = np.empty((h.M, h.P)), np.empty((h.M, 1))
        rc = h.lib.gp_fit_predict(h.h, maxtries, 1, *sc, _lib.dptr(mean), _lib.dptr(var))
        out = (mean, var)
    else:
        dv, dn, dl = ctypes.c_double(), ctypes.c_double(), np.empty(1)
        rc = h.lib.gp_fit_grad(h.h, maxtries, *sc, ctypes.byref(dv), _lib.dptr(dl), ctypes.byref(dn))
        out = (np.array([dv.value]), dl, np.array([dn.value]))
    return rc, (lml.value, logdet.value, jit.value), out


def run(h, entry):
    """An entry point that must succeed: (scalars, arrays) as bytes-comparable tuples."""
    rc, sc, out = raw(h, entry, J.MAXTRIES)
    assert rc == 0, (entry, rc)
    return sc, out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- A: the oracle ----------------------------------------------------------------------------------------------------------------
def check_scalars(tag, got, p):
    lml, logdet, jit = got
    e = (abs(jit - p["jitter"]) / p["jitter"], abs(lml - p["lml"]) / max(1.0, abs(p["lml"])),
         abs(logdet - p["logdet"]) / max(1.0, abs(p["logdet"])))
    print("jitter_routes: %-34s jitter %.1e lml %.1e logdet %.1e" % ((tag,) + e))
    assert e[0] <= 1e-12 and e[1] <= 1e-8 and e[2] <= 1e-8
    return e


def check_posterior(tag, h, gp, Xs, full):
    """alpha, the candidates' posterior and the LML gradient of the resident fit against the oracle ``gp``; with ``full`` also the
    full covariance of a 128-row slice, Ky^-1, the predictive gradients, fmin on both routes and the one-location calls."""
    p = gp.posterior
    P = gp.Y.shape[1]
    err = {"alpha": relmax(h.alpha(), p["alpha"])}
    mu, v = h.predict(True)
    m0, v0 = gp.predict(Xs)
    err["mean"], err["var"] = relmax(mu, m0), float(np.max(np.abs(v - v0) / np.abs(v0)))
    mu2, v2 = h.predict(False)
    m1, v1 = gp.predict_noiseless(Xs)
    err["mean0"] = relmax(mu2, m1)
    err["var0"] = float(np.max(np.abs(v2 - v1)))
    var0_bound = 1e-6 * max(1.0, np.max(np.abs(v1))) + 1e-9            # the sweep's criterion (tests/test_gpu_random_shapes.py)
    dv, dl, dn = h.lml_grad(1)
    r = gp.gradients()
    sc = max(1.0, abs(r[0]), np.max(np.abs(r[1])), abs(r[2]))
    err["lml_grad"] = max(abs(dv - r[0]), float(np.max(np.abs(dl - r[1]))), abs(dn - r[2])) / sc
    if full:
        Wi = h.woodbury_inv()
        err["Wi"] = float(np.max(np.abs(Wi - p["Wi"])) / np.max(np.abs(p["Wi"])))
    if full and P == 1:
        dm, dvx = h.predict_grad()
        dm0, dv0 = gp.predictive_gradients(Xs)
        err["dmean"] = float(np.max(np.abs(dm - dm0)) / max(1.0, np.max(np.abs(dm0))))
        err["dvar"] = float(np.max(np.abs(dvx - dv0)) / max(1.0, np.max(np.abs(dv0))))
        model = O.OracleGPModel(gp)
        f0 = model.get_fmin()
        fmin = h.fmin()
        err["fmin"] = abs(fmin - f0) / max(1.0, abs(f0))
        h.set_option("fmin_direct", 1)
        try:
            err["fmin_direct"] = abs(h.fmin() - f0) / max(1.0, abs(f0))
        finally:
            h.set_option("fmin_direct", 0)
        err["rows"] = err["rows_grad"] = err["ei"] = err["ei_grad"] = 0.0
        for k in (1, 3, 5):                                              # Xs[0] is the duplicated point itself
            xs = Xs[:k]
            mr, vr, dmr, dvr = h.predict_rows(xs, True, grad=True)
            err["rows"] = max(err["rows"], relmax(mr, m0[:k]), float(np.max(np.abs(vr - v0[:k]) / np.abs(v0[:k]))))
            err["rows_grad"] = max(err["rows_grad"], float(np.max(np.abs(dmr - dm0[:k])) / max(1.0, np.max(np.abs(dm0)))),
                                   float(np.max(np.abs(dvr - dv0[:k])) / max(1.0, np.max(np.abs(dv0)))))
            a0, da0 = O.acq_EI_withGradients(model, xs, 0.01, f0)
            ar, dar = h.acq_rows(xs, _lib.GP_ACQ_EI, 0.01, fmin, grad=True)
            err["ei"] = max(err["ei"], float(np.max(np.abs(ar + a0)) / max(1.0, np.max(np.abs(a0)))))
            err["ei_grad"] = max(err["ei_grad"], float(np.max(np.abs(dar + da0)) / max(1.0, np.max(np.abs(da0)))))
    if full:
        # gp_predict_full_cov keeps its candidates in one chunk: a 128-row slice of the table, the duplicated point in it
        h.set_candidates(Xs[:128])
        try:
            _, cf = h.predict_full_cov(True)
            _, c0 = gp.predict(Xs[:128], full_cov=True)
            err["full_cov"] = float(np.max(np.abs(cf - c0)) / max(1.0, np.max(np.abs(c0))))
        finally:
            h.set_candidates(Xs)
    print("jitter_routes: %-34s %s" % (tag, " ".join("%s %.1e" % kv for kv in sorted(err.items()))))
    assert err.pop("var0") < var0_bound
    assert err.pop("ei_grad", 0.0) < 1e-5
    for k, e in err.items():
        assert e < 1e-6, (k, e)


@pytest.mark.parametrize("cid,delta", J.SINGLE, ids=lambda v: str(v))
def test_single_stream_against_the_oracle(h, cid, delta):
    """lookahead = 0.  Everything at panel_tiles = 3 (b = 383 / 384 sit on either side of a panel edge, 1279 in the one-tile last
    panel); the scalars, alpha and the candidates' posterior at panel_tiles = 1 as well."""
    c = load(h, cid, delta)
    gp = J.oracle(cid, delta)
    Xs = J.problem(cid)[2]
    for W in (3, 1):
        tag = "single-W%d %s %g" % (W, cid, delta)
        with route(h, single(W)):
            sc = h.fit()
            check_scalars(tag, sc, gp.posterior)
            assert h.fit_state() == sc
            check_posterior(tag, h, gp, Xs, full=(W == 3))


# ---- B + C: routes ---------------------------------------------------------------------------------------------------------------
_BASE = {}


def baseline(h, cid, delta, W):
    """The single-stream results of a case at panel width W through the separate calls: computed once, never changed."""
    key = (cid, delta, W)
    if key not in _BASE:
        load(h, cid, delta)
        with route(h, single(W)):
            sc = h.fit()
            ref = dict(sc=sc, L=h.chol(), alpha=h.alpha(), pred=h.predict(True), grad=h.lml_grad(1))
        for a in (ref["L"], ref["alpha"]) + tuple(ref["pred"]):
            a.setflags(write=False)
        _BASE[key] = ref
    return _BASE[key]


def check_codes(h, c, delta, entries=ENTRIES):
    """C: too few attempts return LAPACK's info on the first duplicate row, exactly enough succeed on the table's rung."""
    need = J.TRIES[delta]
    for entry in entries:
        for mt in range(need):
            rc, _, _ = raw(h, entry, mt)
            assert rc == J.first_pivot(c) + 1, (entry, mt, rc)
        rc, sc, _ = raw(h, entry, need)
        assert rc == 0 and abs(sc[2] - J.rung(delta, need)) <= 1e-12 * sc[2], (entry, rc, sc)


def _route_cases():
    out = [(name, cid, J.DELTA) for name in sorted(LA) for cid in J.MULTI]
    out += [(FULL_DELTAS_ROUTE, c.id, d) for c in J.TABLE if c.multi for d in c.deltas if d != J.DELTA]
    return out


@pytest.mark.parametrize("name,cid,delta", _route_cases(), ids=lambda v: str(v))
def test_lookahead_routes_equal_the_single_stream_bits_under_jitter(h, name, cid, delta):
    """Attempts that fail behind released stages, inverted panels built from a failed factor, owned columns: after the rung that
    passes, the factor, alpha, the LML, the jitter, the posterior and the gradients are BITWISE those of lookahead = 0 at the same
    panel width -- the invariant tests/test_gpu_lookahead.py holds at jitter 0."""
    W, opts = LA[name]
    ref = baseline(h, cid, delta, W)
    c = load(h, cid, delta)
    with route(h, opts):
        check_codes(h, c, delta)
        assert h.fit() == ref["sc"] and ref["sc"][2] > 0.0
        assert np.array_equal(h.chol(), ref["L"]) and np.array_equal(h.alpha(), ref["alpha"])
        assert same(h.predict(True), ref["pred"])
        sc, (mu, var) = run(h, "fit_predict")
        assert sc == ref["sc"] and np.array_equal(mu, ref["pred"][0]) and np.array_equal(var, ref["pred"][1])
        assert np.array_equal(h.chol(), ref["L"]) and np.array_equal(h.alpha(), ref["alpha"])
        sc, (dv, dl, dn) = run(h, "fit_grad")
        assert sc == ref["sc"]
        assert dv[0] == ref["grad"][0] and np.array_equal(dl, ref["grad"][1]) and dn[0] == ref["grad"][2]
        assert np.array_equal(h.chol(), ref["L"]) and np.array_equal(h.alpha(), ref["alpha"])
        # Ky^-1 of gp_fit_grad's pipe (wi_valid, w_in_t2) belongs to the attempt that succeeded
        got = h.lml_grad(1)
        assert got[0] == ref["grad"][0] and np.array_equal(got[1], ref["grad"][1]) and got[2] == ref["grad"][2]


@pytest.mark.parametrize("cid", J.MULTI)
@pytest.mark.parametrize("name", ["single-W1", "single-W3"])
def test_single_stream_return_codes(h, name, cid):
    c = load(h, cid, J.DELTA)
    with route(h, ROUTES[name]):
        check_codes(h, c, J.DELTA)


@pytest.mark.parametrize("cid,delta", [(c.id, d) for c in J.TABLE if not c.multi for d in c.deltas], ids=lambda v: str(v))
def test_ragged_rows_return_codes(h, cid, delta):
    """N = 257 and 385: the failing pivot is the only row of the last tile, 127 padding rows (rows of the identity) follow it."""
    c = load(h, cid, delta)
    with route(h, single(1)):
        check_codes(h, c, delta)
    with route(h, single(3)):
        check_codes(h, c, delta)


@pytest.mark.parametrize("cid", J.MULTI)
@pytest.mark.parametrize("name", sorted(HELD))
def test_other_arithmetic_routes_against_the_oracle(h, name, cid):
    """inner_tiles = 2 (potrf_pair_kernel, trsm2_kernel) and the emulated trailing update (rns_prepare scales the fixed point per
    attempt) contract in another order: return codes as everywhere, results at the bounds of A through all three entry points."""
    c = load(h, cid, J.DELTA)
    gp = J.oracle(cid, J.DELTA)
    p = gp.posterior
    Xs = J.problem(cid)[2]
    tag = "%s %s" % (name, cid)
    with route(h, ROUTES[name]):
        check_codes(h, c, J.DELTA)
        check_scalars(tag + " fit", h.fit(), p)
        check_posterior(tag + " fit", h, gp, Xs, full=False)
        sc, (mu, var) = run(h, "fit_predict")
        check_scalars(tag + " fit_predict", sc, p)
        m0, v0 = gp.predict(Xs)
        assert relmax(mu, m0) < 1e-6 and np.max(np.abs(var - v0) / np.abs(v0)) < 1e-6
        assert relmax(h.alpha(), p["alpha"]) < 1e-6
        sc, (dv, dl, dn) = run(h, "fit_grad")
        check_scalars(tag + " fit_grad", sc, p)
        r = gp.gradients()
        s = max(1.0, abs(r[0]), np.max(np.abs(r[1])), abs(r[2]))
        assert abs(dv[0] - r[0]) < 1e-6 * s and np.max(np.abs(dl - r[1])) < 1e-6 * s and abs(dn[0] - r[2]) < 1e-6 * s
        check_posterior(tag + " fit_grad", h, gp, Xs, full=False)
        if "emulate_fp64" in ROUTES[name]:       # the residue GEMM did run: every attempt's trailing update goes through it
            h.profile(1)
            try:
                n0 = h.rns_stats()["launches"]
                assert h.fit()[2] == sc[2]
                assert h.rns_stats()["launches"] >= n0 + 1 + J.TRIES[J.DELTA]
            finally:
                h.profile(0)


# ---- C + D: what a failure leaves behind ------------------------------------------------------------------------------------------
D_CASE = "mid"
GOOD_NOISE = 1e-2


def refused_calls(h, Xs):
    """The return codes of the calls that need a fit."""
    lib, one = h.lib, np.zeros((8, 8))
    d = [ctypes.c_double() for _ in range(3)]
    mean, var = np.empty((h.M, h.P)), np.empty((h.M, 1))
    buf = np.empty((h.N, h.P))
    xr = np.ascontiguousarray(Xs[:2])
    ynew = np.zeros((h.N + 1, h.P))
    return {
        "gp_predict": lib.gp_predict(h.h, 1, _lib.dptr(mean), _lib.dptr(var)),
        "gp_get_alpha": lib.gp_get_alpha(h.h, _lib.dptr(buf)),
        "gp_lml_grad": lib.gp_lml_grad(h.h, ctypes.byref(d[0]), _lib.dptr(one), ctypes.byref(d[1])),
        "gp_fmin": lib.gp_fmin(h.h, ctypes.byref(d[2])),
        "gp_append": lib.gp_append(h.h, _lib.dptr(xr), 1, _lib.dptr(ynew), None, None),
        "gp_predict_rows": lib.gp_predict_rows(h.h, xr.ctypes.data, 1, 1, mean.ctypes.data, var.ctypes.data, None, None),
        "gp_es_set_representers": lib.gp_es_set_representers(h.h, _lib.dptr(xr), 2, 0.0, 1.0, _lib.dptr(one), _lib.dptr(one[1:])),
    }


def good_fit(h, entry, Xs):
    """A well-conditioned fit through ``entry`` and everything read from it, as comparable arrays."""
    c = J.CASES[D_CASE]
    h.set_params(J.KERNEL_ID[c.fam], 0, J.VAR, [J.LS], GOOD_NOISE)
    sc, out = run(h, entry)
    rows = h.predict_rows(Xs[:3], True, grad=True)
    return (np.array(sc),) + tuple(out) + (h.chol(), h.alpha()) + tuple(h.predict(True)) + tuple(rows)


@pytest.fixture(scope="module")
def fresh():
    """What a fresh context returns for set_data, set_params (noise 1e-2), set_candidates and one entry point, per route."""
    memo = {}

    def get(name, entry):
        if (name, entry) not in memo:
            X, Y, Xs = J.problem(D_CASE)
            f = _lib.Handle(0)
            try:
                for k, v in ROUTES[name].items():
                    f.set_option(k, v)
                f.set_data(X, Y)
                f.set_params(J.KERNEL_ID[J.CASES[D_CASE].fam], 0, J.VAR, [J.LS], GOOD_NOISE)
                f.set_candidates(Xs)
                memo[name, entry] = good_fit(f, entry, Xs)
            finally:
                f.close()
        return memo[name, entry]
    return get


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(ROUTES))
def test_what_a_failed_and_a_jittered_fit_leave_behind(h, fresh, name, entry):
    c = J.CASES[D_CASE]
    Xs = J.problem(D_CASE)[2]
    want = fresh(name, entry)
    with route(h, ROUTES[name]):
        # the diagonal is not positive: before any ladder
        load(h, D_CASE, J.DELTA)
        h.set_params(J.KERNEL_ID[c.fam], 0, J.VAR, [J.LS], -2.0)
        assert raw(h, entry, J.MAXTRIES)[0] == _lib.GP_ERR_NOT_PD_DIAG
        # five attempts do not save delta = 0.5
        h.set_params(J.KERNEL_ID[c.fam], 0, J.VAR, [J.LS], J.noise_of(J.DELTA_FAILS))
        rc = raw(h, entry, J.MAXTRIES)[0]
        assert 0 < rc <= c.N, rc
        assert set(refused_calls(h, Xs).values()) == {_lib.GP_ERR_STATE}
        # an exhausted ladder at delta = 3e-5 (attempts behind released stages, inverted panels of a failed factor)
        load(h, D_CASE, J.DELTA)
        assert raw(h, entry, J.TRIES[J.DELTA] - 1)[0] == J.first_pivot(c) + 1
        codes = refused_calls(h, Xs)
        assert set(codes.values()) == {_lib.GP_ERR_STATE}, codes
        assert h.M == c.M                         # the candidates stay resident: nothing below sets them again
        assert same(good_fit(h, entry, Xs), want)
        assert h.fit_state()[2] == 0.0
        # a jittered success, then the same well-conditioned fit
        h.set_params(J.KERNEL_ID[c.fam], 0, J.VAR, [J.LS], J.noise_of(J.DELTA))
        sc, _ = run(h, entry)
        assert abs(sc[2] - J.rung(J.DELTA, J.TRIES[J.DELTA])) <= 1e-12 * sc[2]
        h.predict_rows(Xs[:3], True, grad=True)
        assert same(good_fit(h, entry, Xs), want)
        assert h.fit_state()[2] == 0.0


# ---- E: append --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rb", (1, 0))
@pytest.mark.parametrize("c", J.APPEND, ids=lambda c: c.id)
def test_append_to_a_jittered_fit(c, rb):
    """The border's diagonal carries the jitter of the fit (append.hip) and fmin's identity y - (noise + 1e-8 + jitter) alpha
    as well: against the oracle's refit of the grown data, which stops on the same rung (tests/test_jitter_cases_host.py)."""
    X, Y, Xs = J.append_problem(c.id)
    kern = J.kernel(c.fam)
    want = J.rung(J.DELTA, J.TRIES[J.DELTA])
    f = _lib.Handle(0)
    try:
        f.set_option("rows_build", rb)
        f.set_data(X[:c.N0], 0.5 * Y[:c.N0] + 0.3)
        f.set_params(J.KERNEL_ID[c.fam], 0, J.VAR, [J.LS], J.noise_of(J.DELTA))
        f.set_candidates(Xs)
        jit = f.fit()[2]
        assert abs(jit - want) <= 1e-12 * want
        f.predict(True)
        f.fmin()
        if rb:
            f.predict_rows(Xs[:1], True)
        lml, logdet = f.append(X[c.N0:], Y)
        assert f.fit_state() == (lml, logdet, jit)                       # the jitter of the fit stays
        gp = O.OracleGP(X, Y, kern, J.noise_of(J.DELTA))
        tag = "append %s rb%d" % (c.id, rb)
        check_scalars(tag, (lml, logdet, jit), gp.posterior)
        check_posterior(tag, f, gp, Xs, full=True)
    finally:
        f.close()


def _raw_append(h, Xn, k, Yall):
    return h.lib.gp_append(h.h, _lib.dptr(np.ascontiguousarray(Xn)), k, _lib.dptr(np.ascontiguousarray(Yall)), None, None)


def _state(h):
    return h.fit_state(), h.alpha().tobytes(), h.chol().tobytes()


@pytest.mark.parametrize("rb", (1, 0))
@pytest.mark.parametrize("c", J.BORDER, ids=lambda c: c.id)
def test_finite_border_that_is_not_positive_definite(c, rb):
    """New row j repeats training row a under Ky = K - delta I: the border's pivot is -2 delta, not a rounding matter.  The code
    is the 1-based row of the grown matrix, LAPACK's info; nothing of the context changes (for the split append the committed
    first border is taken back); the refit of the grown data lands on the oracle's rung; a clean append matches the oracle."""
    X, Xbad, Y, Xs = J.border_problem(c.id)
    kern = J.kernel(c.fam)
    f = _lib.Handle(0)
    try:
        f.set_option("rows_build", rb)
        f.set_data(X[:c.N0], Y[:c.N0])
        f.set_params(J.KERNEL_ID[c.fam], 0, J.VAR, [J.LS], J.noise_of(J.DELTA))
        f.set_candidates(Xs)
        assert f.fit()[2] == 0.0                                         # distinct rows: no jitter needed
        f.predict(True)
        if rb:
            f.predict_rows(Xs[:1], True)
        s = _state(f)
        rows0 = f.predict_rows(Xs[:2], True, grad=True)
        for n in (1, 2):
            assert _raw_append(f, Xbad, c.k, Y) == c.N0 + c.j + 1
            assert f.append_stats() == (0, 0, n)
            assert f.N == c.N0 and _state(f) == s
            assert all(a.tobytes() == b.tobytes() for a, b in zip(rows0, f.predict_rows(Xs[:2], True, grad=True)))
        with pytest.raises(np.linalg.LinAlgError):
            f.append(Xbad, Y)
        assert f.append_stats() == (0, 0, 3) and _state(f) == s
        # a clean append goes through and matches the oracle
        lml, logdet = f.append(X[c.N0:], Y)
        gp = O.OracleGP(X, Y, kern, J.noise_of(J.DELTA))
        assert f.fit_state()[2] == 0.0 and gp.posterior["jitter"] == 0.0
        assert abs(lml - gp.posterior["lml"]) <= 1e-8 * max(1.0, abs(gp.posterior["lml"]))
        assert abs(logdet - gp.posterior["logdet"]) <= 1e-8 * max(1.0, abs(gp.posterior["logdet"]))
        check_posterior("border %s rb%d clean" % (c.id, rb), f, gp, Xs, full=True)
        # the caller's way out of the refusal: set_data + fit of the grown data
        Xg = np.vstack([X[:c.N0], Xbad])
        f.set_data(Xg, Y)
        gpg = O.OracleGP(Xg, Y, kern, J.noise_of(J.DELTA))
        tag = "border %s rb%d refit" % (c.id, rb)
        check_scalars(tag, f.fit(), gpg.posterior)
        check_posterior(tag, f, gpg, Xs, full=False)
    finally:
        f.close()
